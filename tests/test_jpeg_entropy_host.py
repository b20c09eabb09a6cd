"""CPU-only: the host entropy stage of JPEG decode (csrc/jpeg_entropy.h through refid_jpeg_probe / refid_jpeg_entropy_decode)
against tests/jpeg_decode_ref.py -- header fields, coefficients and tables exactly --, every refusal of include/refid_hip.h
provoked by a hand-made or mutated file with its message checked by word, truncation at every byte offset, and the same
code as a stand-alone program under the host address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_decode_cases as K
import jpeg_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library(data):
    """('ok', info, coefs, quant) or ('refused', message) from the library."""
    from refid_amd import jpeg
    from refid_amd._lib import RefidHipError
    try:
        info = jpeg.probe(data)
        coefs = np.full((info.total_blocks, 64), 0x5a5a, dtype=np.int16)
        quant = np.full((info.components, 64), 0x5a5a, dtype=np.uint16)
        jpeg.entropy_decode(data, info, coefs, quant)
    except RefidHipError as e:
        message = str(e).split(": ", 1)[1]
        assert message.startswith("jpeg_decode: "), message
        return ("refused", message)
    return ("ok", info, coefs, quant)


def _reference(data):
    try:
        return ("ok",) + R.entropy_decode(data)
    except R.Refused as e:
        return ("refused", str(e))


def _same(a, b):
    return a[0] == b[0] == "ok" and tuple(a[1]) == tuple(b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def _valid_files():
    files = {name: data for name, (data, _) in K.golden().items()}
    files.update(K.own_files())
    return files


def test_probe_and_entropy_decode_equal_the_restatement():
    for name, data in _valid_files().items():
        got, want = _library(data), _reference(data)
        assert _same(got, want), (name, got[:2], want[:2])
        info = got[1]
        blocks, total = R.blocks_of(info.height, info.width, K.CODES[info.sampling])
        assert list(info.blocks) == blocks and info.total_blocks == total and got[2].dtype == np.int16 and got[3].dtype == np.uint16


def test_fill_bytes_app_segments_and_split_tables_are_accepted():
    data = K.golden()["s420_17x35_q90"][0]
    want = _reference(data)
    segs, tail = K.split(data)
    padded = bytearray(b"\xff\xd8")
    for m, p in [(0xe1, b"Exif\0\0" + bytes(40)), (0xfe, b"a comment")] + segs:
        if m == 0xc4 and len(p) > 17 + sum(p[1:17]):                # several tables in one DHT: one segment each
            at = 0
            while at < len(p):
                n = 17 + sum(p[at + 1:at + 17])
                padded += b"\xff\xff\xff\xc4" + bytes([(n + 2) >> 8, (n + 2) & 255]) + p[at:at + n]
                at += n
            continue
        padded += b"\xff\xff" + bytes([m, (len(p) + 2) >> 8, (len(p) + 2) & 255]) + p
    assert _same(_library(bytes(padded) + tail), want)
    # a table defined twice: the later one holds
    dqt = [s for s in segs if s[0] == 0xdb][0]
    wrong = (0xdb, K.put(dqt[1], 1, [7] * 64))
    assert _same(_library(K.join([wrong] + segs, tail)), want)
    # fill bytes in front of a restart marker
    rst = K.golden()["s420_33x65_q30_rst3"][0]
    head, scan = K.split(rst)
    assert b"\xff\xd0" in scan
    assert _same(_library(K.join(head, scan.replace(b"\xff\xd0", b"\xff\xff\xff\xd0"))), _reference(rst))


def _sof(data, at, values, marker=None):
    return K.edit(data, 0xc0, lambda p: K.put(p, at, values), marker)


def _refusals():
    """[(name, file, a word of the library's message)]"""
    base = K.golden()["s420_17x35_q90"][0]
    rst = K.golden()["s420_33x65_q30_rst3"][0]
    segs, tail = K.split(base)
    one = {1: [0]}                                                  # a table with the single code '0' for symbol 0
    out = [
        ("progressive", _sof(base, 0, [8], 0xc2), "progressive (SOF2)"),
        ("sof1", _sof(base, 0, [8], 0xc1), "extended sequential (SOF1)"),
        ("arithmetic", _sof(base, 0, [8], 0xc9), "arithmetic coding"),
        ("dac", K.join([(0xcc, bytes([0, 0]))] + segs, tail), "arithmetic coding (DAC)"),
        ("twelve_bit", _sof(base, 0, [12]), "sample precision 12"),
        ("four_components", K.edit(base, 0xc0, lambda p: K.put(p, 5, [4]) + bytes([4, 0x11, 1])), "4 components"),
        ("two_components", K.edit(base, 0xc0, lambda p: K.put(p[:-3], 5, [2])), "2 components"),
        ("sampling_1x2", _sof(base, 7, [0x12]), "sampling 1x2 1x1 1x1"),
        ("sampling_chroma", _sof(base, 10, [0x21]), "sampling 2x2 2x1 1x1"),
        ("sampling_4x1", _sof(base, 7, [0x41]), "sampling 4x1"),
        ("non_interleaved", K.edit(base, 0xda, lambda p: bytes([1, 1, 0x00, 0, 63, 0])), "non-interleaved scan: 1 of the frame's 3"),
        ("progressive_scan", K.edit(base, 0xda, lambda p: K.put(p, len(p) - 3, [0, 5, 0])), "progressive scan"),
        ("dqt16", K.join([(0xdb, bytes([0x10]) + bytes(128))] + segs, tail), "16-bit quantisation table"),
        ("rgb_ids", K.edit(K.edit(base, 0xc0, lambda p: K.put(K.put(K.put(p, 6, [82]), 9, [71]), 12, [66])),
                           0xda, lambda p: K.put(K.put(K.put(p, 1, [82]), 3, [71]), 5, [66])), "RGB-coded file (component ids R G B)"),
        ("adobe_rgb", K.join([(0xee, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0]))] + segs, tail), "RGB-coded file (Adobe transform 0)"),
        ("height_0", _sof(base, 1, [0, 0]), "dimensions of 0"),
        ("width_0", _sof(base, 3, [0, 0]), "dimensions of 0"),
        ("no_dqt", K.join([s for s in segs if s[0] != 0xdb], tail), "quantisation table 0 is not defined"),
        ("huffman_slot", K.edit(base, 0xda, lambda p: K.put(p, 2, [0x22])), "Huffman table that is not defined"),
        ("segment_past_end", base[:20] + bytes([0xff, 0xfe, 0xff, 0xf0]) + base[20:24], "passes the end of the file"),
        ("no_soi", b"\x00" + base[1:], "no SOI"),
        ("eoi_first", base[:2] + b"\xff\xd9" + base[2:], "EOI before SOS"),
        ("wrong_rst", rst.replace(b"\xff\xd0", b"\xff\xd1", 1), "wrong RST number: found marker D1, expected RST0"),
        ("missing_rst", rst.replace(b"\xff\xd0", b"", 1), None),
        ("bytes_before_rst", rst.replace(b"\xff\xd1", b"\x55\xaa\xff\xd1", 1), "bytes are left over in front of RST1"),
        ("code_not_in_table", K.grey_file(8, 8, one, one, "1" * 32), "Huffman code that is not in the DC table"),
        ("ac_code_not_in_table", K.grey_file(8, 8, one, one, "0" + "1" * 32), "Huffman code that is not in the AC table"),
        ("dc_category_12", K.grey_file(8, 8, {1: [12]}, one, "0" * 32), "DC category of 12, above 11"),
        ("ac_category_11", K.grey_file(8, 8, one, {1: [0x0b]}, "0" * 32), "AC category of 11, above 10"),
        ("dc_leaves_int16", K.grey_file(8, 8 * 17, {1: [11]}, one, ("0" + "1" * 11 + "0") * 17), "DC value of 34799 leaves int16"),
        ("run_past_63", K.grey_file(8, 8, one, {1: [0xf1]}, "0" + "01" * 4), "zero run past coefficient 63"),
        ("zrl_past_63", K.grey_file(8, 8, one, {1: [0xf0]}, "0" + "0" * 4), "zero run past coefficient 63"),
        ("too_many_codes", K.join([(0xc4, bytes([0x00]) + bytes([3] + [0] * 15) + bytes([0, 1, 2]))] + segs, tail), "more codes of a length"),
        ("ends_early", K.grey_file(8, 16, one, one, "00"), "ends before the last MCU (MCU 1 of 2)"),
        ("marker_in_data", K.join(segs, tail[:10] + b"\xff\xd9"), "ends before the last MCU"),
    ]
    return out


def test_every_refusal_has_its_message_and_the_restatement_refuses_too():
    seen = set()
    for name, data, word in _refusals():
        got, want = _library(data), _reference(data)
        assert got[0] == "refused" and want[0] == "refused", (name, got[:2], want[:2])
        assert word is None or word in got[1], (name, got[1])
        seen.add(name)
    assert len(seen) >= 30
    # the hand-made files are well-formed up to the one thing that is wrong with each: their sound versions decode
    one = {1: [0]}
    ok = _library(K.grey_file(8, 16, one, one, "0000"))
    assert ok[0] == "ok" and not ok[2].any() and _same(ok, _reference(K.grey_file(8, 16, one, one, "0000")))
    ok = _library(K.grey_file(8, 8 * 16, {1: [11]}, one, ("0" + "1" * 11 + "0") * 16))
    assert ok[0] == "ok" and ok[2][:, 0].tolist() == [2047 * (k + 1) for k in range(16)]
    ok = _library(K.grey_file(8, 8, one, {1: [0xf1], 2: [0]}, "0" + "01" * 3 + "10"))
    assert ok[0] == "ok" and np.flatnonzero(ok[2][0]).tolist() == sorted(int(R.J.ZIGZAG[k]) for k in (16, 32, 48))


def test_a_file_that_does_not_match_the_expected_header_is_refused():
    from refid_amd import jpeg
    from refid_amd._lib import RefidHipError
    a, b = K.golden()["s420_17x35_q90"][0], K.golden()["s422_17x35_q90"][0]
    info = jpeg.probe(a)
    coefs, quant = np.zeros((info.total_blocks, 64), dtype=np.int16), np.zeros((3, 64), dtype=np.uint16)
    with pytest.raises(RefidHipError, match="jpeg_decode: the file is 17x35, 3 components, sampling 2.* expected 17x35, 3, 3"):
        jpeg.entropy_decode(b, info, coefs, quant)
    for bad_coefs, bad_quant in ((coefs[:-1], quant), (coefs.astype(np.int32), quant), (coefs, quant.astype(np.int16)), (coefs[:, ::-1], quant)):
        with pytest.raises(RefidHipError, match="jpeg.entropy_decode: .* must be a writeable C-contiguous"):
            jpeg.entropy_decode(a, info, bad_coefs, bad_quant)
    with pytest.raises(RefidHipError, match="jpeg.probe: jpeg_decode: no SOI"):
        jpeg.probe(b"")


def test_truncation_at_every_byte_offset_gives_the_right_answer_or_a_clean_refusal():
    data = K.golden()["s420_17x35_q90"][0]
    whole = _library(data)
    assert whole[0] == "ok"
    ok_from = None
    for n in range(len(data)):
        got = _library(data[:n])
        if got[0] == "ok":
            assert _same(got, whole), n
            ok_from = n if ok_from is None else ok_from
        else:
            assert ok_from is None, (n, got)                         # once enough bytes are there, more never hurt
        if n % 16 == 0 or got[0] == "ok":
            assert _reference(data[:n])[0] == got[0], n
    assert ok_from is not None and len(data) - 4 <= ok_from <= len(data) - 2      # only the padding bits and EOI may be missing


def test_entropy_decode_runs_from_several_threads_at_once():
    files = list(_valid_files().values()) * 4
    want = [_library(d) for d in files[:len(files) // 4]] * 4
    with ThreadPoolExecutor(max_workers=8) as pool:
        got = list(pool.map(_library, files))
    assert all(_same(g, w) for g, w in zip(got, want))


def _checksum(result):
    info = result[1]
    fields = [info.height, info.width, info.components, K.CODES[info.sampling], *info.blocks, info.total_blocks, info.restart_interval]
    values = np.concatenate([np.asarray(fields, dtype=np.uint32).astype(np.uint64), result[2].reshape(-1).view(np.uint16).astype(np.uint64),
                             result[3].reshape(-1).astype(np.uint64)])
    with np.errstate(over="ignore"):
        return int(((values + np.uint64(1)) * (np.uint64(2) * np.arange(values.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def test_the_entropy_stage_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/jpeg_entropy_check.cpp -- a stand-alone main around csrc/jpeg_entropy.h -- built with -fsanitize=address,undefined
    and run over the valid files, every truncation of one and a few hundred seeded byte mutations: exit status 0, no
    sanitizer report, and the library's checksums and refusals line for line.  Host code only."""
    compiler = shutil.which("g++") or shutil.which("clang++") or next(
        (p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_entropy_check")
    subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    files = dict(_valid_files())
    files.update((name, data) for name, data, _ in _refusals())
    base = K.golden()["s420_33x65_q30_rst3"][0]
    files.update((f"cut_{n:04d}", base[:n]) for n in range(len(base)))
    rng = np.random.default_rng(11)
    seeds = list(_valid_files().values())
    for k in range(400):
        data = bytearray(seeds[k % len(seeds)])
        for _ in range(int(rng.integers(1, 4))):
            data[int(rng.integers(2, len(data)))] = int(rng.integers(0, 256))
        files[f"mutated_{k:03d}"] = bytes(data)
    paths = []
    for name, data in files.items():
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            f.write(data)
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(paths)
    outcomes = set()
    for line, path, data in zip(lines, paths, files.values()):
        got_path, got = line.split("\t", 1)
        want = _library(data)
        outcomes.add(want[0])
        assert got_path == path and got == (f"{_checksum(want):016x}" if want[0] == "ok" else "refused: " + want[1]), (path, got, want[:2])
    assert outcomes == {"ok", "refused"}
