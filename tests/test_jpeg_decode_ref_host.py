"""CPU-only: pins tests/jpeg_decode_ref.py, the numpy restatement of the JPEG decoder of include/refid_hip.h, against PIL
(libjpeg-turbo with its defaults: islow IDCT, fancy upsampling) byte for byte, before the library's entropy stage
(tests/test_jpeg_entropy_host.py) and the GPU (tests/test_hip_jpeg_decode.py) are compared with it.  Integers only: every
comparison is exact equality."""
import io

import numpy as np
import pytest

import jpeg_decode_cases as K
import jpeg_decode_ref as R

SHAPES = [(1, 1), (8, 8), (16, 16), (17, 35), (33, 65), (37, 53), (8, 5), (9, 4), (5, 3), (20, 6), (7, 9), (2, 17)]
PIL_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
SETTINGS = [dict(quality=30), dict(quality=90), dict(quality=100), dict(quality=90, restart_marker_blocks=1),
            dict(quality=90, restart_marker_blocks=3), dict(quality=75, optimize=True)]


def _pil_decode(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def _pil_encode(frame, sampling, **options):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(frame).convert("L").save(buf, "JPEG", **options)
    else:
        Image.fromarray(frame).save(buf, "JPEG", subsampling=PIL_SUBSAMPLING[sampling], **options)
    return buf.getvalue()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_restatement_equals_pil_on_pils_files(shape):
    """Noise and smooth frames, every sampling, quality 30 / 90 / 100, restart markers every 1 and 3 MCUs, optimised tables."""
    h, w = shape
    for family in ("noise", "smooth"):
        frame = K.image(h, w, family, seed=h * 100 + w)
        for sampling in K.SAMPLINGS:
            for options in SETTINGS:
                data = _pil_encode(frame, sampling, **options)
                info = R.probe(data)
                assert (info.height, info.width, info.sampling) == (h, w, sampling), (family, sampling, options)
                assert info.restart_interval == options.get("restart_marker_blocks", 0)
                assert np.array_equal(R.decode(data), _pil_decode(data)), (family, sampling, options)


def test_the_restatement_equals_pil_on_the_encoders_files():
    for name, data in K.own_files().items():
        assert np.array_equal(R.decode(data), _pil_decode(data)), name


def test_a_file_without_dht_decodes_with_the_annex_k_tables_as_pil_does():
    for sampling in K.SAMPLINGS:
        whole = _pil_encode(K.image(17, 35, "noise", 3), sampling, quality=90)
        data = K.strip_dht(whole)
        assert b"\xff\xc4" in whole and len(data) < len(whole) - 200 and 0xc4 not in [m for m, _ in K.split(data)[0]]
        want = _pil_decode(data)
        assert np.array_equal(want, _pil_decode(whole)) and np.array_equal(R.decode(data), want), sampling


def test_the_restatement_equals_the_stored_pil_pixels_of_the_golden_cases():
    """tests/golden/jpeg_decode_cases.npz (tools/make_jpeg_decode_golden.py) holds PIL's pixels: this needs no PIL."""
    cases = K.golden()
    assert len(cases) >= 12 and {R.probe(d).sampling for d, _ in cases.values()} == set(K.SAMPLINGS)
    assert any(R.probe(d).restart_interval for d, _ in cases.values())
    assert any(0xc4 not in [m for m, _ in K.split(d)[0]] for d, _ in cases.values())
    assert {3, 4, 5} <= {R.probe(d).width for d, _ in cases.values()}
    for name, (data, rgb) in cases.items():
        assert np.array_equal(R.decode(data), rgb), name


def test_the_idct_wraps_like_a_32_bit_register():
    """Coefficients of +-2047 under quantisers of 255 overflow int32 in the column pass: the restatement wraps, and an
    independent plain-Python evaluation with explicit masking agrees."""
    coefs, quant = K.coefficients(8, 8, "grey", "extreme", seed=5)

    def wrap(v):
        return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)

    def idct8(i, shift):
        z1 = wrap(wrap(i[2] + i[6]) * 4433)
        t2, t3 = wrap(z1 - wrap(i[6] * 15137)), wrap(z1 + wrap(i[2] * 6270))
        t0, t1 = wrap(wrap(i[0] + i[4]) << 13), wrap(wrap(i[0] - i[4]) << 13)
        e = [wrap(t0 + t3), wrap(t1 + t2), wrap(t1 - t2), wrap(t0 - t3)]
        a, b, c, d = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = wrap(a + d), wrap(b + c), wrap(a + c), wrap(b + d)
        z5 = wrap(wrap(z3 + z4) * 9633)
        a, b, c, d = wrap(a * 2446), wrap(b * 16819), wrap(c * 25172), wrap(d * 12299)
        z1, z2, z3, z4 = wrap(-z1 * 7373), wrap(-z2 * 20995), wrap(wrap(-z3 * 16069) + z5), wrap(wrap(-z4 * 3196) + z5)
        o = [wrap(a + wrap(z1 + z3)), wrap(b + wrap(z2 + z4)), wrap(c + wrap(z2 + z3)), wrap(d + wrap(z1 + z4))]
        half = 1 << (shift - 1)
        return [wrap(wrap(e[k] + o[3 - k]) + half) >> shift for k in range(4)] + [wrap(wrap(e[3 - k] - o[k]) + half) >> shift for k in range(4)]

    x = [[wrap(int(coefs[0][8 * r + c]) * 255) for c in range(8)] for r in range(8)]
    cols = [idct8([x[r][c] for r in range(8)], 11) for c in range(8)]
    want = [[min(max(v + 128, 0), 255) for v in idct8([cols[c][r] for c in range(8)], 18)] for r in range(8)]
    assert R.idct_blocks(coefs[:1], quant[0])[0].tolist() == want
    assert any(abs(int(coefs[0][k]) * 255) << 13 > 2 ** 31 for k in range(64))
