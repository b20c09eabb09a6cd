"""CPU-only: tests/png_filter_ref.py (the forward PNG filters) pinned to the project's own decoder before the GPU test
relies on it -- files it writes decode through png.read_png to the original array, bit for bit; png.read_filtered returns
the rows whose _unfilter is read_png; the errors of the new route.  Sizes stay <= 65x33: _unfilter walks Average and Paeth
rows byte by byte in Python."""
import struct
import zlib

import numpy as np
import pytest

import png_filter_ref as R
from refid_amd import png

STRESS = [4, 4, 0, 4, 3, 1, 2, 4, 1, 1, 3]


def _image(shape, seed, high=256):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, high, shape, dtype=np.uint8)


def _programmes(h, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.full(h, t) for t in range(5)] + [rng.integers(0, 5, h), np.resize(STRESS, h)]


@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 7), (2, 1, 3), (5, 3, 3), (9, 17), (33, 20, 3), (65, 33, 3), (65, 33)])
def test_written_files_decode_to_the_original(tmp_path, shape):
    for high in (256, 4):                                   # 0..3: Paeth ties on almost every byte
        img = _image(shape, 5, high)
        for k, types in enumerate(_programmes(shape[0], 6) + [R.adaptive_types(img)]):
            path = R.write_filtered_png(str(tmp_path / f"{high}_{k}.png"), img, types)
            got = png.read_png(path)
            assert got.dtype == np.uint8 and got.shape == img.shape and np.array_equal(got, img), (high, k)
            w, h, ch, rows = png.read_filtered(path)
            assert (h, w) == shape[:2] and ch == (3 if len(shape) == 3 else 1)
            assert rows.dtype == np.uint8 and rows.shape == (h, 1 + w * ch) and np.array_equal(rows[:, 0], types)
            assert np.array_equal(rows, R.apply_filters(img, types))
            assert np.array_equal(png._unfilter(rows, ch).reshape(img.shape), got)


def test_wrap_modulo_256_and_the_average_needs_nine_bits(tmp_path):
    for img in (np.full((6, 5, 3), 255, np.uint8), (254 + (np.indices((7, 9)).sum(0) & 1)).astype(np.uint8)):
        for t in range(5):
            path = R.write_filtered_png(str(tmp_path / "w.png"), img, np.full(img.shape[0], t))
            assert np.array_equal(png.read_png(path), img), t


def test_adaptive_types_picks_the_least_sum(tmp_path):
    ramp = (np.arange(33, dtype=np.uint8)[None, :, None] * 3 + np.arange(20, dtype=np.uint8)[:, None, None] * 5 +
            np.arange(3, dtype=np.uint8)) .astype(np.uint8)
    types = R.adaptive_types(ramp)
    assert types.shape == (20,) and types.min() >= 0 and types.max() <= 4 and (types != 0).any()   # a ramp is never cheapest raw
    cost = lambda t: np.abs(R.apply_filters(ramp, np.full(20, t))[:, 1:].view(np.int8).astype(np.int64)).sum(axis=1)   # noqa: E731
    costs = np.stack([cost(t) for t in range(5)])
    assert np.array_equal(costs[types, np.arange(20)], costs.min(axis=0))
    assert np.array_equal(png.read_png(R.write_filtered_png(str(tmp_path / "r.png"), ramp, types)), ramp)


def test_find_bands_start_only_where_the_row_above_is_not_read():
    filters = np.array([[4, 4, 0, 4, 3, 1, 2, 4, 1, 1, 3], [2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]])
    assert png.find_bands(filters, 1).tolist() == [[0, 0, 2], [0, 2, 5], [0, 5, 8], [0, 8, 9], [0, 9, 11], [1, 0, 11]]
    assert png.find_bands(filters, 4).tolist() == [[0, 0, 5], [0, 5, 9], [0, 9, 11], [1, 0, 11]]
    assert png.find_bands(filters).tolist() == [[0, 0, 11], [1, 0, 11]]
    column = np.resize(STRESS, 200)
    for min_rows in (1, 7, 64):
        bands = png.find_bands(column[None], min_rows)
        assert bands.dtype == np.int32 and bands[0, 1] == 0 and bands[-1, 2] == 200
        assert np.array_equal(bands[1:, 1], bands[:-1, 2]) and (column[bands[1:, 1]] <= 1).all()
        assert (bands[:-1, 2] - bands[:-1, 1] >= min_rows).all()
    with pytest.raises(ValueError, match="unknown filter type 5 in row 1"):
        png.find_bands(np.array([[0, 5, 1]]))


def test_errors_of_the_filtered_route(tmp_path):
    img = _image((4, 5, 3), 9)
    rows = R.apply_filters(img, [1, 2, 3, 4])
    ihdr = struct.pack(">IIBBBBB", 5, 4, 8, 2, 0, 0, 0)

    def put(name, rows_bytes, head=ihdr):
        data = png.SIGNATURE + png._chunk(b"IHDR", head) + png._chunk(b"IDAT", zlib.compress(rows_bytes)) + png._chunk(b"IEND", b"")
        (tmp_path / name).write_bytes(data)
        return str(tmp_path / name)

    bad = rows.copy()
    bad[2, 0] = 7
    for reader in (png.read_png, png.read_filtered):        # the same ValueError on both routes
        with pytest.raises(ValueError, match="read_png: unknown filter type 7 in row 2"):
            reader(put("bad.png", bad.tobytes()))
        with pytest.raises(ValueError, match="read_png: image data has the wrong length"):
            reader(put("short.png", rows.tobytes()[:-1]))
        with pytest.raises(ValueError, match="read_png: image data has the wrong length"):
            reader(put("size.png", rows.tobytes(), struct.pack(">IIBBBBB", 5, 5, 8, 2, 0, 0, 0)))
        with pytest.raises(ValueError, match="only 8-bit RGB / grey"):
            reader(put("rgba.png", rows.tobytes(), struct.pack(">IIBBBBB", 5, 4, 8, 6, 0, 0, 0)))
        whole = open(put("ok.png", rows.tobytes()), "rb").read()
        (tmp_path / "cut.png").write_bytes(whole[:-20])
        with pytest.raises(ValueError, match="read_png: truncated chunk"):
            reader(str(tmp_path / "cut.png"))
        (tmp_path / "crc.png").write_bytes(whole[:40] + bytes([whole[40] ^ 1]) + whole[41:])
        with pytest.raises(ValueError, match="CRC mismatch"):
            reader(str(tmp_path / "crc.png"))
    assert np.array_equal(png.read_png(str(tmp_path / "ok.png")), img)


def test_load_png_frames_needs_a_gpu_device_and_sane_arguments(tmp_path):
    from refid_amd._lib import RefidHipError
    from refid_amd.sequence import PNG_WORKERS_MAX, load_png_frames
    assert PNG_WORKERS_MAX <= 16
    path = R.write_filtered_png(str(tmp_path / "a.png"), _image((3, 4, 3), 1), [0, 1, 2])
    with pytest.raises(RefidHipError, match="GPU device"):
        load_png_frames([path], device="cpu")
    with pytest.raises(RefidHipError, match="workers 17"):
        load_png_frames([path], workers=17)
    with pytest.raises(RefidHipError, match="no files"):
        load_png_frames([])


def test_a_pil_written_file_decodes_to_pils_own_decode(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(3))
    yy, xx = np.mgrid[0:40, 0:33]
    smooth = (96 + 60 * np.sin(xx / 7.0) + 50 * np.cos(yy / 5.0))[:, :, None] + np.array([0.0, 20.0, -30.0])
    img = np.clip(smooth + rng.normal(0, 3, smooth.shape), 0, 255).astype(np.uint8)
    for name, arr in (("rgb.png", img), ("grey.png", img[:, :, 1])):
        Image.fromarray(arr).save(tmp_path / name)
        want = np.asarray(Image.open(tmp_path / name))
        assert np.array_equal(want, arr)
        assert np.array_equal(png.read_png(str(tmp_path / name)), want)
        w, h, ch, rows = png.read_filtered(str(tmp_path / name))
        assert np.array_equal(png._unfilter(rows, ch).reshape(arr.shape), want)
