"""The input streams that test_deflate_ref_host.py and test_hip_png_deflate.py share, and their expected zlib streams from
tests/deflate_ref.py: built once per (case, block size), read-only.  A case is a uint8 array (streams, bytes)."""
import functools

import numpy as np

import deflate_ref as D
import png_filter_ref as R
from test_hip_png_filter import FAMILIES, _frame

ROW_SHAPES = [(1, 1), (2, 3), (17, 35), (65, 33), (130, 21), (5, 1367)]
BLOCKS = [1, 64, 257, 4096, 65535, D.DEFAULT_BLOCK_BYTES]
CASES = ["x".join(map(str, s)) for s in ROW_SHAPES] + ["fibonacci", "all256"]


def adaptive_rows(img):
    return R.apply_filters(img, R.adaptive_types(img))


@functools.lru_cache(maxsize=None)
def frames_of(h, w):
    rng = np.random.Generator(np.random.PCG64(100 * h + w))
    frames = np.stack([_frame(f, h, w, rng) for f in FAMILIES])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def streams(case):
    """uint8 (n, bytes).  'HxW': the adaptive rows of the nine families' frames; 'fibonacci': 17 byte values with the
    frequencies 1, 2, 3, 5, 8, ... 2584 (6763 bytes, shuffled) -- with end-of-block's 1 the merge is one chain 17 deep, past the
    15-bit limit; 'all256': every byte value, four of them often (a dynamic block that uses all 257 symbols)."""
    rng = np.random.Generator(np.random.PCG64(11))
    if case == "fibonacci":
        fib = [1, 2]
        while len(fib) < 17:
            fib.append(fib[-1] + fib[-2])
        data = np.concatenate([np.full(f, 7 * k + 3, dtype=np.uint8) for k, f in enumerate(fib)])
        out = rng.permutation(data)[None]
    elif case == "all256":
        data = np.concatenate([np.arange(256), rng.integers(0, 4, 3000)]).astype(np.uint8)
        out = rng.permutation(data)[None]
    else:
        h, w = map(int, case.split("x"))
        out = np.stack([adaptive_rows(img).reshape(-1) for img in frames_of(h, w)])
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(case, block_bytes):
    """([stream bytes per input stream], [block records per input stream]) from the restatement."""
    outs, infos = [], []
    for data in streams(case):
        info = []
        outs.append(D.deflate(data, block_bytes, info))
        infos.append(info)
    return outs, infos
