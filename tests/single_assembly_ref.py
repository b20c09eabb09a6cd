"""numpy restatement of the single-image assembly and of voxel_norm on the device (refid_amd/csrc/sample.hip:
refid_assemble_single, refid_voxel_norm), shared by test_single_assembly_host.py, test_hip_single_assembly.py and
test_hip_voxel_norm.py.  The event terms, the index map and the frames are those of sample_assembly_ref; new here are the
plain-bin voxel layout and the two-pass normalisation with its fixed summation order: per chunk of 4096 elements a thread
t adds elements k*256 + t for k = 0..15 in sequence, the 64 lanes of a wave are added by the xor tree 1, 2, .., 32
(adjacent pairs first), the four waves and then the chunks in index order.  S0 is an integer, S2 float64 in that order, S1
float64 in that order (stand-alone route) or the exact integer sum of v * 2^32 (fused route).  Every step is an integer
operation or one correctly rounded IEEE operation, so the device must reproduce it bit for bit."""
import os

import numpy as np

import sample_assembly_ref as R

CHUNK = 4096
FIXTURES = ("single_bins6", "single_bins2")


def load_fixture(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    bins, gt_size, use_hflip, use_rot = (int(v) for v in z["config"])
    cfg = dict(bins=bins, gt_size=None if gt_size < 0 else gt_size, use_hflip=bool(use_hflip), use_rot=bool(use_rot),
               seeds=[int(s) for s in z["seeds"]])
    return z, cfg


def _tree_sum(x):
    """The device's fixed order over a flat array, in x's dtype (float64 or int64)."""
    n = x.size
    chunks = -(-n // CHUNK)
    pad = np.zeros(chunks * CHUNK, dtype=x.dtype)
    pad[:n] = x
    a = pad.reshape(chunks, CHUNK // 256, 256)
    t = a[:, 0].copy()
    for k in range(1, CHUNK // 256):                      # a thread's elements in sequence (padding adds +0: no change)
        t = t + a[:, k]
    t = t.reshape(chunks, 4, 64)
    while t.shape[-1] > 1:                                # xor tree 1, 2, 4, ..: adjacent pairs first
        t = t[..., 0::2] + t[..., 1::2]
    t = t[..., 0]
    w = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]         # the four waves
    total = x.dtype.type(0)
    for c in range(chunks):                               # the chunks in index order
        total = total + w[c]
    return total


def stats(v, acc=None):
    """(S0, S1 as float64, S2) of one sample.  v: the fp32 elements; acc: the int64 scratch on the fused route."""
    v = np.ascontiguousarray(v, dtype=np.float32).ravel()
    s0 = int(np.count_nonzero(v))
    s2 = _tree_sum(v.astype(np.float64) * v.astype(np.float64))
    if acc is None:
        s1 = _tree_sum(v.astype(np.float64))
    else:
        vi = (v * np.float32(4294967296.0)).astype(np.int64)                  # exact: v is a multiple of 2^-32
        s1 = np.float64(_tree_sum(vi)) * np.float64(2.0 ** -32)
    return s0, np.float64(s1), np.float64(s2)


def normalise(v, acc=None):
    """voxel_norm of one sample as the device computes it; all zeros for a sample without spread."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    s0, s1, s2 = stats(v, acc)
    if s0 == 0:
        return np.zeros_like(v)
    n = np.float64(s0)
    mean = s1 / n
    var = s2 / n - mean * mean
    with np.errstate(invalid="ignore"):
        std_f = np.float32(np.sqrt(var))
    mean_f = np.float32(mean)
    if not (var > 0 and std_f != 0):
        return np.zeros_like(v)
    out = (v - mean_f) / std_f                                                # two fp32 operations
    assert out.dtype == np.float32
    return np.where(v != 0, out, np.float32(0)).astype(np.float32)


def float64_norm(v):
    """(exact normalisation in float64, mu, sigma) of the fp32 elements v over their non-zero entries."""
    v64 = np.asarray(v, dtype=np.float64)
    nz = v64 != 0
    mu = v64[nz].mean()
    sigma = v64[nz].std()
    return np.where(nz, (v64 - mu) / sigma, 0.0), mu, sigma


def depth(per_sample):
    """D: the float64 additions an element's term passes through: 16 in its thread, 6 in the wave, 3 over the waves, then
    one per chunk."""
    return 25 + -(-per_sample // CHUNK)


def eps_sigma(mu, sigma, per_sample):
    """Relative error of the float64 standard deviation, cancellation in S2/S0 - mean^2 included."""
    return (2 * depth(per_sample) + 8) * 2.0 ** -53 * (1 + (mu / sigma) ** 2)


def bound(v, mu, sigma, per_sample):
    """Bound B per element, second-order and float64-reduction terms included (derived in test_hip_voxel_norm.py)."""
    v64 = np.asarray(v, dtype=np.float64)
    u = 2.0 ** -24
    first = (3 * np.abs(v64 - mu) + abs(mu)) * u / sigma * (1 + 4 * u)
    red = np.abs(v64 - mu) / sigma * eps_sigma(mu, sigma, per_sample) + \
        (depth(per_sample) + 2) * 2.0 ** -53 * np.sqrt(sigma * sigma + mu * mu) / sigma
    return first + red + 2.0 ** -149


def assemble_sample(sample, bins, gt_size, norm=True):
    """One raw sample (the DeviceBatchAssembler contract, layout='single') -> (lq, voxel, gt, pre-norm voxel) float32."""
    ev = np.asarray(sample["events"], dtype=np.float32).reshape(-1, 4)
    fr = np.asarray(sample["frames"])
    y0, x0 = sample.get("origin", (0, 0))
    H, W = sample.get("frame_hw", (y0 + fr.shape[1], x0 + fr.shape[2]))
    ch, cw = (H, W) if gt_size is None else (gt_size, gt_size)
    if "crop_hw" in sample:
        ch, cw = sample["crop_hw"]
    first, last = sample.get("first_stamp"), sample.get("last_stamp")
    if first is None or last is None:
        first, last = (ev[0, 0], ev[-1, 0]) if len(ev) else (0.0, 0.0)
    aug = [sample.get(k, 0) for k in ("top", "left", "hflip", "vflip", "rot90")]
    acc = R.accumulate(ev, first, last, bins, H, W, aug[0], aug[1], ch, cw, *aug[2:])
    pre = R.fixed_to_float(acc)
    img = R.frames_to_chw(fr, y0, x0, aug[0], aug[1], ch, cw, *aug[2:])
    voxel = normalise(pre, acc) if norm else pre
    return np.ascontiguousarray(img[0]), np.ascontiguousarray(voxel), np.ascontiguousarray(img[1]), pre


def assemble_batch(samples, bins, gt_size, norm=True):
    outs = [assemble_sample(s, bins, gt_size, norm) for s in samples]
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))


def float64_sums(events, bins, H, W, top, left, ch, cw, hflip, vflip, rot90):
    """Per output element: float64 sum of the reference's per-event values (event_util.py:44-47), the number of
    contributions and their total magnitude."""
    events = np.asarray(events, dtype=np.float32).reshape(-1, 4)
    e, cnt, mass = (np.zeros((bins, ch * cw), dtype=t) for t in (np.float64, np.int64, np.float64))
    if len(events):
        keep, ti, idx, q, sign = R.event_terms(events, events[0, 0], events[-1, 0], bins, H, W, top, left, ch, cw, hflip, vflip,
                                               rot90)
        dT = np.float32(events[-1, 0] - events[0, 0])
        ts = (np.float32(bins - 1) * (events[:, 0] - events[0, 0])) / (dT if dT != 0 else np.float32(1))
        dts = ts.astype(np.float64) - ti                                      # as numpy promotes float32 - int64
        for sel, b, v in ((keep, ti, sign * (1.0 - dts)), (keep & (ti + 1 < bins), ti + 1, sign * dts)):
            np.add.at(e, (b[sel], idx[sel]), v[sel])
            np.add.at(cnt, (b[sel], idx[sel]), 1)
            np.add.at(mass, (b[sel], idx[sel]), np.abs(v[sel]))
    return (a.reshape(bins, ch, cw) for a in (e, cnt, mass))


def check_voxel(out, ref, e, cnt, mass, what):
    """The bounds of test_sample_assembly_host.py: (cnt+1)*mass*2^-24 against the reference's sequential fp32 sum, and
    cnt*2^-32 + ulp/2 against float64."""
    assert out.shape == ref.shape == e.shape
    assert np.all(out[cnt == 0] == 0) and np.all(ref[cnt == 0] == 0), what
    d = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    bnd = (cnt + 1) * mass * 2.0 ** -24
    assert np.all(d <= bnd), (what, float((d - bnd).max()), int(cnt.max()))
    d = np.abs(out.astype(np.float64) - e)
    bnd = cnt * 2.0 ** -32 + 0.5 * np.spacing(np.abs(e).astype(np.float32)).astype(np.float64)
    assert np.all(d <= bnd), (what, "vs float64", float((d - bnd).max()))
