"""numpy restatement of the NIQE arithmetic contract (refid_amd/niqe.py, csrc/niqe.hip): the reference's ``calculate_niqe``
(basicsr/metrics/niqe.py) with its dtypes -- float32 maps, float64 window -- and every block sum in float64.

Stages, each pinned to the device bit for bit where the contract says so:
  ``y_plane``     uint8 frame -> cropped float32 Y (to_y_channel after astype(float32))
  ``mscn``        49-tap float64 sums in row-major tap order, rounded to float32; float32 normalisation
  ``half``        the exact-factor-2 bilinear resize: a float32 2x2 mean, horizontal pair first
  ``block_sums``  per block and map: count(<0), count(>0), sum_{<0} x^2, sum_{>0} x^2, sum |x| (float64)
  ``finish_ref``  the reference's estimate_aggd_param / compute_feature / niqe tail, one block at a time with the 9801-wide
                  argmin, from the sums: the slow form that refid_amd.niqe.finish's searchsorted is checked against

``cv2.resize`` is not reproduced from a real cv2: at an exact factor 2 INTER_LINEAR is the 2x2 mean, and nobody has
compared ``half`` with cv2 itself."""
import math

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))

# The restatement against the values the reference recorded on the four frames of tests/golden/niqe.npz
# (tools/make_niqe_golden.py prints them): the reference takes its block means in float32 (pairwise), the restatement in
# float64.  The bars are the measured deviations times 4.
MEASURED_FEATURE_REL = 7.697e-6   # max |ours - ref| / (|ref| + 1e-3) over every feature (0 of 200 alphas differ)
MEASURED_SCORE_ABS = 7.956e-6     # max |ours - ref| over the four scores (4.56, 4.72, 10.40, 37.74)
FEATURE_REL_BAR = 4 * MEASURED_FEATURE_REL
SCORE_ABS_BAR = 4 * MEASURED_SCORE_ABS     # far below the 1.3e-3 by which one alpha grid step moves a score


def y_plane(u8, bgr=False, crop_border=0):
    """uint8 (H, W, 3) -> float32 (floor(h/96)*96, floor(w/96)*96) Y in [16, 235]."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 3 and u8.shape[2] == 3
    if crop_border:
        u8 = u8[crop_border:u8.shape[0] - crop_border, crop_border:u8.shape[1] - crop_border]
    h, w = u8.shape[:2]
    if h < BLOCK or w < BLOCK:
        raise ValueError(f"niqe: the frame is {h}x{w} after the border crop, smaller than one {BLOCK}x{BLOCK} block")
    u8 = u8[:h // BLOCK * BLOCK, :w // BLOCK * BLOCK]
    v = (u8.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    b, g, r = (v[..., 0], v[..., 1], v[..., 2]) if bgr else (v[..., 2], v[..., 1], v[..., 0])
    y64 = ((b * 24.966 + g * 128.553) + r * 65.481) + 16.0
    return (y64 / 255.0).astype(np.float32) * np.float32(255.0)


def _filter49(x32, window):
    """sum_k w_k * x_k in float64, taps in row-major order from a zero accumulator, edges clamped; rounded to float32."""
    h, w = x32.shape
    p = np.pad(x32.astype(np.float64), 3, mode="edge")
    acc = np.zeros((h, w), dtype=np.float64)
    for i in range(7):
        for j in range(7):
            acc = acc + float(window[i, j]) * p[i:i + h, j:j + w]
    return acc.astype(np.float32)


def mscn(y, window):
    """The locally normalised map of a float32 plane, float32."""
    assert y.dtype == np.float32
    mu = _filter49(y, window)
    sq = _filter49(y * y, window)
    sigma = np.sqrt(np.abs(sq - mu * mu))
    return (y - mu) / (sigma + np.float32(1.0))


def half(y):
    """fl32(h2(fl32(Y / 255)) * 255): the scale-2 plane."""
    v = y / np.float32(255.0)
    hz = v[:, 0::2] * np.float32(0.5) + v[:, 1::2] * np.float32(0.5)
    return (hz[0::2] * np.float32(0.5) + hz[1::2] * np.float32(0.5)) * np.float32(255.0)


def block_sums(n, bs):
    """(blocks, 5 maps, 5) float64 of a float32 map: blocks width-major (column of blocks by column), maps = n and
    fl32(n * roll(n, s)) with the roll inside the block, entries count(<0), count(>0), sum_{<0} x^2, sum_{>0} x^2, sum |x|."""
    nbh, nbw = n.shape[0] // bs, n.shape[1] // bs
    out = np.zeros((nbw * nbh, 5, 5), dtype=np.float64)
    for bw in range(nbw):
        for bh in range(nbh):
            blk = n[bh * bs:(bh + 1) * bs, bw * bs:(bw + 1) * bs]
            maps = [blk] + [blk * np.roll(blk, s, axis=(0, 1)) for s in SHIFTS]
            for m, x in enumerate(maps):
                assert x.dtype == np.float32
                x64 = x.astype(np.float64)
                neg, pos = x64[x64 < 0], x64[x64 > 0]
                out[bw * nbh + bh, m] = (neg.size, pos.size, np.sum(neg * neg), np.sum(pos * pos), np.sum(np.abs(x64)))
    return out


def frame_stages(u8, window, bgr=False, crop_border=0):
    """dict(y, mscn1, mscn2, sums): sums is (2 scales, blocks, 5, 5), the layout of refid_niqe_moments for one frame."""
    y = y_plane(u8, bgr, crop_border)
    n1 = mscn(y, window)
    n2 = mscn(half(y), window)
    return dict(y=y, mscn1=n1, mscn2=n2, sums=np.stack([block_sums(n1, BLOCK), block_sums(n2, BLOCK // 2)]))


_GAM = np.arange(0.2, 10.001, 0.001)
_R_GAM = np.array([math.gamma(2.0 / g) ** 2 / (math.gamma(1.0 / g) * math.gamma(3.0 / g)) for g in _GAM.tolist()])


def _aggd(s, count):
    """estimate_aggd_param from the five sums of one map: (alpha, beta_l, beta_r), NaN where a side is empty."""
    with np.errstate(invalid="ignore", divide="ignore"):
        left = np.sqrt(np.float64(s[2]) / np.float64(s[0]))
        right = np.sqrt(np.float64(s[3]) / np.float64(s[1]))
        gammahat = left / right
        rhat = (s[4] / count) ** 2 / ((s[2] + s[3]) / count)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        alpha = _GAM[np.argmin((_R_GAM - rhatnorm) ** 2)]      # a NaN rhatnorm gives index 0, alpha 0.2, as in the reference
        k = math.sqrt(math.gamma(1 / alpha) / math.gamma(3 / alpha))
    return alpha, left * k, right * k


def features_ref(sums, count):
    """compute_feature per block: (blocks, 18) from (blocks, 5, 5)."""
    feat = np.zeros((sums.shape[0], 18), dtype=np.float64)
    for b in range(sums.shape[0]):
        alpha, bl, br = _aggd(sums[b, 0], count)
        row = [alpha, (bl + br) / 2]
        for m in range(1, 5):
            alpha, bl, br = _aggd(sums[b, m], count)
            mean = (br - bl) * (math.gamma(2 / alpha) / math.gamma(1 / alpha))
            row += [alpha, mean, bl, br]
        feat[b] = row
    return feat


def finish_ref(sums, mu_pris, cov_pris):
    """(score, features (blocks, 36)) from one frame's (2, blocks, 5, 5) sums: niqe()'s tail."""
    feat = np.concatenate([features_ref(sums[0], BLOCK * BLOCK), features_ref(sums[1], BLOCK * BLOCK // 4)], axis=1)
    ok = ~np.isnan(feat).any(axis=1)
    if ok.sum() < 2:
        return float("nan"), feat
    with np.errstate(invalid="ignore"):
        mu = np.nanmean(feat, axis=0)
    cov = np.cov(feat[ok], rowvar=False)
    inv = np.linalg.pinv((cov_pris + cov) / 2)
    d = mu_pris - mu
    return float(np.sqrt(np.matmul(np.matmul(d, inv), np.transpose(d))).reshape(-1)[0]), feat


def niqe_ref(u8, params, bgr=False, crop_border=0):
    """(score, features) of one uint8 frame; ``params`` maps mu_pris_param, cov_pris_param, gaussian_window."""
    st = frame_stages(u8, params["gaussian_window"], bgr, crop_border)
    return finish_ref(st["sums"], params["mu_pris_param"], params["cov_pris_param"])
