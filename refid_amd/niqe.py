"""NIQE, the reference's no-reference score (basicsr/metrics/niqe.py ``calculate_niqe``), for frames without ground truth.

The per-pixel work -- Y plane, the two 7x7 Gaussian local normalisations, the four neighbour products and the per-block
moment sums, at both scales -- is ONE pass of csrc/niqe.hip over the uint8 frames that ``metrics.val_tail`` leaves on the
device (``moments``).  What remains is 50 numbers per 96x96 block: ``finish`` turns them into the 36 AGGD features per
block and the Mahalanobis distance to the pristine model on the host, in float64, with numpy and ``math`` only, for all
blocks of all frames at once.

The arithmetic contract (every rounding, INTEGRATION.md "NIQE") is shared with the numpy restatement in
tests/niqe_ref.py, bit for bit up to the order of the float64 block sums.  Two things to know: the reference's
``cv2.resize`` to half size is taken as the float32 2x2 mean (what INTER_LINEAR is at an exact factor 2; not compared with
a real cv2), and inside an area of constant colour the map is exactly zero (fl32(mu) equals Y there), so a block of
constant colour has samples on one side at most, NaN features and a row that the score leaves out, as in the
reference.  ``convert_to='gray'`` is not offered (it is cv2's conversion)."""
import collections
import math

import numpy as np

from ._lib import RefidHipError

BLOCK = 96
DEFAULT_PARAMS = "basicsr/metrics/niqe_pris_params.npz"

_GAM = np.arange(0.2, 10.001, 0.001)                       # the reference's alpha grid, len 9801
_G1, _G2, _G3 = (np.array([math.gamma(k / g) for g in _GAM.tolist()]) for k in (1.0, 2.0, 3.0))
R_GAM = _G2 ** 2 / (_G1 * _G3)                             # strictly increasing in alpha
_BETA = np.sqrt(_G1 / _G3)                                 # beta = std * sqrt(gamma(1/alpha) / gamma(3/alpha))
_MEAN = _G2 / _G1                                          # mean = (beta_r - beta_l) * gamma(2/alpha) / gamma(1/alpha)


class NiqeModel(collections.namedtuple("NiqeModel", "mu_pris cov_pris window")):
    """The pristine model: ``mu_pris`` (36,), ``cov_pris`` (36, 36) and the 7x7 float64 ``window`` of the parameter file."""

    @classmethod
    def load(cls, path=None):
        """Reads ``niqe_pris_params.npz``; ``path`` defaults to where the reference reads it, relative to the working
        directory.  The window is used as stored, never rebuilt."""
        with np.load(DEFAULT_PARAMS if path is None else path) as z:
            mu = np.asarray(z["mu_pris_param"], dtype=np.float64).reshape(-1)
            cov = np.asarray(z["cov_pris_param"], dtype=np.float64)
            win = np.ascontiguousarray(z["gaussian_window"], dtype=np.float64)
        if mu.shape != (36,) or cov.shape != (36, 36) or win.shape != (7, 7):
            raise RefidHipError(f"NiqeModel.load: unexpected shapes mu {mu.shape}, cov {cov.shape}, window {win.shape}")
        return cls(mu, cov, win)


def cropped_size(h, w, crop_border=0):
    """(rows, columns) of the Y plane: the border crop, then whole 96x96 blocks from the top-left.  Raises when no block fits."""
    crop_border = int(crop_border)
    hc, wc = h - 2 * crop_border, w - 2 * crop_border
    if crop_border < 0 or hc < BLOCK or wc < BLOCK:
        raise RefidHipError(f"niqe: a {h}x{w} frame with crop_border {crop_border} holds no {BLOCK}x{BLOCK} block")
    return hc // BLOCK * BLOCK, wc // BLOCK * BLOCK


def select_alpha(rhatnorm):
    """Indices into the alpha grid whose ``R_GAM`` is nearest to ``rhatnorm`` (any shape), the lower one on a tie: what
    ``argmin((r_gam - rhatnorm)**2)`` returns, by ``searchsorted`` and a comparison of the two neighbours.  NaN and
    +-inf give 0, as the argmin over a row of NaN or inf does."""
    r = np.asarray(rhatnorm, dtype=np.float64)
    finite = np.isfinite(r)
    x = np.where(finite, r, 0.0)
    hi = np.clip(np.searchsorted(R_GAM, x, side="left"), 1, R_GAM.size - 1)
    lo = hi - 1
    take_hi = (R_GAM[hi] - x) ** 2 < (R_GAM[lo] - x) ** 2
    return np.where(finite, np.where(take_hi, hi, lo), 0)


def _aggd(s, count):
    """estimate_aggd_param on (..., 5) sums: (grid index, left std, right std)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        left = np.sqrt(s[..., 2] / s[..., 0])
        right = np.sqrt(s[..., 3] / s[..., 1])
        gammahat = left / right
        rhat = (s[..., 4] / count) ** 2 / ((s[..., 2] + s[..., 3]) / count)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
    return select_alpha(rhatnorm), left, right


def features(sums, count):
    """compute_feature for every block at once: (..., 5 maps, 5) sums of maps of ``count`` pixels -> (..., 18)."""
    sums = np.asarray(sums, dtype=np.float64)
    idx, left, right = _aggd(sums, float(count))
    bl, br = left * _BETA[idx], right * _BETA[idx]
    feat = np.empty(sums.shape[:-2] + (18,), dtype=np.float64)
    feat[..., 0] = _GAM[idx[..., 0]]
    feat[..., 1] = (bl[..., 0] + br[..., 0]) / 2
    for m in range(1, 5):
        feat[..., 4 * m - 2] = _GAM[idx[..., m]]
        feat[..., 4 * m - 1] = (br[..., m] - bl[..., m]) * _MEAN[idx[..., m]]
        feat[..., 4 * m] = bl[..., m]
        feat[..., 4 * m + 1] = br[..., m]
    return feat


def finish(sums, model, with_features=False):
    """Scores from the moment sums of ``moments`` (or of the numpy restatement): ``sums`` (nf, 2 scales, blocks, 5 maps, 5)
    float64 -> a list of nf floats.  A frame with fewer than two NaN-free blocks scores ``nan``."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 5 or sums.shape[1] != 2 or sums.shape[3:] != (5, 5):
        raise RefidHipError(f"niqe.finish: sums must be (nf, 2, blocks, 5, 5), got {sums.shape}")
    feat = np.concatenate([features(sums[:, 0], BLOCK * BLOCK), features(sums[:, 1], BLOCK * BLOCK // 4)], axis=-1)
    scores = []
    for f in feat:
        ok = ~np.isnan(f).any(axis=1)
        if ok.sum() < 2:
            scores.append(float("nan"))
            continue
        with np.errstate(invalid="ignore"):
            mu = np.nanmean(f, axis=0)
        cov = np.cov(f[ok], rowvar=False)
        d = model.mu_pris - mu
        scores.append(float(math.sqrt(d @ np.linalg.pinv((model.cov_pris + cov) / 2) @ d)))
    return (scores, feat) if with_features else scores


_windows = {}            # (device, window bytes) -> the 49 float64 weights on the device


def _window_dev(model, device):
    import torch
    key = (str(device), model.window.tobytes())
    t = _windows.get(key)
    if t is None:
        t = _windows[key] = torch.from_numpy(model.window.reshape(-1).copy()).to(device)
    return t


def moments(u8, model, bgr=False, crop_border=0, planes=False):
    """The device half: ``u8`` uint8 CUDA (..., H, W, 3) -> float64 CUDA sums (nf, 2, blocks, 5, 5) on the current stream,
    without synchronising.  ``planes=True`` also returns the float32 [Y, MSCN scale 1, MSCN scale 2] planes."""
    import torch
    from . import ops
    if not torch.is_tensor(u8) or not u8.is_cuda:
        raise RefidHipError("niqe.moments: a uint8 CUDA tensor (..., H, W, 3) is required (the HIP path has no CPU fallback)")
    return ops.niqe_moments(u8, _window_dev(model, u8.device), bgr, crop_border, planes)


def calculate_niqe_frames(u8, model, bgr=False, crop_border=0, convert_to="y"):
    """``calculate_niqe(img, crop_border, input_order='HWC', convert_to='y')`` per frame: ``u8`` uint8 (..., H, W, 3), a
    CUDA tensor, host tensor or numpy array (uploaded); ``bgr``: the channel order of ``u8`` (the reference takes BGR; the
    PNG path here holds RGB).  ``convert_to='gray'`` raises: it is cv2's conversion.  One device->host copy for all
    frames.  Returns a list of floats."""
    import torch
    if convert_to != "y":
        raise RefidHipError(f"calculate_niqe_frames: convert_to={convert_to!r} is not offered (only 'y'; 'gray' needs cv2)")
    if not torch.is_tensor(u8):
        u8 = torch.from_numpy(np.ascontiguousarray(u8))
    if u8.dim() >= 3:
        cropped_size(int(u8.shape[-3]), int(u8.shape[-2]), crop_border)      # raises before any upload
    if not u8.is_cuda:
        u8 = u8.to("cuda")
    return finish(moments(u8, model, bgr, crop_border).cpu().numpy(), model)
