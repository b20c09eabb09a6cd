"""CPU: the numpy restatement of the NIQE contract (tests/niqe_ref.py) and the host finish (refid_amd/niqe.py) against what
the reference's ``calculate_niqe`` recorded in tests/golden/niqe.npz (tools/make_niqe_golden.py): the NaN pattern and every
alpha identical, the other features and the scores within the measured bars of niqe_ref.py; the searchsorted alpha
selection against the reference's argmin; the error paths."""
import functools
import os

import numpy as np
import pytest

import niqe_ref as R
from refid_amd import niqe
from refid_amd._lib import RefidHipError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALPHA_COLS = [c + 18 * s for s in (0, 1) for c in (0, 2, 6, 10, 14)]


@functools.lru_cache(maxsize=None)
def _model():
    return niqe.NiqeModel.load(os.path.join(GOLDEN, "niqe_pris_params.npz"))


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(GOLDEN, "niqe.npz"))
    out = []
    for k in range(int(z["n_frames"])):
        frame = z[f"f{k}_bgr"]
        sums = R.frame_stages(frame, _model().window, bgr=True)["sums"]
        sums.setflags(write=False)
        out.append(dict(frame=frame, feat=np.concatenate([z[f"f{k}_feat1"], z[f"f{k}_feat2"]], axis=1),
                        score=float(z[f"f{k}_score"]), sums=sums))
    return out


def test_fixture_is_what_the_issue_lists():
    g = _golden()
    assert [c["frame"].shape for c in g] == [(192, 192, 3), (200, 301, 3), (192, 288, 3), (192, 192, 3)]
    assert [c["feat"].shape for c in g] == [(4, 36), (6, 36), (6, 36), (4, 36)]
    flat = np.isnan(g[2]["feat"]).any(axis=1)                               # the block of constant 255: NaN betas and means,
    assert flat.sum() == 1 and np.all(g[2]["feat"][flat][:, ALPHA_COLS] == 0.2)      # alpha 0.2 (argmin over a NaN row)
    assert all(not np.isnan(g[k]["feat"]).any() for k in (0, 1, 3))
    assert R.FEATURE_REL_BAR == 4 * R.MEASURED_FEATURE_REL and R.SCORE_ABS_BAR == 4 * R.MEASURED_SCORE_ABS
    assert R.SCORE_ABS_BAR < 1.3e-3                                         # one wrong alpha must fail


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("side", ["restatement", "finish"])
def test_against_the_reference(k, side):
    c, m = _golden()[k], _model()
    if side == "restatement":
        score, feat = R.finish_ref(c["sums"], m.mu_pris, m.cov_pris)
    else:
        scores, feats = niqe.finish(c["sums"][None], m, with_features=True)
        score, feat = scores[0], feats[0]
    ref = c["feat"]
    assert np.array_equal(np.isnan(feat), np.isnan(ref))
    assert np.array_equal(feat[:, ALPHA_COLS], ref[:, ALPHA_COLS], equal_nan=True)
    ok = ~np.isnan(ref)
    dev = np.abs(feat[ok] - ref[ok]) / (np.abs(ref[ok]) + 1e-3)
    print(f"f{k} {side}: feature deviation {dev.max():.3e}, score {score:.9f} vs {c['score']:.9f}")
    assert dev.max() <= R.FEATURE_REL_BAR
    assert abs(score - c["score"]) <= R.SCORE_ABS_BAR


def test_finish_equals_the_blockwise_restatement():
    """The vectorised finish against the one-block-at-a-time form, on the four frames and on one-sided maps: a side
    without samples gives that side's beta NaN and alpha 0.2, as the reference's argmin over a NaN row does."""
    m = _model()
    for c in _golden():
        score, feat = R.finish_ref(c["sums"], m.mu_pris, m.cov_pris)
        scores, feats = niqe.finish(c["sums"][None], m, with_features=True)
        assert np.array_equal(np.isnan(feats[0]), np.isnan(feat))
        np.testing.assert_allclose(feats[0], feat, rtol=1e-12, atol=0, equal_nan=True)
        assert abs(scores[0] - score) <= 1e-9
    sums = np.array(_golden()[0]["sums"])
    sums[0, 1, 0, [0, 2]] = 0.0                    # block 1, map n: no negative sample
    sums[1, 2, 3, [1, 3]] = 0.0                    # scale 2, block 2, map (1,1): no positive sample
    score, feat = R.finish_ref(sums, m.mu_pris, m.cov_pris)
    scores, feats = niqe.finish(sums[None], m, with_features=True)
    assert np.isnan(feat[1, 1]) and feat[1, 0] == 0.2
    assert feat[2, 18 + 10] == 0.2 and not np.isnan(feat[2, 18 + 12]) and np.isnan(feat[2, 18 + 13])
    assert np.array_equal(np.isnan(feats[0]), np.isnan(feat))
    np.testing.assert_allclose(feats[0], feat, rtol=1e-12, atol=0, equal_nan=True)
    assert abs(scores[0] - score) <= 1e-9


def test_r_gam_is_strictly_monotonic():
    assert niqe.R_GAM.shape == (9801,) and np.all(np.diff(niqe.R_GAM) > 0)
    assert np.all(np.diff(R._R_GAM) > 0)
    np.testing.assert_allclose(niqe.R_GAM, R._R_GAM, rtol=1e-15, atol=0)      # two spellings of one formula


def test_searchsorted_selection_equals_argmin():
    """Across every grid midpoint (the ties and both their float64 neighbours), the grid values, both ends and NaN / inf."""
    r = niqe.R_GAM
    mid = (r[:-1] + r[1:]) / 2
    xs = np.concatenate([mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf), r, r[:1] - 1e-3, r[-1:] + 1e-3,
                         [0.0, -1.0, 5.0, np.nan, np.inf, -np.inf]])
    want = np.array([int(np.argmin((r - x) ** 2)) for x in xs])
    np.testing.assert_array_equal(niqe.select_alpha(xs), want)
    np.testing.assert_array_equal(niqe.select_alpha(xs[:-1].reshape(2, -1)), want[:-1].reshape(2, -1))


def test_small_frames_raise():
    m = _model()
    for shape in ((95, 200, 3), (200, 95, 3)):
        with pytest.raises(ValueError):
            R.y_plane(np.zeros(shape, np.uint8))
        with pytest.raises(RefidHipError):
            niqe.calculate_niqe_frames(np.zeros(shape, np.uint8), m)
    with pytest.raises(RefidHipError):
        niqe.calculate_niqe_frames(np.zeros((101, 300, 3), np.uint8), m, crop_border=3)
    with pytest.raises(RefidHipError):
        niqe.cropped_size(96, 96, crop_border=-1)
    with pytest.raises(RefidHipError, match="gray"):
        niqe.calculate_niqe_frames(np.zeros((96, 96, 3), np.uint8), m, convert_to="gray")
    assert niqe.cropped_size(200, 301) == (192, 288) and niqe.cropped_size(198, 294, 3) == (192, 288)


def test_one_valid_block_gives_nan():
    m = _model()
    sums = np.array(_golden()[0]["sums"][:, :1])                              # a 96x96 frame: one block
    assert np.isnan(niqe.finish(sums[None], m)[0]) and np.isnan(R.finish_ref(sums, m.mu_pris, m.cov_pris)[0])
    sums = np.array(_golden()[0]["sums"][:, :2])
    sums[:, 1] = 0.0                                                          # two blocks, one of them flat
    assert np.isnan(niqe.finish(sums[None], m)[0]) and np.isnan(R.finish_ref(sums, m.mu_pris, m.cov_pris)[0])


def test_model_default_path_and_shapes(tmp_path, monkeypatch):
    assert niqe.DEFAULT_PARAMS == "basicsr/metrics/niqe_pris_params.npz"
    m = _model()
    assert m.window.shape == (7, 7) and m.window.dtype == np.float64 and m.mu_pris.shape == (36,) and m.cov_pris.shape == (36, 36)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(OSError):
        niqe.NiqeModel.load()
    np.savez(tmp_path / "bad.npz", mu_pris_param=np.zeros(3), cov_pris_param=np.zeros((3, 3)), gaussian_window=np.zeros((7, 7)))
    with pytest.raises(RefidHipError):
        niqe.NiqeModel.load(tmp_path / "bad.npz")
