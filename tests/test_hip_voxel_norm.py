"""MI355X: refid_voxel_norm (csrc/sample.hip, ops.voxel_norm) per element against float64, and bit for bit against its
numpy restatement (tests/single_assembly_ref.py).

Bound B.  v: an fp32 element, mu / sigma: the float64 mean and standard deviation of the sample's non-zero elements,
u = 2^-24.  The kernel computes out = fl(fl(v - mean_f) / std_f), mean_f = fl32(m), std_f = fl32(s), where m and s are
the float64 mean and standard deviation AS SUMMED.  With |d1..d4| <= u for the four fp32 roundings,
    out = (v - mu - mu d1 - dm)(1 + d3)(1 + d4) / (sigma (1 + es)(1 + d2)),
dm = m - mu, es = s/sigma - 1.  First order in u: |out - (v-mu)/sigma| <= (3|v-mu| + |mu|) u / sigma, the issue's B(v).
Second order: every product of two of the d's is below u^2 and there are fewer than 4 per first-order term: a factor
(1 + 4u).  Float64 reduction, for the order of this kernel (an element's term passes through D = 16 + 6 + 3 + chunks
additions: its thread, the wave's xor tree, the four waves, the chunks of 4096 elements):
  * |dm| <= (D+2) 2^-53 sqrt(sigma^2 + mu^2): the sum of v carries at most D 2^-53 sum|v|, sum|v|/N <= sqrt(sigma^2+mu^2),
    plus the division and (fused route) the conversion of the exact integer S1;
  * var = S2/N - m^2 is a CANCELLATION: S2/N and m^2 are each about sigma^2 + mu^2 with absolute errors (D+1) 2^-53 and
    (2(D+2) + 1) 2^-53 times that, the subtraction and the square root add 2 2^-53 sigma^2; relative to sigma^2 that is at
    most (3D+8) 2^-53 (1 + (mu/sigma)^2), and s carries half of it: es <= eps_sigma = (2D+8) 2^-53 (1 + (mu/sigma)^2)
    (rounded up).
A quotient in the fp32 subnormal range may lose its last bits: + 2^-149.  Final form (single_assembly_ref.bound):
    B(v) = (3|v-mu| + |mu|) u/sigma (1 + 4u) + |v-mu|/sigma eps_sigma + (D+2) 2^-53 sqrt(sigma^2+mu^2)/sigma + 2^-149.
Families are chosen so that the cancellation term stays below one fp32 ulp of sigma, eps_sigma <= 2^-24:
    (mu/sigma)^2 <= 2^29/(2D+8) - 1,    D = 25 + ceil(N/4096), N the elements per sample.
For the N <= 8192 of this file (D <= 27): sigma/|mu| >= 1/2942.  The mean-dominated family sits at sigma/|mu| = 1/2900
(its draws are standardised, so the sample statistic is at the target); the test asserts the condition on every sample."""
import numpy as np
import pytest
import torch

import single_assembly_ref as S

pytestmark = pytest.mark.gpu

# elements per sample: two partials on the vector path | one element more than one chunk covers (scalar path: not a
# multiple of 4) | one partial, scalar path
SIZES = {"two_chunks_vec_6144": 6144, "chunk_plus_one_scalar_4097": 4097, "one_chunk_scalar_1554": 1554}


def _family(name, rng, n):
    z = rng.standard_normal(n)
    if name == "sparse_signed":                                                # event-like: about 5 % non-zero, both signs
        return np.where(rng.random(n) < 0.05, np.round(z * 3 * 2 ** 12) / 2 ** 12, 0.0)
    if name == "dense":
        return 0.3 + z
    if name == "small_1e-6":
        return (0.3 + z) * 1e-6
    if name == "large_1e+4":
        return (0.3 + z) * 1e4
    if name == "mean_dominated":
        return 1.0 + (z - z.mean()) / z.std() / 2900.0                        # standardised: the statistic sits at the target
    raise AssertionError(name)


FAMILIES = ("sparse_signed", "dense", "small_1e-6", "large_1e+4", "mean_dominated")


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("family", FAMILIES)
def test_per_element_against_float64_within_B(family, size):
    from refid_amd import ops
    n = SIZES[size]
    rng = np.random.Generator(np.random.PCG64(FAMILIES.index(family) * 10 + n))
    x = np.stack([_family(family, rng, n) for _ in range(3)]).astype(np.float32)
    x[1, 7] = 0.0                                                              # a masked element in every family
    t = torch.from_numpy(x).cuda()
    out = ops.voxel_norm(t)
    got = out.cpu().numpy()
    want = np.stack([S.normalise(x[b]) for b in range(3)])
    worst = 0.0
    for b in range(3):
        x64, mu, sigma = S.float64_norm(x[b])
        assert S.eps_sigma(mu, sigma, n) <= 2.0 ** -24, (family, "cancellation term above one ulp of sigma", mu / sigma)
        bound = S.bound(x[b], mu, sigma, n)
        nz = x[b] != 0
        assert nz.sum() >= 20 and np.all(got[b][~nz] == 0)
        d = np.abs(got[b].astype(np.float64) - x64)
        worst = max(worst, float((d[nz] / bound[nz]).max()))
        assert np.all(d[nz] <= bound[nz]), (family, size, b, worst)
    print(f"{family} {size}: worst |out - float64| / B = {worst:.3f}")
    assert np.array_equal((got + np.float32(0)).view(np.uint32), (want + np.float32(0)).view(np.uint32)), "vs the restatement"
    assert torch.equal(ops.voxel_norm(t), out), "two consecutive calls"
    inplace = t.clone()
    assert ops.voxel_norm(inplace, out=inplace) is inplace and torch.equal(inplace, out), "in place == out of place"


def test_degenerate_samples_and_batch_independence():
    from refid_amd import ops
    rng = np.random.Generator(np.random.PCG64(77))
    n = 6144
    normal = _family("sparse_signed", rng, n).astype(np.float32)
    equal = np.where(rng.random(n) < 0.1, 0.75, 0.0).astype(np.float32)         # no spread: the reference gives NaN
    one = np.zeros(n, np.float32)
    one[4100] = -2.5
    x = torch.from_numpy(np.stack([np.zeros(n, np.float32), normal, equal, one, normal])).cuda()
    out = ops.voxel_norm(x)
    assert not out[0].any() and not out[2].any() and not out[3].any(), "zeros, not NaN: the documented departure"
    assert not torch.isnan(out).any()
    assert torch.equal(out[1], out[4]) and out[1].any()
    alone = ops.voxel_norm(torch.from_numpy(normal[None]).cuda())
    assert torch.equal(alone[0], out[1]), "position 0 of 1 == position 1 of 5"
    assert torch.equal(ops.voxel_norm(x.view(5, 6, 32, 32)).view(5, n), out)


def test_rejections():
    from refid_amd import ops
    from refid_amd._lib import RefidHipError
    with pytest.raises(RefidHipError):
        ops.voxel_norm(torch.zeros(2, 8))                                       # host tensor: no CPU path
    with pytest.raises(RefidHipError):
        ops.voxel_norm(torch.zeros(2, 8, device="cuda", dtype=torch.float64))
    with pytest.raises(RefidHipError):
        ops.voxel_norm(torch.zeros(2, 8, device="cuda"), out=torch.zeros(2, 4, device="cuda"))
