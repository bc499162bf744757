"""CPU checks of the float64 compositing reference (tests/_composite_ref.py) that the GPU sweep compares the kernels with:
forward64 equals the plain-loop np_oracle.composite, and backward64's gradient passes finite differences."""
import numpy as np
import pytest
import torch

import _composite_ref as cref
from oracle import np_oracle


def _case(seed, R, N, C, K):
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 1, (R, 3))
    d = (rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])) * rng.uniform(0.5, 2.0, (R, 1))     # non-unit directions
    rays = np.concatenate([o, d, np.full((R, 1), 0.5), np.full((R, 1), 6.0)], 1)
    z = 0.5 + 5.5 * (np.arange(N) + rng.random((R, N))) / N
    z[0, 2:4] = z[0, 1]                                        # a run of equal z (dist = 0)
    raw = rng.normal(0, 1, (R, N, 4 + C + K))
    raw[..., 3] = rng.normal(0.3, 0.5, (R, N))
    noise = rng.normal(0, 0.05, (R, N))
    # -1 / -7 / >= n are ignored by the kernels; the reference must ignore them too
    ls = rng.choice(np.array([-7, -1, C, C + 2] + list(range(C)), dtype=np.int32), (R, N))
    li = rng.choice(np.array([-7, -1, K, K + 2] + list(range(K)), dtype=np.int32), (R, N))
    return raw, z, rays, noise, ls, li


@pytest.mark.parametrize("sem_mode", [0, 1])
@pytest.mark.parametrize("white_bkgd", [False, True])
@pytest.mark.parametrize("C,K", [(0, 0), (1, 0), (3, 2), (7, 5)])
def test_forward64_equals_np_oracle(sem_mode, white_bkgd, C, K):
    raw, z, rays, noise, ls, li = _case(10 * C + K + sem_mode, 5, 12, C, K)
    got = cref.forward64(raw, z, rays, C, K, noise, ls, li, sem_mode, white_bkgd)
    want = np_oracle.composite(raw, z, rays, C, K, noise, ls, li, sem_mode, white_bkgd)
    keys = {"rgb", "depth", "acc", "weights"} | ({"semantic", "fix_semantic"} if C else set()) | ({"instance", "fix_instance"} if K else set())
    assert set(got) == keys
    for k in keys:
        assert got[k].dtype == torch.float64
        np.testing.assert_allclose(got[k].numpy(), want[k], atol=1e-12, rtol=0, err_msg=k)
    # without labels the fixed fields are absent
    assert "fix_semantic" not in cref.forward64(raw, z, rays, C, K, noise, None, li, sem_mode, white_bkgd)


@pytest.mark.parametrize("sem_mode", [0, 1])
def test_backward64_passes_gradcheck(sem_mode):
    R, N, C, K = 3, 8, 3, 2
    raw, z, rays, noise, ls, li = _case(7 + sem_mode, R, N, C, K)
    rng = np.random.default_rng(99)
    shapes = {"rgb": (R, 3), "depth": (R,), "acc": (R,), "semantic": (R, C), "instance": (R, K), "weights": (R, N),
              "fix_semantic": (R, C), "fix_instance": (R, K)}
    grads = {k: torch.tensor(rng.normal(size=s)) for k, s in shapes.items()}
    assert (ls >= 0).any() and (ls < C).any() and ((ls < 0) | (ls >= C)).any()
    r = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    fn = lambda x: cref.loss64(x, z, rays, C, K, grads, noise, ls, li, 0.3, 0.2, sem_mode)   # noqa: E731
    assert torch.autograd.gradcheck(fn, (r,), eps=1e-6, atol=1e-7, rtol=1e-5)
    # backward64 is that gradient, channel-major
    d = cref.backward64(raw, z, rays, C, K, grads, noise, ls, li, 0.3, 0.2, sem_mode)
    (want,) = torch.autograd.grad(fn(r), r)
    assert d.shape == (4 + C + K, R * N)
    assert torch.equal(d, want.reshape(R * N, -1).T)
    # every source reaches d_raw: the CE term alone moves only the logit rows of labelled samples
    d_ce = cref.backward64(raw, z, rays, C, K, {}, noise, ls, li, 0.3, 0.0, sem_mode)
    valid = torch.tensor(((ls >= 0) & (ls < C)).reshape(-1))
    assert (d_ce[:4] == 0).all() and (d_ce[4 + C:] == 0).all()
    assert (d_ce[4:4 + C, ~valid] == 0).all() and (d_ce[4:4 + C, valid] != 0).all()
    for k in shapes:
        assert cref.backward64(raw, z, rays, C, K, {k: grads[k]}, noise, ls, li, sem_mode=sem_mode).abs().max() > 0, k
