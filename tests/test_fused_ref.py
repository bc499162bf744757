"""CPU checks of the float64 reference of the fused inference pass (tests/_fused_ref.py) that tests/test_gpu_fused_sweep.py compares
the kernels with: its tile factorisation, combined again, is the plain compositing graph (_composite_ref.forward64) to 1e-12 at
every sample count the fused pass takes, in both compositing modes, with and without white background and labels; it equals
np_oracle.composite_by_tiles; and each of the mistakes a fused kernel could make (the tile transmittance one tile late, a finite
last interval, no 1e-10, an inclusive scan, a softmax denominator over half the channels) makes that comparison fail."""
import numpy as np
import pytest
import torch

import _composite_ref as cref
import _fused_io as fio
import _fused_ref as fref
from oracle import np_oracle

ALL_N = list(range(32, 257, 32))


def _case(seed, R, N, C, K):
    """the sweep's edge rays and z (tests/_fused_io.py) with raw of every kind: translucent rays whose last sample matters,
    an opaque sample in the first tile (ray 2), an empty ray (ray 4), a ray opaque only at its last sample (ray 5), logits of +-80
    (every 6th ray), labels with ignored values"""
    rays, z = fio.rays_z(seed, R, N)
    rng = np.random.default_rng(seed)
    raw = rng.normal(0, 1, (R, N, 4 + C + K))
    raw[..., 3] = rng.normal(0.0, 0.05, (R, N)) * rng.uniform(0.2, 3.0, (R, 1))
    raw[2, 1, 3] = 1e3
    raw[4, :, 3] = -1.0
    raw[5, :, 3] = -1.0
    raw[5, -1, 3] = 1e-3
    raw[::6, :, 4:] = rng.choice([-80.0, 80.0], (len(range(0, R, 6)), N, C + K))
    return raw, z.astype(np.float64), rays.astype(np.float64), fio.labels(seed, R, N, C), fio.labels(seed + 1, R, N, K)


def _err(got, want, k, rays):
    """max over rays of |got - want| / the ray's scale (max(1, max |want[ray]|), its far for depth)"""
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    scale = torch.as_tensor(rays[:, 7]) if k == "depth" else w.abs().amax(1).clamp(min=1.0)
    return float(((g - w).abs().amax(1) / scale).max()) if w.numel() else 0.0


def _compare(raw, z, rays, C, K, ls, li, sem_mode, white):
    got = fref.forward_fused64(raw, z, rays, C, K, ls, li, sem_mode, white)
    want = cref.forward64(raw, z, rays, C, K, None, ls, li, sem_mode, white)
    assert set(got) == set(want), (sorted(got), sorted(want))
    return max(_err(got[k], want[k], k, rays) for k in want)


@pytest.mark.parametrize("N", ALL_N)
@pytest.mark.parametrize("sem_mode", [0, 1])
def test_tiles_then_combine_is_forward64(N, sem_mode):
    for C, K in ((7, 5), (19, 8), (0, 3), (0, 0)):
        raw, z, rays, ls, li = _case(N + C, 23, N, C, K)
        for white in (False, True):
            for lab in (False, True):
                e = _compare(raw, z, rays, C, K, ls if lab else None, li if lab else None, sem_mode, white)
                assert e <= 1e-12, (N, sem_mode, C, K, white, lab, e)


def test_records_layout_and_labels():
    C, K, N = 7, 5, 96
    raw, z, rays, ls, li = _case(3, 11, N, C, K)
    rec, qd = fref.tiles64(raw, z, rays, C, K)
    assert rec.shape == (11, 3, 1 + C + K) and qd.shape == (11, N, 4) and rec.dtype == torch.float64
    assert torch.equal(qd[..., 1:], torch.as_tensor(raw[..., :3]))
    assert float(rec[2, 0, 0]) < 1e-9                                            # opaque in tile 0
    assert float((rec[4, :, 0] - (1 + 1e-10) ** 32).abs().max()) < 1e-15           # empty: only the 1e-10 terms
    assert float(qd[5, -1, 0]) > 0.99                                           # 1e10 interval of the last sample
    full = fref.combine64(rec, qd, z, C, K, ls, li)
    clean = fref.combine64(rec, qd, z, C, K, np.where(ls < C, ls, -1), np.where((li >= 0) & (li < K), li, -1))
    for k in ("fix_semantic", "fix_instance"):
        assert torch.equal(full[k], clean[k]), k
    assert set(fref.combine64(rec, qd, z, C, K)) == {"rgb", "depth", "acc", "weights", "semantic", "instance"}


@pytest.mark.parametrize("N", [32, 96, 256])
def test_equals_np_oracle_composite_by_tiles(N):
    C, K = 4, 3
    raw, z, rays, ls, li = _case(N + 5, 6, N, C, K)
    for white in (False, True):
        got = fref.forward_fused64(raw, z, rays, C, K, ls, li, 0, white)
        want = np_oracle.composite_by_tiles(raw, z, rays, C, K, 32, ls, li, white)
        for k in got:
            np.testing.assert_allclose(got[k].numpy(), want[k], atol=1e-12, rtol=0, err_msg=k)


def _inclusive(f):
    inc = torch.cumprod(f, -1)
    return inc, inc[..., -1]


def _tk_late(Q):
    return torch.cumprod(Q, 1)


def _finite_last(z, rays):
    d = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], 1)
    return d * torch.linalg.vector_norm(rays[:, 3:6], dim=-1)[:, None]


def _half_softmax(raw, C, K, sem_mode):
    """softmax whose denominator covers one 16-channel half of each 32-channel block (a missing half-wave exchange)"""
    v = raw[..., 4:4 + C + K]
    if int(sem_mode) != 1:
        return v
    out = []
    for a, n in ((0, C), (C, K)):
        h = v[..., a:a + n]
        e = torch.exp(h - h.amax(-1, keepdim=True))
        den = torch.stack([e[..., (torch.arange(n) // 16) == g].sum(-1) for g in range((n + 15) // 16)], -1)
        out.append(e / den[..., torch.arange(n) // 16])
    return torch.cat(out, -1)


MUTANTS = {"Tk one tile late": ("_tile_T", _tk_late), "last interval not 1e10": ("_dists", _finite_last),
           "no 1e-10": ("EPS_T", 0.0), "inclusive scan": ("_tile_scan", _inclusive),
           "softmax over half the channels": ("_values", _half_softmax)}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_reference_mutants_fail(name, monkeypatch):
    attr, bad = MUTANTS[name]
    C, K, N = 19, 8, 64
    raw, z, rays, ls, li = _case(11, 23, N, C, K)
    sem_mode = 1 if "softmax" in name else 0
    assert _compare(raw, z, rays, C, K, ls, li, sem_mode, False) <= 1e-12
    monkeypatch.setattr(fref, attr, bad)
    assert _compare(raw, z, rays, C, K, ls, li, sem_mode, False) > 1e-9, name
