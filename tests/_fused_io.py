"""Inputs and C-ABI plumbing shared by the tests of the fused inference pass (pnr_mlp_forward_composite = pnr_mlp_forward_tiles +
pnr_composite_combine): seeded rays / z / labels with the edge cases the float64 sweep needs, the workspace the MLP epilogue
fills (per-tile records, then per-sample quadruples), and k_composite_combine run on a workspace written by hand."""
import ctypes

import numpy as np
import torch

NEAR, FAR = 0.5, 60.0


def rays_z(seed, R, N, near=NEAR, far=FAR, edge=True):
    """float32 rays (R, 8) and sorted z (R, N) in [near, far].  Directions have |d| in 0.5 .. 2.  edge=True adds, in separate
    rays: an axis-aligned d (ray 0), one ray whose z are all equal (ray 1), far = 1e3 (every 7th ray from 3), and runs of equal
    z across every tile edge -- samples 29 .. 34, 61 .. 66, ... share one z (every 5th ray from 2)."""
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 1, (R, 3)) + np.array([0, 1.5, 0])
    d = (rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])) * rng.uniform(0.5, 2.0, (R, 1))
    fr = np.full(R, far)
    if edge:
        d[0] = (0.0, 0.0, 1.7)
        fr[3::7] = 1e3
    rays = np.concatenate([o, d, np.full((R, 1), near), fr[:, None]], 1).astype(np.float32)
    z = (near + (fr[:, None] - near) * (np.arange(N) + rng.random((R, N))) / N).astype(np.float32)
    if edge:
        if R > 1:
            z[1] = z[1, N // 2]
        for r in range(2, R, 5):
            for e in range(32, N + 1, 32):
                z[r, e - 3:e + 3] = z[r, e - 3]
    return rays, z


def labels(seed, R, N, n):
    """int32 (R, N) labels drawn from -7, -1, n, n + 3 (all ignored) and 0 .. n - 1"""
    rng = np.random.default_rng(seed + 77)
    return rng.choice(np.array([-7, -1, n, n + 3] + list(range(n)), np.int32), (R, N))


def rec_floats(C, K):
    """pnr_fuse_record_floats: a record's stride in floats"""
    return (1 + C + K + 3) & ~3


def ws_layout(R, N, C, K):
    """(padded tile count, record stride, byte offset of the quadruples) of a fused workspace (pnr_composite_combine)"""
    pad = (R * N + 255) // 256 * 8
    rf = rec_floats(C, K)
    return pad, rf, pad * rf * 4


def tiles_workspace(desc, img, rays, z):
    """pnr_mlp_forward_tiles into a 0xAB-filled workspace: (records (tiles, 1 + C + K), quadruples (S, 4))"""
    from panopticnerf_amd import _lib
    lib = _lib.load()
    R, N = z.shape
    S = R * N
    nbytes = lib.pnr_mlp_forward_composite_workspace_bytes(ctypes.byref(desc), R, N, 0)
    ws = torch.full((int(nbytes),), 0xAB, device=z.device, dtype=torch.uint8)
    _lib.check(lib.pnr_mlp_forward_tiles(ctypes.byref(desc), ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(rays.data_ptr()),
                                         ctypes.c_void_p(z.data_ptr()), R, N, ctypes.c_void_p(ws.data_ptr()),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pnr_mlp_forward_tiles")
    pad, rf, q0 = ws_layout(R, N, desc.n_sem, desc.n_inst)
    rec = ws[:q0].view(torch.float32).reshape(pad, rf)[: (S + 31) // 32, : 1 + desc.n_sem + desc.n_inst]
    ps = ws[q0: q0 + S * 16].view(torch.float32).reshape(S, 4)
    return rec.clone(), ps.clone()


def combine(desc, records, quads, z, label_sem=None, label_inst=None, white_bkgd=False):
    """pnr_composite_combine on records (R, T, 1 + C + K) and quadruples (R, N, 4) written into a workspace by hand (float32 on
    the device; the record padding holds NaN, which the kernel must not read).  Returns every map, weights included."""
    from panopticnerf_amd import _lib
    lib = _lib.load()
    R, N = z.shape
    C, K = desc.n_sem, desc.n_inst
    pad, rf, q0 = ws_layout(R, N, C, K)
    ws = torch.full((q0 // 4 + R * N * 4,), float("nan"), device=z.device, dtype=torch.float32)
    ws[: R * (N // 32) * rf].view(R * (N // 32), rf)[:, : 1 + C + K] = records.reshape(R * (N // 32), 1 + C + K)
    ws[q0 // 4:] = quads.reshape(-1)
    f32 = dict(device=z.device, dtype=torch.float32)
    out = {"rgb": torch.empty((R, 3), **f32), "depth": torch.empty(R, **f32), "acc": torch.empty(R, **f32),
           "weights": torch.empty((R, N), **f32)}
    if C:
        out["semantic"] = torch.empty((R, C), **f32)
        if label_sem is not None:
            out["fix_semantic"] = torch.empty((R, C), **f32)
    if K:
        out["instance"] = torch.empty((R, K), **f32)
        if label_inst is not None:
            out["fix_instance"] = torch.empty((R, K), **f32)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)   # noqa: E731
    g = out.get
    _lib.check(lib.pnr_composite_combine(ctypes.byref(desc), p(ws), p(z), R, N, p(label_sem), p(label_inst), int(bool(white_bkgd)),
                                         p(out["rgb"]), p(out["depth"]), p(out["acc"]), p(out["weights"]), p(g("semantic")),
                                         p(g("instance")), p(g("fix_semantic")), p(g("fix_instance")),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pnr_composite_combine")
    return out
