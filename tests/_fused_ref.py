"""Float64 reference of the fused inference pass (SURVEY.md 8a rows a5 + a6 in one pass) for tests/test_gpu_fused_sweep.py.

tiles64 is what the MLP epilogue writes (csrc/pnr_mlp_fuse.h, the tails of csrc/asm/gen_mlp_tt.py): per 32-sample tile
    Q   = prod_i (1 - alpha_i + 1e-10),   S_c = sum_i lw_i v_ci   (v = the logits, or softmax of each head's logits in sem_mode 1)
and per sample lw_i = alpha_i prod_{j < i in tile} (1 - alpha_j + 1e-10) with the raw r, g, b.  combine64 is what
k_composite_combine (csrc/pnr_composite.hip) makes of them: T_k = prod_{k' < k} Q_k', w_i = T_k lw_i, acc / depth / rgb =
sum_i w_i {1, z_i, sigmoid(rgb_i)}, fix_x[c] = sum_i w_i [label_i == c], logits_c = sum_k T_k S_c(k).

Each step is a small function or constant of its own (_dists, EPS_T, _tile_scan, _values, _tile_T), so that
tests/test_fused_ref.py can corrupt one at a time and show that the comparison with _composite_ref.forward64 notices.  Vectorised torch, float64, CPU."""
import torch

from _composite_ref import _labels, _t

TILE = 32
F64 = torch.float64
EPS_T = 1e-10               # added to every 1 - alpha (the oracle's cumprod term)


def _dists(z, rays):
    """(R, N) interval of every sample times |d|: z_{i+1} - z_i, 1e10 for the ray's last sample"""
    d = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], 1)
    return d * torch.linalg.vector_norm(rays[:, 3:6], dim=-1)[:, None]


def _tile_scan(f):
    """(R, T, 32) factors -> exclusive product inside each tile, and each tile's total"""
    inc = torch.cumprod(f, -1)
    excl = torch.cat([torch.ones_like(f[..., :1]), inc[..., :-1]], -1)
    return excl, inc[..., -1]


def _values(raw, C, K, sem_mode):
    """(R, N, C + K): what the tile sums weight -- the logits, or in sem_mode 1 softmax over each head's own channels"""
    v = raw[..., 4:4 + C + K]
    if int(sem_mode) != 1:
        return v
    parts = [torch.softmax(v[..., :C], -1)] if C else []
    if K:
        parts.append(torch.softmax(v[..., C:], -1))
    return torch.cat(parts, -1) if parts else v


def _tile_T(Q):
    """(R, T) tile factors -> transmittance in front of each tile: exclusive product over the tiles"""
    return torch.cat([torch.ones_like(Q[:, :1]), torch.cumprod(Q, 1)[:, :-1]], 1)


def tiles64(raw, z, rays, C, K, sem_mode=0):
    """raw (R, N, 4 + C + K) sample-major, z (R, N), rays (R, 8); N % 32 == 0.  Returns float64 CPU tensors:
    records (R, T, 1 + C + K) in the kernel's layout ([0] Q, then the semantic and instance sums) and quads (R, N, 4) =
    (lw, r, g, b) with the raw colour channels."""
    raw, z, rays = _t(raw, F64), _t(z, F64), _t(rays, F64)
    R, N = z.shape
    assert N % TILE == 0 and raw.shape == (R, N, 4 + C + K)
    T = N // TILE
    alpha = 1.0 - torch.exp(-torch.relu(raw[..., 3]) * _dists(z, rays))
    excl, Q = _tile_scan((1.0 - alpha + EPS_T).reshape(R, T, TILE))
    lw = alpha * excl.reshape(R, N)
    S = (lw[..., None] * _values(raw, C, K, sem_mode)).reshape(R, T, TILE, C + K).sum(2)
    records = torch.cat([Q[..., None], S], -1)
    quads = torch.cat([lw[..., None], raw[..., :3]], -1)
    return records, quads


def combine64(records, quads, z, C, K, label_sem=None, label_inst=None, white_bkgd=False):
    """records (R, T, 1 + C + K), quads (R, N, 4) as tiles64 returns them (or as the kernel wrote them), z (R, N), labels
    (R, N) or None (outside [0, n) ignored).  Returns the dict ops.mlp_forward_composite returns, weights included."""
    rec, qd, z = _t(records, F64), _t(quads, F64), _t(z, F64)
    R, N = z.shape
    T = N // TILE
    Tk = _tile_T(rec[..., 0])
    w = (Tk[..., None] * qd[..., 0].reshape(R, T, TILE)).reshape(R, N)
    rgb = (w[..., None] * torch.sigmoid(qd[..., 1:4])).sum(1)
    acc = w.sum(1)
    out = {"weights": w, "rgb": rgb + (1.0 - acc[:, None]) if white_bkgd else rgb, "depth": (w * z).sum(1), "acc": acc}
    logits = (Tk[..., None] * rec[..., 1:1 + C + K]).sum(1)
    for key, fix, lab, n, c0 in (("semantic", "fix_semantic", label_sem, C, 0), ("instance", "fix_instance", label_inst, K, C)):
        if not n:
            continue
        out[key] = logits[:, c0:c0 + n]
        if lab is not None:
            lab = _labels(lab, n)
            oh = torch.nn.functional.one_hot(lab.clamp(min=0), n).to(F64) * (lab >= 0)[..., None]
            out[fix] = (w[..., None] * oh).sum(1)
    return out


def forward_fused64(raw, z, rays, C, K, label_sem=None, label_inst=None, sem_mode=0, white_bkgd=False):
    """combine64(tiles64(...)): the whole fused pass in float64"""
    rec, qd = tiles64(raw, z, rays, C, K, sem_mode)
    return combine64(rec, qd, z, C, K, label_sem, label_inst, white_bkgd)
