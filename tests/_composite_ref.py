"""Float64 reference of compositing for the kernel sweeps in tests/test_gpu_composite_sweep.py.

forward64 is oracle.torch_oracle.raw2outputs run on float64 CPU tensors; backward64 is float64 autograd through the same graph,
plus the per-sample 3D cross-entropy (torch_oracle.ce3d) at the scales the kernel receives.  Labels outside [0, n) are masked to
-1 first: the kernels ignore them, and one_hot would raise on them.  tests/test_composite_ref.py pins both against np_oracle and
finite differences.  `dtype` exists for one thing: running the same graph in float32 to show what fp32 rounding alone costs."""
import numpy as np
import torch

from oracle import torch_oracle as to

GRAD_KEYS = ("rgb", "depth", "acc", "semantic", "instance", "weights", "fix_semantic", "fix_instance")


def _t(x, dtype):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(dtype)
    return torch.as_tensor(np.asarray(x)).to(dtype)


def _labels(lab, n):
    """int64 CPU labels with everything outside [0, n) set to -1 (None stays None)."""
    if lab is None:
        return None
    lab = (lab.detach().cpu() if isinstance(lab, torch.Tensor) else torch.as_tensor(np.asarray(lab))).long()
    return torch.where((lab >= 0) & (lab < n), lab, torch.full_like(lab, -1))


def _forward(raw, z, rays, C, K, noise, label_sem, label_inst, sem_mode, white_bkgd):
    """raw2outputs on tensors already in the working dtype (raw may require grad); the keys ops.composite returns."""
    ls, li = _labels(label_sem, C), _labels(label_inst, K)
    return to.raw2outputs(raw, z, rays[:, 3:6], C, K, noise, ls, li, int(sem_mode), bool(white_bkgd))


def forward64(raw, z, rays, C, K, noise=None, label_sem=None, label_inst=None, sem_mode=0, white_bkgd=False, dtype=torch.float64):
    """raw (R, N, 4+C+K) sample-major, z (R, N), rays (R, 8), noise (R, N) or None, labels (R, N) or None (tensors on any
    device, or arrays).  Returns every map ops.composite returns (weights included), as `dtype` CPU tensors."""
    with torch.no_grad():
        return _forward(_t(raw, dtype), _t(z, dtype), _t(rays, dtype), C, K, _t(noise, dtype), label_sem, label_inst,
                        sem_mode, white_bkgd)


def loss64(raw, z, rays, C, K, grads, noise=None, label_sem=None, label_inst=None, ce_sem=0.0, ce_inst=0.0, sem_mode=0):
    """The scalar whose gradient w.r.t. raw is what k_composite_bwd computes: sum over the given maps of <map, g_map>, plus
    ce_x times the SUM over labelled samples of the cross-entropy of their raw logits (the kernel adds ce_x (softmax - onehot)
    per labelled sample; ce3d is that sum over its count).  raw must already be a CPU tensor of the working dtype."""
    dt = raw.dtype
    z, rays, noise = _t(z, dt), _t(rays, dt), _t(noise, dt)
    out = _forward(raw, z, rays, C, K, noise, label_sem, label_inst, sem_mode, False)
    loss = raw.sum() * 0
    for k in GRAD_KEYS:
        g = grads.get(k)
        if g is not None:
            loss = loss + (out[k] * _t(g, dt)).sum()
    R, N = z.shape
    for scale, lab, n, c0 in ((ce_sem, label_sem, C, 4), (ce_inst, label_inst, K, 4 + C)):
        if not scale or lab is None or n == 0:
            continue
        ce, cnt = to.ce3d(raw[..., c0:c0 + n].reshape(R * N, n), _labels(lab, n).reshape(-1))
        loss = loss + float(scale) * cnt * ce
    return loss


def backward64(raw, z, rays, C, K, grads, noise=None, label_sem=None, label_inst=None, ce_sem=0.0, ce_inst=0.0, sem_mode=0,
               dtype=torch.float64):
    """d loss64 / d raw as (4+C+K, R*N), channel-major: the layout of ops.composite_backward's d_raw.  raw (R, N, ch)
    sample-major; grads: any subset of GRAD_KEYS (None or missing = that source off); ce_sem / ce_inst: floats."""
    r = _t(raw, dtype).requires_grad_(True)
    loss = loss64(r, z, rays, C, K, grads, noise, label_sem, label_inst, ce_sem, ce_inst, sem_mode)
    (d,) = torch.autograd.grad(loss, r, allow_unused=True)
    if d is None:
        d = torch.zeros_like(r)
    R, N, ch = r.shape
    return d.reshape(R * N, ch).T.contiguous()
