"""Test support: one device allocation filled with a sentinel, every buffer of a call an interior view of it with a guard on both
sides (test_gpu_mlp_fp32_sweep.py, test_gpu_mlp_fp32_infer_sweep.py).  Not part of the product package."""
import torch

SENTINEL = -7.5e33
GUARD = 64                      # floats on each side of every buffer


class Arena:
    """one device allocation filled with the sentinel; every buffer an interior view with a guard on both sides"""

    def __init__(self, dev, sizes):
        """sizes: [(name, floats, guard floats)]"""
        self.off, o = {}, 0
        guard_idx = []
        for name, n, g in sizes:
            self.off[name] = (o + g, n)
            guard_idx += [torch.arange(o, o + g), torch.arange(o + g + n, o + 2 * g + n)]
            o += n + 2 * g
        self.buf = torch.full((o,), SENTINEL, device=dev, dtype=torch.float32)
        self.guard_idx = torch.cat(guard_idx).to(dev)

    def view(self, name):
        o, n = self.off[name]
        return self.buf[o:o + n]

    def guards_intact(self):
        return bool((self.buf[self.guard_idx] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())
