"""Test support: one device allocation filled with a sentinel, every buffer of a call an interior view of it with a guard on both
sides (test_gpu_mlp_fp32_sweep.py, test_gpu_mlp_fp32_infer_sweep.py; ByteArena, for byte buffers: test_gpu_pack_device.py).  Not
part of the product package."""
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


BYTE_SENTINEL = 0xA5
BYTE_GUARD = 4096               # bytes on each side of every buffer: four fragments of a packed image


class ByteArena:
    """Arena's sibling for byte buffers (test_gpu_pack_device.py): one uint8 allocation filled with BYTE_SENTINEL, every buffer an
    interior view at a 256-byte aligned offset with at least `guard` sentinel bytes on both sides.  The buffers themselves start
    out as sentinel too, so a caller sees which of their bytes a kernel wrote."""

    def __init__(self, dev, sizes, guard=BYTE_GUARD):
        """sizes: [(name, bytes)]"""
        self.off, o = {}, guard
        for name, n in sizes:
            self.off[name] = (o, n)
            o = (o + n + guard + 255) // 256 * 256
        self.buf = torch.full((o,), BYTE_SENTINEL, device=dev, dtype=torch.uint8)
        assert self.buf.data_ptr() % 256 == 0
        inside = torch.zeros(o, dtype=torch.bool, device=dev)
        for a, n in self.off.values():
            inside[a:a + n] = True
        self.guard = ~inside

    def view(self, name):
        o, n = self.off[name]
        return self.buf[o:o + n]

    def guards_intact(self):
        return bool((self.buf[self.guard] == BYTE_SENTINEL).all())
