"""A CPU tensor that says it is on the GPU: the ops' checks behind the device check (contiguity, "is on cuda:1, not on ...", a
CPU tensor among GPU ones) run on a machine without one.  A test helper, not a test; nothing here touches a GPU."""
import torch


class _FakeCuda(torch.Tensor):
    """a CPU tensor that says it is on the GPU (and, with `device`, on which): lets the checks behind `is_cuda` run without one.
    A tensor made from one (a view, a reshape) says it is on the GPU too, on the default device."""
    @staticmethod
    def __new__(cls, t, device=None):
        self = torch.Tensor._make_subclass(cls, t)
        self._says = device
        return self

    def __init__(self, t, device=None):
        pass

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        out = super().__torch_function__(func, types, args, kwargs)
        if isinstance(out, _FakeCuda) and not hasattr(out, "_says"):
            out._says = next((a._says for a in args if isinstance(a, _FakeCuda)), None)
        return out

    @property
    def is_cuda(self):
        return True

    @property
    def device(self):
        return torch.device(self._says) if self._says else torch.device("cpu")


def _fake(t, device=None):
    return _FakeCuda(t, device)


def z(*shape, dtype=torch.float32, device=None):
    """a contiguous fake GPU tensor of zeros"""
    return _fake(torch.zeros(*shape, dtype=dtype), device)


def zt(*shape, dtype=torch.float32):
    """a NON-contiguous fake GPU tensor of that shape: the last two axes of its memory are swapped (1-D: every second element)"""
    if len(shape) == 1:
        return _fake(torch.zeros(2 * shape[0], dtype=dtype)[::2])
    return _fake(torch.zeros(*shape[:-2], shape[-1], shape[-2], dtype=dtype).transpose(-1, -2))


def cpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)
