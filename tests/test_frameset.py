"""CPU tests of the training-frame surface (panopticnerf_amd/data.py, ops.sample_batch, pnr_sample_batch): every refusal of
FrameSet.add / set_boxes / sample happens on host values before any device work, and the C entry point rejects bad arguments
with PNR_EINVAL before any launch (libpnr.so loads without a GPU, as in tests/test_abi.py)."""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

from panopticnerf_amd import FrameSet, Fisheye, Pinhole, _lib, ops, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 24, 16


def _cam():
    return Pinhole(20.0, 20.0, 11.5, 7.5, W, H)


def _pose():
    return torch.eye(4)[:3]


def _rgb():
    return torch.zeros(H, W, 3, dtype=torch.uint8)


def test_frame_record_matches_the_header():
    """_lib.Frame is, field by field, the pnr_frame of include/pnr.h: 144 bytes at the offsets its comment states."""
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    body = re.search(r"typedef struct pnr_frame \{(.*?)\} pnr_frame;", hdr, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, rest = decl.split(None, 1)
            names += [(n.strip().split("[")[0], ty) for n in rest.split(",")]
    assert [n for n, _ in names] == [n for n, *_ in _lib.Frame._fields_]
    assert ctypes.sizeof(_lib.Frame) == 144 and ctypes.sizeof(_lib.Frame) % 16 == 0
    stated = {n: int(o) for o, n in re.findall(r"\*\s+(?:offset\s+)?(\d+)\s+(?:int32|float|int64|uint64)\s+(\w+)", hdr)}
    for name in ("model", "cam", "c2w", "near_", "n_valid", "valid_pix", "rgb", "depth", "sem", "inst"):
        assert getattr(_lib.Frame, name).offset == stated[name], name
    assert (_lib.TAG_PIXEL, _lib.TAG_FRAME) == tuple(int(re.search(r"#define\s+%s\s+(\d+)" % n, hdr).group(1)) for n in ("PNR_TAG_PIXEL", "PNR_TAG_FRAME"))


def test_cpu_device_and_capacity_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FrameSet("cpu")
    with pytest.raises(ValueError, match="capacity"):
        FrameSet("cuda", capacity=0)
    fs = FrameSet("cuda", capacity=2)
    fs.frames += [{}, {}]                    # (two frames' worth of host records: nothing here needs the device)
    with pytest.raises(RuntimeError, match="full"):
        fs.add(_cam(), _pose(), 0.5, 50.0, _rgb())


def test_add_refuses_bad_images_before_touching_the_device():
    fs = FrameSet("cuda", capacity=4)
    ok = dict(camera=_cam(), c2w=_pose(), near=0.5, far=50.0)
    with pytest.raises(TypeError, match="camera"):
        fs.add("pinhole", _pose(), 0.5, 50.0, _rgb())
    with pytest.raises(ValueError, match="c2w"):
        fs.add(_cam(), torch.eye(3), 0.5, 50.0, _rgb())
    for bad in (torch.zeros(H, W + 1, 3, dtype=torch.uint8), torch.zeros(W, H, 3, dtype=torch.uint8), torch.zeros(H, W, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="rgb must be"):
            fs.add(rgb=bad, **ok)
    with pytest.raises(TypeError, match="uint8 or float"):
        fs.add(rgb=torch.zeros(H, W, 3, dtype=torch.int32), **ok)
    for bad in (torch.full((H, W, 3), 1.5), torch.full((H, W, 3), -0.1), torch.full((H, W, 3), float("nan")), torch.full((H, W, 3), 200.0)):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            fs.add(rgb=bad, **ok)
    with pytest.raises(ValueError, match="depth must be"):
        fs.add(rgb=_rgb(), depth=torch.zeros(H, W + 1), **ok)
    with pytest.raises(TypeError, match="depth"):
        fs.add(rgb=_rgb(), depth=torch.zeros(H, W, dtype=torch.int32), **ok)
    for key in ("pseudo_label", "instance_label"):
        with pytest.raises(ValueError, match=key + " must be"):
            fs.add(rgb=_rgb(), **{key: torch.zeros(H + 1, W, dtype=torch.int64)}, **ok)
        with pytest.raises(TypeError, match=key):
            fs.add(rgb=_rgb(), **{key: torch.zeros(H, W)}, **ok)
        for v in (32768, -32769, 10 ** 6):
            lab = torch.zeros(H, W, dtype=torch.int64)
            lab[3, 5] = v
            with pytest.raises(ValueError, match="int16"):
                fs.add(rgb=_rgb(), **{key: lab}, **ok)
    # a fisheye frame is checked against ITS camera's size
    fish = Fisheye(2.2134, 0.016798, 1.6548, 22.9, 22.9, 11.5, 7.5, W, H)
    with pytest.raises(ValueError, match="rgb must be"):
        fs.add(fish, _pose(), 0.5, 50.0, torch.zeros(H, H, 3, dtype=torch.uint8))
    assert len(fs) == 0 and fs.table is None           # nothing was added, no device memory was asked for


def test_set_boxes_and_sample_refusals():
    fs = FrameSet("cuda")
    with pytest.raises(ValueError, match=r"\(M, 15\)"):
        fs.set_boxes(torch.zeros(4, 14), torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="bbox_ids"):
        fs.set_boxes(torch.zeros(4, 15), torch.zeros(3, 2, dtype=torch.int32))
    with pytest.raises(TypeError, match="integers"):
        fs.set_boxes(torch.zeros(4, 15), torch.zeros(4, 2))
    with pytest.raises(ValueError, match="mode"):
        fs.sample(16, mode="random")
    for rank, world in ((1, 1), (-1, 2), (4, 4), (0, 0)):
        with pytest.raises(ValueError, match="rank"):
            fs.sample(16, rank=rank, world=world)
    with pytest.raises(ValueError, match="n_rays"):
        fs.sample(-1)
    with pytest.raises(ValueError, match="2\\^32"):
        fs.sample(2 ** 30, rank=0, world=8)
    with pytest.raises(ValueError, match="sample\\(\\) returned"):
        fs.sample(16, out={"rays": None})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_batch(torch.zeros(144, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32),
                         ops.Draw(torch.zeros(2, dtype=torch.int64), 16), 4)


def test_byte_over_255_through_float64_is_the_float32_quotient():
    """FrameSet.frame_batch divides in float64 and rounds; pnr_sample_batch divides in float32 (correctly rounded): the same 256 values."""
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal((v.double() / 255.0).float(), v.float() / 255.0)
    assert np.array_equal((np.arange(256) / 255.0).astype(np.float32), np.arange(256, dtype=np.float32) / np.float32(255))


def test_graphed_step_argument_rules():
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    with pytest.raises(ValueError, match="n_rays"):
        train.GraphedStep(None, opt, frames=FrameSet("cuda"))
    with pytest.raises(ValueError, match="no example batch"):
        train.GraphedStep(None, opt, {"rays": torch.zeros(1, 4, 8)}, frames=FrameSet("cuda"), n_rays=4)
    with pytest.raises(ValueError, match="example batch"):
        train.GraphedStep(None, opt)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    null, a16, a8 = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)       # never dereferenced: validation fails first
    rng = lambda tag=16, base=0, call=4096: ctypes.byref(_lib.RngDesc(call, base, tag, 1.0))
    call = lambda frames=a16, cum=a16, nf=a16, mode=0, r=None, n=64, rays=a16: lib.pnr_sample_batch(
        frames, cum, nf, mode, r if r is not None else rng(), n, rays, null, null, null, null, null, null, null)
    for kw in (dict(frames=null), dict(cum=null), dict(nf=null)):
        assert call(**kw) == -1 and b"null frame table" in lib.pnr_last_error()
    for kw in (dict(frames=a8), dict(cum=ctypes.c_void_p(4100)), dict(nf=ctypes.c_void_p(4098))):
        assert call(**kw) == -1 and b"misaligned frame table" in lib.pnr_last_error()
    for mode in (-1, 2, 7):
        assert call(mode=mode) == -1 and b"mode" in lib.pnr_last_error()
    assert call(r=ctypes.POINTER(_lib.RngDesc)()) == -1 and b"null rng" in lib.pnr_last_error()
    assert call(r=rng(call=0)) == -1 and b"null rng" in lib.pnr_last_error()
    for tag in (0, 256, -3):
        assert call(r=rng(tag=tag)) == -1 and b"outside [1,255]" in lib.pnr_last_error()
    for tag in (1, 2, 3, 4, 15, 17, 18, 254, 255):  # the render streams' tags, the frame stream's, anything but PNR_TAG_PIXEL
        assert call(r=rng(tag=tag)) == -1 and b"tag clash" in lib.pnr_last_error(), tag
    assert call(r=rng(base=-1)) == -1 and call(r=rng(base=2 ** 32 - 63)) == -1 and b"2^32" in lib.pnr_last_error()
    assert call(n=-1) == -1
    assert call(rays=a8) == -1 and b"16-byte aligned" in lib.pnr_last_error()
    assert call(n=0) == 0 and call(n=0, rays=null) == 0                                    # an empty batch is a no-op
