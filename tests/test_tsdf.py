"""CPU tests of the depth-fusion boundary: every refusal of pnr_tsdf_integrate, ops.tsdf_integrate and fusion.* happens before
any launch and names its argument; a Volume's initial values; label packing and unpacking."""
import ctypes

import numpy as np
import pytest
import torch

import _camera_ref as cr
import _tsdf_ref as tr
from panopticnerf_amd import FrameSet, _lib, fusion, ops

NULL = ctypes.c_void_p(0)
PTR = ctypes.c_void_p(4096)             # non-null and aligned, never dereferenced: validation fails first
F3 = ctypes.c_float * 3
INF = float("inf")
NAN = float("nan")


def refused(rc, *words):
    msg = _lib.load().pnr_last_error()
    return rc == -1 and all(w.encode() in msg for w in words)


def call(frames=PTR, w2c=PTR, f0=0, f1=1, res=(4, 4, 4), lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), trunc=0.5, max_depth=INF, w_max=INF,
         tsdf=PTR, weight=PTR, rgb=NULL, rgb_weight=NULL, label=NULL, conf=NULL):
    lo = None if lo is None else F3(*lo)
    step = None if step is None else F3(*step)
    return _lib.load().pnr_tsdf_integrate(frames, w2c, f0, f1, res[0], res[1], res[2], lo, step, trunc, max_depth, w_max, tsdf, weight, rgb,
                                          rgb_weight, label, conf, NULL)


# ---------------------------------------------------------------- the entry point
def test_entry_point_refuses_before_any_launch():
    who = "pnr_tsdf_integrate"
    assert refused(call(frames=NULL), who, "null frames or w2c")
    assert refused(call(w2c=NULL), who, "null frames or w2c")
    assert refused(call(tsdf=NULL), who, "null tsdf or weight")
    assert refused(call(weight=NULL), who, "null tsdf or weight")
    assert refused(call(rgb=PTR), who, "rgb and rgb_weight go together")
    assert refused(call(rgb_weight=PTR), who, "rgb and rgb_weight go together")
    assert refused(call(label=PTR), who, "label and conf go together")
    assert refused(call(conf=PTR), who, "label and conf go together")
    assert refused(call(frames=ctypes.c_void_p(4104)), who, "misaligned table")
    assert refused(call(w2c=ctypes.c_void_p(4100)), who, "misaligned table")
    for name in ("tsdf", "weight"):
        assert refused(call(**{name: ctypes.c_void_p(4098)}), who, "misaligned volume array"), name
    for pair in (("rgb", "rgb_weight"), ("label", "conf")):
        for k in range(2):
            kw = {pair[0]: PTR, pair[1]: PTR}
            kw[pair[k]] = ctypes.c_void_p(4097)
            assert refused(call(**kw), who, "misaligned volume array"), pair[k]
    for f0, f1 in ((-1, 1), (2, 1), (-2, -1)):
        assert refused(call(f0=f0, f1=f1), who, "bad frame range")
    for res in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1 << 16, 1 << 16, 1), (1290, 1290, 1291), (2 ** 31 - 1, 2, 1)):
        assert refused(call(res=res), who, "lattice"), res
    assert refused(call(lo=None), who, "null lo or step")
    assert refused(call(step=None), who, "null lo or step")
    for axis in range(3):
        for bad in (NAN, INF, -INF):
            v = [0.5, 0.5, 0.5]
            v[axis] = bad
            assert refused(call(lo=v), who, "finite", "axis %d" % axis)
            assert refused(call(step=v), who, "finite", "axis %d" % axis)
        v = [0.5, 0.5, 0.5]
        v[axis] = 0.0
        assert refused(call(step=v), who, "step non-zero", "axis %d" % axis)
        v[axis] = -0.0
        assert refused(call(step=v), who, "step non-zero", "axis %d" % axis)
    for trunc in (0.0, -1.0, NAN, INF, -INF):
        assert refused(call(trunc=trunc), who, "trunc"), trunc
    for md in (0.0, -2.0, NAN, -INF):
        assert refused(call(max_depth=md), who, "max_depth"), md
    for wm in (0.0, 0.5, -1.0, NAN, -INF):
        assert refused(call(w_max=wm), who, "w_max"), wm
    # an empty frame range is PNR_OK at once (nothing is launched: these pointers could not be read), after the checks
    assert call(f0=0, f1=0) == 0 and call(f0=5, f1=5, rgb=PTR, rgb_weight=PTR, label=PTR, conf=PTR, max_depth=3.0, w_max=1.0) == 0
    assert call(f0=0, f1=0, res=(2 ** 31 - 1, 1, 1)) == 0 and call(f0=0, f1=0, res=(1290, 1290, 1290)) == 0
    assert refused(call(f0=3, f1=3, trunc=0.0), who, "trunc")


def test_launch_constants_match_the_header():
    assert ops.TSDF_BLOCK == cr._header_constant("PNR_TSDF_BLOCK") and ops.TSDF_BLOCKS_PER_CU == cr._header_constant("PNR_TSDF_BLOCKS_PER_CU")
    assert ops.TSDF_MAX_POINTS == 2 ** 31 - 1


# ---------------------------------------------------------------- ops
def test_ops_refuse_by_name():
    rec = ctypes.sizeof(_lib.Frame)
    table, w2c = torch.zeros(2 * rec, dtype=torch.uint8), torch.zeros(2, 12)
    t, w = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)
    lo, step = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    go = lambda *a, **kw: ops.tsdf_integrate(*a, **kw)
    with pytest.raises(RuntimeError, match="tsdf_integrate: tsdf.*no CPU fallback"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        go(table, w2c, 0, 0, lo, step, 0.5, t, w)
    with pytest.raises(ValueError, match="tsdf must be a GPU tensor"):
        go(table, w2c, 0, 1, lo, step, 0.5, np.zeros((3, 4, 5), np.float32), w)
    for bad in (torch.zeros(4, 5), torch.zeros(0, 4, 5), torch.zeros(2, 3, 4, 5)):
        with pytest.raises(ValueError, match=r"tsdf must be \(res_z, res_y, res_x\)"):
            go(table, w2c, 0, 1, lo, step, 0.5, bad, w)
    with pytest.raises(ValueError, match="more than the limit"):
        go(table, w2c, 0, 1, lo, step, 0.5, torch.zeros(1).expand(1291, 1290, 1290), w)
    with pytest.raises(TypeError, match="tsdf must be torch.float32"):
        go(table, w2c, 0, 1, lo, step, 0.5, t.double(), w)
    with pytest.raises(TypeError, match="weight must be torch.float32"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w.half())
    with pytest.raises(ValueError, match="weight must be a GPU tensor"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, None)
    with pytest.raises(ValueError, match=r"weight must be \(3, 4, 5\)"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, torch.zeros(3, 4, 6))
    with pytest.raises(ValueError, match="rgb and rgb_weight go together"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, rgb=torch.zeros(3, 4, 5, 3))
    with pytest.raises(ValueError, match="rgb and rgb_weight go together"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, rgb_weight=w.clone())
    with pytest.raises(ValueError, match="label and conf go together"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, label=torch.zeros(3, 4, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="label and conf go together"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, conf=torch.zeros(3, 4, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"rgb must be \(3, 4, 5, 3\)"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, rgb=torch.zeros(3, 4, 5), rgb_weight=w.clone())
    with pytest.raises(TypeError, match="rgb must be torch.float32"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, rgb=torch.zeros(3, 4, 5, 3, dtype=torch.uint8), rgb_weight=w.clone())
    with pytest.raises(TypeError, match="label must be torch.int32"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, label=torch.zeros(3, 4, 5, dtype=torch.int64), conf=torch.zeros(3, 4, 5, dtype=torch.int32))
    with pytest.raises(TypeError, match="conf must be torch.int32"):
        go(table, w2c, 0, 1, lo, step, 0.5, t, w, label=torch.zeros(3, 4, 5, dtype=torch.int32), conf=torch.zeros(3, 4, 5))
    with pytest.raises(ValueError, match="frames must be a uint8 tensor of whole pnr_frame records"):
        go(table[:-1], w2c, 0, 1, lo, step, 0.5, t, w)
    with pytest.raises(ValueError, match="frames must be a uint8 tensor"):
        go(table.int(), w2c, 0, 1, lo, step, 0.5, t, w)
    with pytest.raises(ValueError, match=r"w2c must be an \(F, 12\) float32 tensor"):
        go(table, torch.zeros(2, 3, 4), 0, 1, lo, step, 0.5, t, w)
    with pytest.raises(ValueError, match=r"w2c must be an \(F, 12\) float32 tensor"):
        go(table, w2c.double(), 0, 1, lo, step, 0.5, t, w)
    for first, last in ((-1, 1), (2, 1), (0, 3), (3, 3)):
        with pytest.raises(ValueError, match="need 0 <= first <= last <= 2"):
            go(table, w2c, first, last, lo, step, 0.5, t, w)
    with pytest.raises(ValueError, match="need 0 <= first <= last <= 1"):
        go(table, w2c[:1], 0, 2, lo, step, 0.5, t, w)
    with pytest.raises(ValueError, match="tsdf_integrate: lo"):
        go(table, w2c, 0, 1, (0.0, 0.0), step, 0.5, t, w)
    with pytest.raises(ValueError, match="lo must be finite"):
        go(table, w2c, 0, 1, (0.0, NAN, 0.0), step, 0.5, t, w)
    with pytest.raises(ValueError, match="step must be finite"):
        go(table, w2c, 0, 1, lo, (1.0, 1.0, INF), 0.5, t, w)
    with pytest.raises(ValueError, match="step must be non-zero"):
        go(table, w2c, 0, 1, lo, (1.0, 0.0, 1.0), 0.5, t, w)
    for trunc in (0.0, -0.5, NAN, INF):
        with pytest.raises(ValueError, match="trunc must be positive and finite"):
            go(table, w2c, 0, 1, lo, step, trunc, t, w)
    for md in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="max_depth must be positive"):
            go(table, w2c, 0, 1, lo, step, 0.5, t, w, max_depth=md)
    for wm in (0.0, 0.999, NAN):
        with pytest.raises(ValueError, match="w_max must be >= 1"):
            go(table, w2c, 0, 1, lo, step, 0.5, t, w, w_max=wm)


# ---------------------------------------------------------------- fusion
def test_volume_initial_values_and_refusals():
    v = fusion.Volume((-1, 0, 1), (1, 3, 2), (8, 5, 3), "cpu", color=True, labels=True)
    assert v.res == (8, 5, 3) and repr(v) == "Volume(8 x 5 x 3, color, labels)"
    assert tuple(v.tsdf.shape) == tuple(v.weight.shape) == tuple(v.rgb_weight.shape) == tuple(v.label.shape) == tuple(v.conf.shape) == (3, 5, 8)
    assert tuple(v.rgb.shape) == (3, 5, 8, 3)
    assert v.tsdf.dtype == v.weight.dtype == v.rgb.dtype == v.rgb_weight.dtype == torch.float32 and v.label.dtype == v.conf.dtype == torch.int32
    for t in (v.tsdf, v.weight, v.rgb, v.rgb_weight, v.conf):
        assert not t.any() and t.is_contiguous()
    assert (v.label == -1).all()
    assert (v.sem_label == -1).all() and (v.inst_label == -1).all() and v.sem_label.dtype == torch.int32
    assert v.colors().dtype == torch.uint8 and not v.colors().any() and tuple(v.colors().shape) == (3, 5, 8, 3)
    import _mesh_ref as mr
    rlo, rstep = mr.lattice((-1, 0, 1), (1, 3, 2), (8, 5, 3))
    assert np.array_equal(v.lo32, rlo) and np.array_equal(v.step, rstep) and v.step.dtype == np.float32
    # reset() restores them
    v.tsdf.fill_(0.5); v.weight.fill_(2); v.rgb.fill_(100.4); v.rgb_weight.fill_(2); v.label.fill_(tr.pack(3, -1)); v.conf.fill_(7)
    assert (v.sem_label == 3).all() and (v.inst_label == -1).all() and (v.colors() == 100).all()
    v.rgb.fill_(100.5)
    assert (v.colors() == 100).all()            # ties to even, as torch.round
    v.rgb.fill_(255.0)
    assert (v.colors() == 255).all()
    v.reset()
    assert not v.tsdf.any() and not v.weight.any() and not v.rgb.any() and not v.rgb_weight.any() and not v.conf.any() and (v.label == -1).all()
    bare = fusion.Volume((0, 0, 0), (1, 1, 1), 4, "cpu")
    assert bare.res == (4, 4, 4) and bare.rgb is None and bare.rgb_weight is None and bare.label is None and bare.conf is None
    assert repr(bare) == "Volume(4 x 4 x 4)"
    with pytest.raises(ValueError, match="made without labels"):
        bare.sem_label
    with pytest.raises(ValueError, match="made without labels"):
        bare.inst_label
    with pytest.raises(ValueError, match="made without colour"):
        bare.colors()
    for res in ((4, 4), (4, 0, 4), "abc", (4, 4, -1), 0):
        with pytest.raises(ValueError, match="fusion.Volume: res"):
            fusion.Volume((0, 0, 0), (1, 1, 1), res, "cpu")
    with pytest.raises(ValueError, match="more than the limit"):
        fusion.Volume((0, 0, 0), (1, 1, 1), (1291, 1290, 1290), "cpu")
    with pytest.raises(ValueError, match="mesh: lo must be three numbers"):
        fusion.Volume((0, 0), (1, 1, 1), 4, "cpu")
    with pytest.raises(ValueError, match="mesh: hi must be finite"):
        fusion.Volume((0, 0, 0), (1, NAN, 1), 4, "cpu")
    with pytest.raises(ValueError, match="empty along an axis"):
        fusion.Volume((0, 0, 0), (1, 0, 1), 4, "cpu")


def test_integrate_and_extract_refuse_by_name():
    v = fusion.Volume((0, 0, 0), (1, 1, 1), 4, "cpu")
    frames = FrameSet("cuda:0", capacity=4)                 # no frame added: nothing touches a GPU
    with pytest.raises(TypeError, match="volume must be a fusion.Volume"):
        fusion.integrate(v.tsdf, frames, 0.5)
    with pytest.raises(TypeError, match="frames must be a FrameSet"):
        fusion.integrate(v, [], 0.5)
    for first, last in ((-1, None), (1, None), (0, 1), (1, 0)):
        with pytest.raises(ValueError, match="need 0 <= first <= last <= 0"):
            fusion.integrate(v, frames, 0.5, first=first, last=last)
    for trunc in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="fusion.integrate: trunc must be positive and finite"):
            fusion.integrate(v, frames, trunc)
    with pytest.raises(ValueError, match="fusion.integrate: max_depth must be positive"):
        fusion.integrate(v, frames, 0.5, max_depth=0.0)
    with pytest.raises(ValueError, match="fusion.integrate: w_max must be >= 1"):
        fusion.integrate(v, frames, 0.5, w_max=0.5)
    with pytest.raises(RuntimeError, match="fusion.integrate: the volume is not on the GPU.*no CPU fallback"):
        fusion.integrate(v, frames, 0.5)
    with pytest.raises(TypeError, match="fusion.extract: volume must be a fusion.Volume"):
        fusion.extract(v.tsdf)
    for mw in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="fusion.extract: min_weight must be positive"):
            fusion.extract(v, min_weight=mw)
    with pytest.raises(RuntimeError, match="fusion.extract: the volume is not on the GPU.*no CPU fallback"):
        fusion.extract(v)


# ---------------------------------------------------------------- labels
def test_label_packing():
    sem = torch.tensor([0, 1, 5, 32767, 32767, -1, -1, 7, 0], dtype=torch.int16)
    inst = torch.tensor([0, -1, 300, -1, -32768, 4, -1, 32767, 65], dtype=torch.int16)
    key = fusion.pack_label(sem, inst)
    assert key.dtype == torch.int32
    want = [tr.pack(s, i) if s >= 0 else -1 for s, i in zip(sem.tolist(), inst.tolist())]
    assert key.tolist() == want and all(k >= -1 for k in want) and key[3].item() == 2 ** 31 - 1
    s2, i2 = fusion.unpack_label(key)
    assert s2.dtype == i2.dtype == torch.int32
    assert s2.tolist() == [0, 1, 5, 32767, 32767, -1, -1, 7, 0] and i2.tolist() == [0, -1, 300, -1, -32768, -1, -1, 32767, 65]
    rs, ri = tr.unpack(np.asarray(want, np.int32))
    assert rs.tolist() == s2.tolist() and ri.tolist() == i2.tolist()
    assert fusion.pack_label(3, 7).item() == (3 << 16) | 7 and fusion.LABEL_NONE == -1
