"""CPU tests of the geometry ops' refusals BEHIND the device check, and of the order in which two faults are reported: contiguity
(the kernels index flat: a transposed view of the right shape is stopped only here), a tensor on another device, a CPU tensor
among GPU ones, optional outputs that are no tensors, and double faults.  Every case names the exception type and the WHOLE message.
The tensors are _fake_gpu's: CPU tensors that say they are on the GPU, passed to the op behind `_on_device` (`op.__wrapped__`),
which would ask the runtime for the current device.  Every case is refused before the entry point is called (asking for the
stream, the last thing before it, fails the test).  An op with one tensor argument has no "other device" case.
`_chk` and `_own`, the hot path's helpers, test no type: a non-tensor that reaches them is an AttributeError, pinned as it is.
Nothing here touches a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from panopticnerf_amd import Pinhole, _lib, ops

from _fake_gpu import _fake, cpu, z, zt

H, W = 12, 16                      # the images of test_icp.py
RZ, RY, RX = 3, 4, 5                # a lattice of a few points per axis
EYE = torch.eye(4)[:3]
PIN = (50.0, 50.0, 8.0, 6.0)
CAM = Pinhole(*PIN, W, H)
REC = ctypes.sizeof(_lib.Frame)
NO_GPU = " (the HIP path has no CPU fallback)"
f32, f64, i16, i32, i64, u8 = torch.float32, torch.float64, torch.int16, torch.int32, torch.int64, torch.uint8


@pytest.fixture(autouse=True)
def _no_launch(monkeypatch):
    def stream():
        raise AssertionError("not refused: the op went on to its entry point")
    monkeypatch.setattr(ops, "_stream", stream)


def _mesh_bytes():
    return ops.mesh_workspace_bytes(RX, RY, RZ)


BASE = {
    "tsdf_integrate": lambda: dict(frames=z(2 * REC, dtype=u8), w2c=z(2, 12), first=0, last=2, lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), trunc=0.5,
                                   tsdf=z(RZ, RY, RX), weight=z(RZ, RY, RX), rgb=z(RZ, RY, RX, 3), rgb_weight=z(RZ, RY, RX),
                                   label=z(RZ, RY, RX, dtype=i32), conf=z(RZ, RY, RX, dtype=i32)),
    "tsdf_raycast": lambda: dict(camera_model="pinhole", cam=PIN, c2w=EYE, width=W, height=H, near=0.1, far=5.0, lo=(0.0, 0.0, 0.0),
                                 step=(1.0, 1.0, 1.0), tsdf=z(RZ, RY, RX), weight=z(RZ, RY, RX), depth=z(H, W), code=z(H, W, dtype=u8),
                                 normal=z(H, W, 3), src=z(H, W, dtype=i32)),
    "mesh_count": lambda: dict(field=z(RZ, RY, RX), level=0.0, workspace=z(_mesh_bytes(), dtype=u8), totals=z(2, dtype=i64)),
    "mesh_emit": lambda: dict(field=z(RZ, RY, RX), level=0.0, lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), workspace=z(_mesh_bytes(), dtype=u8),
                              vertices=z(6, 3), faces=z(2, 3, dtype=i32), src=z(6, dtype=i64)),
    "splat_points": lambda: dict(camera=CAM, w2c=EYE, points=z(7, 3), zbuf=z(H, W, dtype=i64), stats=z(3, dtype=i64)),
    "splat_resolve": lambda: dict(zbuf=z(H, W, dtype=i64, device="cuda:0"), want=("depth",), out={"depth": z(H, W, device="cuda:0")}),
    "depth_metrics": lambda: dict(pred=z(H, W), gt=z(H, W), mask=z(H, W, dtype=u8), sums=z(5, dtype=f64), counts=z(5, dtype=i64)),
    "reproject": lambda: dict(src=CAM, c2w_src=EYE, depth_src=z(H, W, device="cuda:0"), tgt=CAM, w2c_tgt=EYE, depth_tgt=z(H, W, device="cuda:0"),
                              pix=z(5, dtype=i32, device="cuda:0"), label_src=z(H, W, dtype=i32, device="cuda:0"),
                              label_tgt=z(H, W, dtype=i32, device="cuda:0"), n_classes=3, agree=z(3, 3, dtype=i64, device="cuda:0"),
                              stats=z(5, dtype=i64, device="cuda:0"), want=("match",), out={"match": z(5, dtype=i32, device="cuda:0")}),
    "project_points": lambda: dict(model="pinhole", cam=PIN, w2c=EYE, width=W, height=H, points=z(7, 3)),
    "census": lambda: dict(img=z(H, W, dtype=u8), out=z(H, W, dtype=i64)),
    "sgm_aggregate": lambda: dict(census_l=z(H, W, dtype=i64), census_r=z(H, W, dtype=i64), max_disp=16, out=z(H, W, 16, dtype=i16)),
    "sgm_select": lambda: dict(S=z(H, W, 16, dtype=i16), out=z(H, W, dtype=i16), disp_right=z(H, W, dtype=i16)),
    "disparity_depth": lambda: dict(d16=z(H, W, dtype=i16), fb=100.0, out=z(H, W)),
}

V, T = ValueError, TypeError
CONTIG = ": tensor must be contiguous"
INF = float("inf")

CASES = [
    # ------------------------------------------------------------------------------------------------ tsdf_integrate
    ("tsdf_integrate", dict(tsdf=zt(RZ, RY, RX)), V, "tsdf_integrate: tsdf" + CONTIG),
    ("tsdf_integrate", dict(weight=zt(RZ, RY, RX)), V, "tsdf_integrate: weight" + CONTIG),
    ("tsdf_integrate", dict(rgb=_fake(torch.zeros(RZ, RX, RY, 3).transpose(1, 2))), V, "tsdf_integrate: rgb" + CONTIG),
    ("tsdf_integrate", dict(rgb_weight=zt(RZ, RY, RX)), V, "tsdf_integrate: rgb_weight" + CONTIG),
    ("tsdf_integrate", dict(label=zt(RZ, RY, RX, dtype=i32)), V, "tsdf_integrate: label" + CONTIG),
    ("tsdf_integrate", dict(conf=zt(RZ, RY, RX, dtype=i32)), V, "tsdf_integrate: conf" + CONTIG),
    ("tsdf_integrate", dict(frames=zt(2 * REC, dtype=u8)), V, "tsdf_integrate: frames" + CONTIG),
    ("tsdf_integrate", dict(w2c=zt(2, 12)), V, "tsdf_integrate: w2c" + CONTIG),
    ("tsdf_integrate", dict(weight=z(RZ, RY, RX, device="cuda:1")), V, "tsdf_integrate: weight is on cuda:1, not on cpu"),
    ("tsdf_integrate", dict(frames=z(2 * REC, dtype=u8, device="cuda:1")), V, "tsdf_integrate: frames is on cuda:1, not on cpu"),
    ("tsdf_integrate", dict(w2c=cpu(2, 12)), RuntimeError, "tsdf_integrate: w2c: expected a GPU tensor" + NO_GPU),
    ("tsdf_integrate", dict(tsdf=cpu(RZ, RY, RX)), RuntimeError, "tsdf_integrate: tsdf: expected a GPU tensor" + NO_GPU),
    ("tsdf_integrate", dict(rgb=[0.0]), V, "tsdf_integrate: rgb must be a GPU tensor, got list"),
    ("tsdf_integrate", dict(rgb_weight=np.zeros((RZ, RY, RX), np.float32)), V, "tsdf_integrate: rgb_weight must be a GPU tensor, got ndarray"),
    ("tsdf_integrate", dict(label=0), V, "tsdf_integrate: label must be a GPU tensor, got int"),
    ("tsdf_integrate", dict(conf="conf"), V, "tsdf_integrate: conf must be a GPU tensor, got str"),
    ("tsdf_integrate", dict(weight=z(RZ, RY, RX + 1, dtype=f64)), T, "tsdf_integrate: weight must be torch.float32, got torch.float64"),
    ("tsdf_integrate", dict(trunc=0.0, weight=z(RZ, RY, RX, device="cuda:1")), V, "tsdf_integrate: trunc must be positive and finite (got 0.0)"),
    ("tsdf_integrate", dict(lo=(INF, 0.0, 0.0), step=(1.0, 0.0, 1.0)), V, "tsdf_integrate: lo must be finite (got [inf, 0.0, 0.0])"),
    ("tsdf_integrate", dict(tsdf=z(RY, RX), rgb_weight=None), V, "tsdf_integrate: tsdf must be (res_z, res_y, res_x) with every res >= 1, got (4, 5)"),
    ("tsdf_integrate", dict(conf=None, rgb=z(RZ, RY, RX)), V, "tsdf_integrate: label and conf go together (both or neither)"),
    ("tsdf_integrate", dict(last=3, step=(0.0, 1.0, 1.0)), V,
     "tsdf_integrate: need 0 <= first <= last <= 2 (the records and w2c rows given), got [0, 3)"),
    ("tsdf_integrate", dict(w_max=0.5, max_depth=0.0), V, "tsdf_integrate: max_depth must be positive (it may be inf; got 0.0)"),
    ("tsdf_integrate", dict(frames=z(2 * REC + 1, dtype=u8), w2c=z(2, 11)), V,
     "tsdf_integrate: frames must be a uint8 tensor of whole pnr_frame records (%d bytes each)" % REC),
    # ------------------------------------------------------------------------------------------------ tsdf_raycast
    ("tsdf_raycast", dict(tsdf=zt(RZ, RY, RX)), V, "tsdf_raycast: tsdf" + CONTIG),
    ("tsdf_raycast", dict(weight=zt(RZ, RY, RX)), V, "tsdf_raycast: weight" + CONTIG),
    ("tsdf_raycast", dict(depth=zt(H, W)), V, "tsdf_raycast: depth" + CONTIG),
    ("tsdf_raycast", dict(code=zt(H, W, dtype=u8)), V, "tsdf_raycast: code" + CONTIG),
    ("tsdf_raycast", dict(normal=_fake(torch.zeros(H, 3, W).transpose(1, 2))), V, "tsdf_raycast: normal" + CONTIG),
    ("tsdf_raycast", dict(src=zt(H, W, dtype=i32)), V, "tsdf_raycast: src" + CONTIG),
    ("tsdf_raycast", dict(code=z(H, W, dtype=u8, device="cuda:1")), V, "tsdf_raycast: code is on cuda:1, not on cpu"),
    ("tsdf_raycast", dict(depth=cpu(H, W)), RuntimeError, "tsdf_raycast: depth: expected a GPU tensor" + NO_GPU),
    ("tsdf_raycast", dict(normal=[0.0]), V, "tsdf_raycast: normal must be a GPU tensor, got list"),
    ("tsdf_raycast", dict(src=np.zeros((H, W), np.int32)), V, "tsdf_raycast: src must be a GPU tensor, got ndarray"),
    ("tsdf_raycast", dict(depth=z(W, H, dtype=f64)), T, "tsdf_raycast: depth must be torch.float32, got torch.float64"),
    ("tsdf_raycast", dict(near=2.0, far=1.0, code=z(H, W, dtype=u8, device="cuda:1")), V, "tsdf_raycast: need 0 <= near < far (got 2.0, 1.0)"),
    ("tsdf_raycast", dict(camera_model="ortho", width=0), V, "tsdf_raycast: camera_model must be 'pinhole', 'fisheye' or 'equirect', not 'ortho'"),
    ("tsdf_raycast", dict(cam=(1.0, 2.0), c2w=torch.eye(3)), V, "tsdf_raycast: model 'pinhole' cam: expected 4 values, got 2"),
    ("tsdf_raycast", dict(width=0, tsdf=None), V, "tsdf_raycast: bad image 0 x 12 (width, height >= 1, at most 2^31 - 1 pixels)"),
    ("tsdf_raycast", dict(tsdf=z(1, RY, RX), weight=z(1, RY, RX, dtype=f64)), V,
     "tsdf_raycast: tsdf must be (res_z, res_y, res_x) with every res >= 2, got (1, 4, 5)"),
    ("tsdf_raycast", dict(src=z(H, W + 1, dtype=i32), step=(0.0, 1.0, 1.0)), V, "tsdf_raycast: src must be (12, 16), got (12, 17)"),
    ("tsdf_raycast", dict(step=(0.0, 1.0, INF), near=-1.0), V, "tsdf_raycast: step must be finite (got [0.0, 1.0, inf])"),
    ("tsdf_raycast", dict(step=(0.0, 1.0, 1.0), min_weight=0.0), V, "tsdf_raycast: step must be non-zero (got [0.0, 1.0, 1.0])"),
    ("tsdf_raycast", dict(min_weight=0.0, dt=0.0), V, "tsdf_raycast: min_weight must be positive (got 0.0)"),
    ("tsdf_raycast", dict(dt=0.0, max_steps=-1), V, "tsdf_raycast: dt must be positive and finite (got 0.0)"),
    ("tsdf_raycast", dict(max_steps=-1, depth=zt(H, W)), V, "tsdf_raycast: max_steps must be >= 0 (got -1)"),
    # ------------------------------------------------------------------------------------------------ mesh_count
    ("mesh_count", dict(field=zt(RZ, RY, RX)), V, "mesh_count: field" + CONTIG),
    ("mesh_count", dict(workspace=zt(_mesh_bytes(), dtype=u8)), V, "mesh_count: workspace" + CONTIG),
    ("mesh_count", dict(totals=zt(2, dtype=i64)), V, "mesh_count: totals" + CONTIG),
    ("mesh_count", dict(totals=z(2, dtype=i64, device="cuda:1")), V, "mesh_count: totals is on cuda:1, not on cpu"),
    ("mesh_count", dict(workspace=cpu(_mesh_bytes(), dtype=u8)), RuntimeError, "mesh_count: workspace: expected a GPU tensor" + NO_GPU),
    ("mesh_count", dict(workspace=bytearray(_mesh_bytes())), V, "mesh_count: workspace must be a uint8 tensor of at least %d bytes" % _mesh_bytes()),
    ("mesh_count", dict(totals=[0, 0]), V, "mesh_count: totals must be a (2,) int64 tensor"),
    ("mesh_count", dict(field=z(RY, RX, dtype=f64)), V, "mesh_count: field must be float32, got torch.float64"),
    ("mesh_count", dict(level=INF, totals=z(2, dtype=i64, device="cuda:1")), V, "mesh_count: level must be finite (got inf)"),
    ("mesh_count", dict(field=z(RY, RX), level=INF), V, "mesh_count: field must be (res_z, res_y, res_x) with every res >= 1, got (4, 5)"),
    ("mesh_count", dict(workspace=z(1, dtype=u8), totals=z(3, dtype=i64)), V,
     "mesh_count: workspace must be a uint8 tensor of at least %d bytes" % _mesh_bytes()),
    # ------------------------------------------------------------------------------------------------ mesh_emit
    ("mesh_emit", dict(field=zt(RZ, RY, RX)), V, "mesh_emit: field" + CONTIG),
    ("mesh_emit", dict(workspace=zt(_mesh_bytes(), dtype=u8)), V, "mesh_emit: workspace" + CONTIG),
    ("mesh_emit", dict(vertices=zt(6, 3)), V, "mesh_emit: vertices" + CONTIG),
    ("mesh_emit", dict(faces=zt(2, 3, dtype=i32)), V, "mesh_emit: faces" + CONTIG),
    ("mesh_emit", dict(src=zt(6, dtype=i64)), V, "mesh_emit: src" + CONTIG),
    ("mesh_emit", dict(faces=z(2, 3, dtype=i32, device="cuda:1")), V, "mesh_emit: faces is on cuda:1, not on cpu"),
    ("mesh_emit", dict(vertices=cpu(6, 3)), RuntimeError, "mesh_emit: vertices: expected a GPU tensor" + NO_GPU),
    ("mesh_emit", dict(src=[0] * 6), V, "mesh_emit: src must be a (n,) torch.int64 tensor"),
    ("mesh_emit", dict(vertices=z(6, 2, dtype=f64)), V, "mesh_emit: vertices must be a (n, 3) torch.float32 tensor"),
    ("mesh_emit", dict(lo=(INF, 0.0, 0.0), workspace=z(1, dtype=u8)), V, "mesh_emit: lo must be finite (got [inf, 0.0, 0.0])"),
    ("mesh_emit", dict(src=z(5, dtype=i64, device="cuda:1")), V, "mesh_emit: src holds 5 rows, vertices 6"),
    ("mesh_emit", dict(level=float("nan"), step=(1.0, 1.0)), V, "mesh_emit: level must be finite (got nan)"),
    ("mesh_emit", dict(step=(1.0, 1.0), faces=None), V, "mesh_emit: step: expected 3 values, got 2"),
    ("mesh_emit", dict(workspace=None, vertices=None), V,
     "mesh_emit: workspace must be the uint8 tensor of at least %d bytes that mesh_count filled" % _mesh_bytes()),
    # ------------------------------------------------------------------------------------------------ splat_points
    ("splat_points", dict(points=zt(7, 3)), V, "splat_points: points" + CONTIG),
    ("splat_points", dict(zbuf=zt(H, W, dtype=i64)), V, "splat_points: zbuf" + CONTIG),
    ("splat_points", dict(stats=zt(3, dtype=i64)), V, "splat_points: stats" + CONTIG),
    ("splat_points", dict(stats=z(3, dtype=i64, device="cuda:1")), V, "splat_points: stats is on cuda:1, points on cpu"),
    ("splat_points", dict(zbuf=cpu(H, W, dtype=i64)), RuntimeError, "splat_points: zbuf: expected a GPU tensor" + NO_GPU),
    ("splat_points", dict(zbuf=[0]), V, "splat_points: zbuf must be a (12, 16) int64 tensor"),
    ("splat_points", dict(stats=[0, 0, 0]), V, "splat_points: stats must be (3,)"),
    ("splat_points", dict(points=z(7, 2, dtype=f64)), V, "splat_points: points must be (P, 3)"),
    ("splat_points", dict(radius=3, zbuf=z(H, W, dtype=i64, device="cuda:1")), V, "splat_points: radius must be 0, 1 or 2 (got 3)"),
    ("splat_points", dict(points=None, radius=3), V, "splat_points: points: expected a GPU tensor, got NoneType"),
    ("splat_points", dict(near=2.0, far=1.0, index_base=-1), V, "splat_points: near and far must satisfy 0 <= near <= far (far may be inf)"),
    ("splat_points", dict(index_base=-1, zbuf=z(W, H, dtype=i64)), V,
     "splat_points: index_base + the number of points must stay within 0 .. 2^31 - 1"),
    ("splat_points", dict(zbuf=z(H, W, dtype=i32), points=z(7, 3, dtype=f64)), T, "splat_points: points: expected torch.float32, got torch.float64"),
    ("splat_points", dict(zbuf=z(H, W, dtype=i32), stats=zt(3, dtype=i64)), T, "splat_points: zbuf: expected torch.int64, got torch.int32"),
    ("splat_points", dict(camera=PIN, w2c=torch.eye(3)), V,
     "splat_points: camera: expected a camera.Pinhole or camera.Fisheye (or camera.Equirect), not (50.0, 50.0, 8.0, 6.0)"),
    # ------------------------------------------------------------------------------------------------ splat_resolve
    ("splat_resolve", dict(zbuf=zt(H, W, dtype=i64)), V, "splat_resolve: zbuf" + CONTIG),
    ("splat_resolve", dict(out={"depth": zt(H, W)}), V,
     "splat_resolve: depth: out must be a contiguous torch.float32 tensor of shape (12, 16) on cuda:0"),
    ("splat_resolve", dict(out={"depth": z(H, W, device="cuda:1")}), V,
     "splat_resolve: depth: out must be a contiguous torch.float32 tensor of shape (12, 16) on cuda:0"),
    ("splat_resolve", dict(out={"depth": cpu(H, W)}), V,
     "splat_resolve: depth: out must be a contiguous torch.float32 tensor of shape (12, 16) on cuda:0"),
    ("splat_resolve", dict(want=("index",), out={"index": z(H, W, dtype=i64, device="cuda:0")}), V,
     "splat_resolve: index: out must be a contiguous torch.int32 tensor of shape (12, 16) on cuda:0"),
    ("splat_resolve", dict(zbuf=cpu(H, W, dtype=i64)), RuntimeError, "splat_resolve: zbuf: expected a GPU tensor" + NO_GPU),
    ("splat_resolve", dict(zbuf=[0]), V, "splat_resolve: zbuf: expected a GPU tensor, got list"),
    ("splat_resolve", dict(out={"depth": [0.0]}), AttributeError, "'list' object has no attribute 'shape'"),
    ("splat_resolve", dict(want=("depth", "colour"), out={"bad": None}), V, "splat_resolve: unknown output 'colour' (depth, index)"),
    ("splat_resolve", dict(out={"bad": None}, zbuf=zt(H, W, dtype=i64)), V, "splat_resolve: out holds 'bad' (only 'depth' and 'index')"),
    ("splat_resolve", dict(zbuf=zt(H, W)), T, "splat_resolve: zbuf: expected torch.int64, got torch.float32"),
    # ------------------------------------------------------------------------------------------------ depth_metrics
    ("depth_metrics", dict(pred=zt(H, W)), V, "depth_metrics: pred" + CONTIG),
    ("depth_metrics", dict(gt=zt(H, W)), V, "depth_metrics: gt" + CONTIG),
    ("depth_metrics", dict(mask=zt(H, W, dtype=u8)), V, "depth_metrics: mask (bool or uint8)" + CONTIG),
    ("depth_metrics", dict(mask=zt(H, W, dtype=torch.bool)), T, "depth_metrics: mask (bool or uint8): expected torch.uint8, got torch.bool"),
    ("depth_metrics", dict(sums=zt(5, dtype=f64)), V, "depth_metrics: sums" + CONTIG),
    ("depth_metrics", dict(counts=zt(5, dtype=i64)), V, "depth_metrics: counts" + CONTIG),
    ("depth_metrics", dict(sums=z(5, dtype=f64, device="cuda:1")), V, "depth_metrics: sums is on cuda:1, gt on cpu"),
    ("depth_metrics", dict(pred=z(H, W, device="cuda:1")), V, "depth_metrics: pred is on cuda:1, gt on cpu"),
    ("depth_metrics", dict(pred=cpu(H, W)), RuntimeError, "depth_metrics: pred: expected a GPU tensor" + NO_GPU),
    ("depth_metrics", dict(mask=cpu(H, W, dtype=torch.bool)), RuntimeError, "depth_metrics: mask (bool or uint8): expected a GPU tensor" + NO_GPU),
    ("depth_metrics", dict(sums=[0.0] * 5), V, "depth_metrics: sums must be (5,)"),
    ("depth_metrics", dict(counts=np.zeros(5, np.int64)), V, "depth_metrics: counts must be (5,)"),
    ("depth_metrics", dict(mask=[[1]]), V, "depth_metrics: mask must have gt's shape (12, 16)"),
    ("depth_metrics", dict(pred=z(H, W - 1, dtype=f64)), V, "depth_metrics: pred is (12, 15), gt (12, 16)"),
    ("depth_metrics", dict(d_range=(1.0, INF), counts=z(5, dtype=i64, device="cuda:1")), V,
     "depth_metrics: d_range must satisfy 0 < d_min <= d_max, both finite"),
    ("depth_metrics", dict(d_range=1.0, sums=z(4, dtype=f64)), V, "depth_metrics: d_range must be (d_min, d_max)"),
    ("depth_metrics", dict(gt=None, pred=None), V, "depth_metrics: pred: expected a GPU tensor, got NoneType"),
    ("depth_metrics", dict(sums=z(5), gt=zt(H, W)), V, "depth_metrics: gt" + CONTIG),
    ("depth_metrics", dict(sums=z(5), counts=zt(5, dtype=i64)), T, "depth_metrics: sums: expected torch.float64, got torch.float32"),
    # ------------------------------------------------------------------------------------------------ reproject
    ("reproject", dict(depth_src=zt(H, W)), V, "reproject: depth_src" + CONTIG),
    ("reproject", dict(depth_tgt=zt(H, W)), V, "reproject: depth_tgt" + CONTIG),
    ("reproject", dict(label_src=zt(H, W, dtype=i32)), V, "reproject: label_src" + CONTIG),
    ("reproject", dict(label_tgt=zt(H, W, dtype=i32)), V, "reproject: label_tgt" + CONTIG),
    ("reproject", dict(pix=zt(5, dtype=i32)), V, "reproject: pix" + CONTIG),
    ("reproject", dict(agree=zt(3, 3, dtype=i64)), V, "reproject: agree" + CONTIG),
    ("reproject", dict(stats=zt(5, dtype=i64)), V, "reproject: stats" + CONTIG),
    ("reproject", dict(out={"match": zt(5, dtype=i32)}), V, "reproject: match: out must be a contiguous torch.int32 tensor of shape (5,) on cuda:0"),
    ("reproject", dict(stats=z(5, dtype=i64, device="cuda:1")), V, "reproject: stats is on cuda:1, depth_src on cuda:0"),
    ("reproject", dict(pix=z(5, dtype=i32, device="cuda:1")), V, "reproject: pix is on cuda:1, depth_src on cuda:0"),
    ("reproject", dict(out={"match": z(5, dtype=i32, device="cuda:1")}), V,
     "reproject: match: out must be a contiguous torch.int32 tensor of shape (5,) on cuda:0"),
    ("reproject", dict(depth_tgt=cpu(H, W)), RuntimeError, "reproject: depth_tgt: expected a GPU tensor" + NO_GPU),
    ("reproject", dict(out={"match": cpu(5, dtype=i32)}), V, "reproject: match: out must be a contiguous torch.int32 tensor of shape (5,) on cuda:0"),
    ("reproject", dict(want=("match", "uv"), out={"match": z(5, dtype=i32, device="cuda:0"), "uv": z(5, 3, device="cuda:0")}), V,
     "reproject: uv: out must be a contiguous torch.float32 tensor of shape (5, 2) on cuda:0"),
    ("reproject", dict(agree=[[0]]), AttributeError, "'list' object has no attribute 'is_cuda'"),
    ("reproject", dict(stats=(0,) * 5), AttributeError, "'tuple' object has no attribute 'is_cuda'"),
    ("reproject", dict(out={"match": [0] * 5}), AttributeError, "'list' object has no attribute 'shape'"),
    ("reproject", dict(want=("bogus",), depth_src=None), V, "reproject: unknown output 'bogus' (one of match, uv, agree, stats)"),
    ("reproject", dict(depth_src=z(W, H, dtype=f64, device="cuda:0")), V,
     "reproject: depth_src: expected a (12, 16) image (or its 192 flattened pixels), got (16, 12)"),
    ("reproject", dict(tol=(-1.0, 0.0), stats=z(5, dtype=i64, device="cuda:1")), V, "reproject: tol = (absolute, relative) must be finite and >= 0"),
    ("reproject", dict(label_tgt=None, n_classes=0), V, "reproject: label_src and label_tgt come together"),
    ("reproject", dict(n_classes=0, pix=z(5, 1, dtype=i32)), V, "reproject: n_classes must be in 1 .. 8192 with label images (got 0)"),
    ("reproject", dict(agree=z(2, 2, dtype=i64, device="cuda:0"), out={"bad": None}), V, "reproject: agree must be (n_classes, n_classes) = (3, 3)"),
    ("reproject", dict(stats=z(4, dtype=i64, device="cuda:0"), out={"bad": None}), V, "reproject: stats must be (5,)"),
    ("reproject", dict(out={"bad": None}, pix=z(5, dtype=i32, device="cuda:1")), V,
     "reproject: out holds 'bad' (only 'match' and 'uv' can be caller-owned)"),
    ("reproject", dict(src=PIN, tgt=None), V, "reproject: src: expected a camera.Pinhole or camera.Fisheye (or camera.Equirect), not (50.0, 50.0, 8.0, 6.0)"),
    ("reproject", dict(depth_tgt=z(H, W, dtype=f64, device="cuda:0"), label_src=zt(H, W, dtype=i32)), T,
     "reproject: depth_tgt: expected torch.float32, got torch.float64"),
    # ------------------------------------------------------------------------------------------------ project_points
    ("project_points", dict(points=zt(7, 3)), V, "points" + CONTIG),
    ("project_points", dict(points=cpu(7, 3)), RuntimeError, "points: expected a GPU tensor" + NO_GPU),
    ("project_points", dict(model="ortho", points=z(7, 2)), V, "project_points: model must be 'pinhole', 'fisheye' or 'equirect', not 'ortho'"),
    ("project_points", dict(points=z(7, 2, dtype=f64)), T, "points: expected torch.float32, got torch.float64"),
    ("project_points", dict(cam=(1.0, 2.0), w2c=torch.eye(3)), V, "project_points: model 'pinhole' cam: expected 4 values, got 2"),
    ("project_points", dict(model="fisheye", points=z(7, 2)), V, "project_points: model 'fisheye' cam: expected 7 values, got 4"),
    ("project_points", dict(w2c=torch.eye(3), points=cpu(7, 3)), V, "project_points: w2c: expected 12 values, got 9"),
    ("project_points", dict(points=z(7, 2)), V, "project_points: points must be (P, 3)"),
    # ------------------------------------------------------------------------------------------------ census
    ("census", dict(img=zt(H, W, dtype=u8)), V, "census: img" + CONTIG),
    ("census", dict(out=zt(H, W, dtype=i64)), V, "census: out" + CONTIG),
    ("census", dict(out=z(H, W, dtype=i64, device="cuda:1")), V, "census: out is on cuda:1, not on cpu"),
    ("census", dict(out=cpu(H, W, dtype=i64)), RuntimeError, "census: out: expected a GPU tensor" + NO_GPU),
    ("census", dict(img=cpu(H, W, dtype=u8)), RuntimeError, "census: img: expected a GPU tensor" + NO_GPU),
    ("census", dict(out=[0]), V, "census: out: expected a GPU tensor, got list"),
    ("census", dict(img=z(2, H, W)), T, "census: img: expected torch.uint8, got torch.float32"),
    ("census", dict(out=z(H, W + 1)), T, "census: out: expected torch.int64, got torch.float32"),
    ("census", dict(img=z(0, W, dtype=u8), out=z(H, W, dtype=i64)), V, "census: img: empty tensor"),
    ("census", dict(img=z(2, H, W, dtype=u8), out=[0]), V, "census: img: expected 2 dimensions, got shape (2, 12, 16)"),
    ("census", dict(out=z(H, W + 1, dtype=i64, device="cuda:1")), V, "census: out: expected shape (12, 16), got (12, 17)"),
    # ------------------------------------------------------------------------------------------------ sgm_aggregate
    ("sgm_aggregate", dict(census_l=zt(H, W, dtype=i64)), V, "sgm_aggregate: census_l" + CONTIG),
    ("sgm_aggregate", dict(census_r=zt(H, W, dtype=i64)), V, "sgm_aggregate: census_r" + CONTIG),
    ("sgm_aggregate", dict(out=zt(H, W, 16, dtype=i16)), V, "sgm_aggregate: out" + CONTIG),
    ("sgm_aggregate", dict(census_r=z(H, W, dtype=i64, device="cuda:1")), V, "sgm_aggregate: census_r is on cuda:1, not on cpu"),
    ("sgm_aggregate", dict(census_r=cpu(H, W, dtype=i64)), RuntimeError, "sgm_aggregate: census_r: expected a GPU tensor" + NO_GPU),
    ("sgm_aggregate", dict(out=[0]), V, "sgm_aggregate: out: expected a GPU tensor, got list"),
    ("sgm_aggregate", dict(max_disp=20, census_r=z(H, W, dtype=i64, device="cuda:1")), V,
     "sgm_aggregate: max_disp must be a multiple of 16 in 16 .. 256 (got 20)"),
    ("sgm_aggregate", dict(census_r=z(H, W + 1, dtype=i32)), T, "sgm_aggregate: census_r: expected torch.int64, got torch.int32"),
    ("sgm_aggregate", dict(p1=50, p2=10, out=z(H, W, 32, dtype=i16)), V, "sgm_aggregate: p1 and p2 must satisfy 0 < p1 <= p2 <= 192 (got 50, 10)"),
    ("sgm_aggregate", dict(paths=5, out=z(H, W, 32, dtype=i16)), V, "sgm_aggregate: paths must be 4 or 8 (got 5)"),
    ("sgm_aggregate", dict(census_r=z(H, W + 1, dtype=i64), max_disp=20), V, "sgm_aggregate: census_r: expected shape (12, 16), got (12, 17)"),
    ("sgm_aggregate", dict(out=z(H, W, 32, dtype=i16), census_l=zt(H, W, dtype=i64)), V,
     "sgm_aggregate: out: expected shape (12, 16, 16), got (12, 16, 32)"),
    # ------------------------------------------------------------------------------------------------ sgm_select
    ("sgm_select", dict(S=zt(H, W, 16, dtype=i16)), V, "sgm_select: S" + CONTIG),
    ("sgm_select", dict(out=zt(H, W, dtype=i16)), V, "sgm_select: out" + CONTIG),
    ("sgm_select", dict(disp_right=zt(H, W, dtype=i16)), V, "sgm_select: disp_right" + CONTIG),
    ("sgm_select", dict(disp_right=z(H, W, dtype=i16, device="cuda:1")), V, "sgm_select: disp_right is on cuda:1, not on cpu"),
    ("sgm_select", dict(out=cpu(H, W, dtype=i16)), RuntimeError, "sgm_select: out: expected a GPU tensor" + NO_GPU),
    ("sgm_select", dict(out=[0]), V, "sgm_select: out: expected a GPU tensor, got list"),
    ("sgm_select", dict(disp_right=np.zeros((H, W), np.int16)), V, "sgm_select: disp_right: expected a GPU tensor, got ndarray"),
    ("sgm_select", dict(S=z(H, W, 20, dtype=i16), uniqueness=100), V,
     "sgm_select (the last dimension of S): max_disp must be a multiple of 16 in 16 .. 256 (got 20)"),
    ("sgm_select", dict(lr_tol=-2, out=z(H, W, dtype=i16, device="cuda:1")), V,
     "sgm_select: lr_tol must be >= 0, or -1 for no left-right check (got -2)"),
    ("sgm_select", dict(uniqueness=100, lr_tol=-2), V, "sgm_select: uniqueness must lie in 0 .. 99 (got 100)"),
    ("sgm_select", dict(out=z(H, W + 1)), T, "sgm_select: out: expected torch.int16, got torch.float32"),
    ("sgm_select", dict(out=z(H, W + 1, dtype=i16), disp_right=[0]), V, "sgm_select: out: expected shape (12, 16), got (12, 17)"),
    # ------------------------------------------------------------------------------------------------ disparity_depth
    ("disparity_depth", dict(d16=zt(H, W, dtype=i16)), V, "disparity_depth: d16" + CONTIG),
    ("disparity_depth", dict(out=zt(H, W)), V, "disparity_depth: out" + CONTIG),
    ("disparity_depth", dict(out=z(H, W, device="cuda:1")), V, "disparity_depth: out is on cuda:1, not on cpu"),
    ("disparity_depth", dict(out=cpu(H, W)), RuntimeError, "disparity_depth: out: expected a GPU tensor" + NO_GPU),
    ("disparity_depth", dict(out=[0.0]), V, "disparity_depth: out: expected a GPU tensor, got list"),
    ("disparity_depth", dict(fb=0.0, d_range=(2.0, 1.0)), V, "disparity_depth: fb = fx * baseline must be positive and finite (got 0.0)"),
    ("disparity_depth", dict(d_range=(2.0, 1.0), out=z(H, W, device="cuda:1")), V,
     "disparity_depth: d_range must satisfy 0 < d_min <= d_max (d_max may be inf)"),
    ("disparity_depth", dict(d_range=None, out=[0.0]), V, "disparity_depth: d_range must be (d_min, d_max)"),
    ("disparity_depth", dict(out=z(H, W + 1, dtype=f64)), T, "disparity_depth: out: expected torch.float32, got torch.float64"),
    ("disparity_depth", dict(d16=z(H, W), fb=0.0), T, "disparity_depth: d16: expected torch.int16, got torch.float32"),
]


@pytest.mark.parametrize("op,over,exc,message", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_by_type_and_whole_message(op, over, exc, message):
    args = BASE[op]()
    args.update(over)
    with pytest.raises(Exception) as e:
        getattr(ops, op).__wrapped__(**args)
    assert type(e.value) is exc and str(e.value) == message, "%s: %s" % (type(e.value).__name__, e.value)


def test_every_op_is_covered_and_its_base_arguments_pass_every_check():
    """the base arguments of every op reach the launch, so that each case above fails for the fault it names and no other"""
    assert {c[0] for c in CASES} == set(BASE)
    for op, base in BASE.items():
        with pytest.raises(AssertionError, match="not refused: the op went on to its entry point"):
            getattr(ops, op).__wrapped__(**base())
