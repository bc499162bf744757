"""Depth fusion: posed depth frames -> a truncated signed distance volume (TSDF) -> a labelled, coloured mesh or image, on the GPU
(ops.tsdf_integrate / pnr_tsdf_integrate; the rule is written out in include/pnr.h "depth fusion").  The step between the
depth producers (stereo.depth_from_pair, Renderer.render_view, pointcloud.splat), the frames a `FrameSet` keeps on the device,
and `mesh.extract`: images -> depth -> volume -> mesh.

    vol = fusion.Volume(lo, hi, res, "cuda", color=True, labels=True)
    fusion.integrate(vol, frames, trunc=0.2)                 # every frame of the FrameSet that has a depth image
    m = fusion.extract(vol)                                   # mesh.Mesh with attributes sem_label, inst_label, rgb
    m = fusion.extract(vol, min_faces=500)                    # ... without the connected pieces of fewer than 500 faces
    m.save_ply("scene.ply", colors=m.attributes["rgb"], labels=m.attributes["sem_label"])

The volume lives on the lattice of `Network.query_grid` and `mesh.extract` (cell centres lo + (i + 0.5) step of the box
[lo, hi]).  One launch takes any number of frames: a lattice point's state stays in registers over the whole frame loop, so
the volume is read and written once per call.  Per point the frames are taken in order, so the result is the CPU
restatement's bit for bit and does not depend on how the frames are split over calls.

Conventions (this build's, unpinned): POSITIVE tsdf is BEHIND the observed surface (mesh.extract calls field > level inside);
nearest-pixel depth lookup; depth as render_view writes it (z-depth in a pinhole frame, range in a fisheye / equirect frame);
every observation weighs 1; colour is the running mean of the frames' bytes; the label is a Boyer-Moore majority vote over
(pseudo_label, instance_label) pairs.  Out of scope: per-pixel confidence weights, voxel hashing or sparse volumes, frustum
culling per block, reading pose files.

The way back from the volume to an image is `raycast` (ops.tsdf_raycast / pnr_tsdf_raycast; include/pnr.h "volume ray casting"):

    maps = fusion.raycast(vol, camera, c2w, near, far)       # depth, normal, code, src, valid, sem_label, inst_label, rgb
    consistency.reproject((camera, c2w, maps), other_view)    # (camera, c2w, maps) is a view like render_view's

Out of scope there: steps that adapt to the tsdf value, block-level empty-space skipping, trilinear colour, shading, sub-lists
of pixels.

The ray-cast is also the model a new frame is aligned to: `track` (ops.icp_accumulate / ops.icp_solve; include/pnr.h "pose
tracking") refines a pose guess by point-to-plane ICP on the device, and FrameSet.set_pose writes it back, which closes the loop:

    view = (camera, c2w_prev, fusion.raycast(vol, camera, c2w_prev, near, far))
    c2w, info = fusion.track(view, camera, depth, c2w_prev)   # device (3, 4); info["history"]: count, E, |w|^2, |v|^2, status per iteration
    frames.set_pose(i, c2w.cpu()); fusion.integrate(vol, frames, trunc, first=i, last=i + 1)

Out of scope there: image pyramids, robust weights, a normal-angle gate, colour terms, stopping early.

Before a volume exists, a depth frame is its own model: depth.view gives any depth image the normals `track` needs, and `odometry`
chains frame-to-frame tracks into poses good enough to integrate the first frames:

    poses, info = fusion.odometry(camera, depths, filter=dict(radius=3, min_support=4))     # device (F, 3, 4); nothing read back
    for i, p in enumerate(poses.cpu()): frames.set_pose(i, p)"""
import numpy as np
import torch

from . import depth as _depth
from . import mesh as _mesh
from . import ops
from .camera import is_camera

LABEL_NONE = -1


def pack_label(sem, inst):
    """the key the vote stores: (sem << 16) | (uint16) inst for sem >= 0, -1 otherwise; integer tensors (any device)"""
    sem, inst = torch.as_tensor(sem).to(torch.int32), torch.as_tensor(inst).to(torch.int32)
    return torch.where(sem >= 0, (sem << 16) | (inst & 0xFFFF), torch.full_like(sem, LABEL_NONE))


def unpack_label(label):
    """(sem, inst) int32 of packed keys: sem = key >> 16, inst = the low half as an int16; both -1 where key < 0 (nothing voted)"""
    label = torch.as_tensor(label).to(torch.int32)
    none = label < 0
    inst = ((label & 0xFFFF) ^ 0x8000) - 0x8000
    return torch.where(none, torch.full_like(label, -1), label >> 16), torch.where(none, torch.full_like(label, -1), inst)


class Volume:
    """A TSDF volume over the box [lo, hi] at res = (res_x, res_y, res_z) cells (an int: the same on every axis).  The arrays
    are plain tensors on `device`; integrate and extract need them on the GPU (the HIP path has no CPU fallback).
    Arrays, (res_z, res_y, res_x) each: tsdf, weight float32; with color=True rgb (..., 3) and rgb_weight float32 (the mean of
    the colour bytes, 0 .. 255); with labels=True label and conf int32.  lo32 / step are mesh.lattice's, so the box means the
    same bits as in query_grid and mesh.extract."""

    def __init__(self, lo, hi, res, device, color=False, labels=False):
        try:
            res3 = (int(res),) * 3 if np.ndim(res) == 0 else tuple(int(r) for r in res)
        except (TypeError, ValueError):
            raise ValueError("fusion.Volume: res must be an int or three ints (res_x, res_y, res_z)") from None
        if len(res3) != 3 or min(res3) < 1:
            raise ValueError("fusion.Volume: res must be an int or three ints >= 1 (res_x, res_y, res_z), got %r" % (res,))
        if res3[0] * res3[1] * res3[2] > ops.TSDF_MAX_POINTS:
            raise ValueError("fusion.Volume: %d x %d x %d points, more than the limit of 2^31 - 1" % res3)
        self.lo32, self.step = _mesh.lattice(lo, hi, res3)
        if not (self.step != 0).all():
            raise ValueError("fusion.Volume: the box is empty along an axis (lo %r, hi %r)" % (self.lo32.tolist(), hi))
        dev = torch.device(device)
        self.lo, self.hi, self.res = lo, hi, res3
        rx, ry, rz = res3
        f32 = lambda *tail: torch.empty((rz, ry, rx) + tail, dtype=torch.float32, device=dev)
        i32 = lambda: torch.empty((rz, ry, rx), dtype=torch.int32, device=dev)
        self.tsdf, self.weight = f32(), f32()
        self.rgb, self.rgb_weight = (f32(3), f32()) if color else (None, None)
        self.label, self.conf = (i32(), i32()) if labels else (None, None)
        self.device = self.tsdf.device
        self.reset()

    def __repr__(self):
        return "Volume(%d x %d x %d%s%s)" % (self.res + (", color" if self.rgb is not None else "", ", labels" if self.label is not None else ""))

    def reset(self):
        """the initial values, in place: everything 0, label -1"""
        for t in (self.tsdf, self.weight, self.rgb, self.rgb_weight, self.conf):
            if t is not None:
                t.zero_()
        if self.label is not None:
            self.label.fill_(LABEL_NONE)

    def _labels(self):
        if self.label is None:
            raise ValueError("fusion.Volume: the volume was made without labels (labels=True)")
        return unpack_label(self.label)

    @property
    def sem_label(self):
        """(res_z, res_y, res_x) int32: the semantic half of the majority key, -1 where nothing voted"""
        return self._labels()[0]

    @property
    def inst_label(self):
        """(res_z, res_y, res_x) int32: the instance half of the majority key, -1 where nothing voted (or the frames had none)"""
        return self._labels()[1]

    def colors(self):
        """(res_z, res_y, res_x, 3) uint8: the mean colour rounded to the nearest byte (0 where no frame coloured the point)"""
        if self.rgb is None:
            raise ValueError("fusion.Volume: the volume was made without colour (color=True)")
        return self.rgb.round().clamp(0, 255).to(torch.uint8)


def integrate(volume, frames, trunc, first=0, last=None, max_depth=float("inf"), w_max=float("inf")):
    """Fuse frames first .. last - 1 (last=None: all) of the FrameSet `frames` into `volume`, in ONE launch.  A frame without a
    depth image is skipped; colour comes from the frames' rgb, labels from pseudo_label / instance_label.  trunc: the band's
    half width in world units -- see `extract` for how small it may be; max_depth: depth pixels beyond it are ignored; w_max:
    the cap of the running weights (1 = the last frame wins, inf = a plain mean).  The world-to-camera rows come from
    FrameSet.w2c_table (camera.invert_pose of every c2w, kept on the device).  Nothing is synchronised; with an unchanged set
    the call is one kernel launch and can be captured in a graph."""
    if not isinstance(volume, Volume):
        raise TypeError("fusion.integrate: volume must be a fusion.Volume")
    if not all(hasattr(frames, k) for k in ("table", "frames", "w2c_table")):
        raise TypeError("fusion.integrate: frames must be a FrameSet")
    n = len(frames)
    first, last = int(first), n if last is None else int(last)
    if not 0 <= first <= last <= n:
        raise ValueError("fusion.integrate: need 0 <= first <= last <= %d (the frames of the set), got [%d, %d)" % (n, first, last))
    trunc, max_depth, w_max = ops.integrate_params("fusion.integrate", trunc, max_depth, w_max)
    if not volume.tsdf.is_cuda:
        raise RuntimeError("fusion.integrate: the volume is not on the GPU (the HIP path has no CPU fallback)")
    if first == last:
        return volume
    ops.tsdf_integrate(frames.table, frames.w2c_table(), first, last, volume.lo32, volume.step, trunc, volume.tsdf, volume.weight,
                       rgb=volume.rgb, rgb_weight=volume.rgb_weight, label=volume.label, conf=volume.conf, max_depth=max_depth,
                       w_max=w_max)
    return volume


def unobserved_near(observed):
    """(res_z, res_y, res_x) bool: the points with an unobserved lattice point within +-1 per axis (themselves included); points
    beyond the lattice do not count.  Torch slicing on any device: a 3 x 3 x 3 dilation of ~observed, one axis at a time."""
    bad = ~observed
    for axis in range(3):
        n = bad.shape[axis]
        grown = bad.clone()
        if n > 1:
            grown.narrow(axis, 0, n - 1).logical_or_(bad.narrow(axis, 1, n - 1))
            grown.narrow(axis, 1, n - 1).logical_or_(bad.narrow(axis, 0, n - 1))
        bad = grown
    return bad


def filter_mesh(vertices, faces, src, observed):
    """The part of a mesh that lies in observed space: a vertex is kept iff every lattice point within +-1 per axis of
    src[v] is observed, a face iff all three of its vertices are kept, and vertices of no kept face are dropped; what remains
    keeps its order.  Returns (vertices, faces int32, src, index) with index = the old number of every remaining vertex.
    Torch indexing on any device."""
    keep_v = ~unobserved_near(observed).reshape(-1)[src]
    f = faces.long()
    keep_f = keep_v[f].all(dim=1) if f.shape[0] else torch.zeros((0,), dtype=torch.bool, device=faces.device)
    f = f[keep_f]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[f.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    index = torch.nonzero(used).reshape(-1)
    return vertices[index], new[f].to(torch.int32), src[index], index


def extract(volume, min_weight=1.0, min_faces=0):
    """The mesh of the fused surface (mesh.Mesh), restricted to observed space.  field = where(weight >= min_weight, tsdf, -1)
    goes through mesh.extract at level 0; then `filter_mesh` removes the shell between observed and never-observed space --
    the back face at depth + trunc included.  attributes: sem_label, inst_label (volumes with labels) and rgb uint8 (volumes
    with colour) per vertex, read at src, so save_ply(colors=m.attributes["rgb"], labels=m.attributes["sem_label"]) works
    directly.  Torch plumbing on the device around mesh.extract; no kernel of its own.  min_faces > 0: the connected pieces of
    fewer faces are removed last (Mesh.remove_small); 0 returns every piece.

    A `trunc` below 4 x the largest lattice step ERODES REAL SURFACE: a vertex needs all 27 points round its inside point
    observed, a neighbour of the first inside point can lie up to about 3.5 steps behind the surface (the inside end of a
    cube-diagonal edge up to sqrt(3) steps, its diagonal neighbour sqrt(3) more), and points deeper than trunc are never
    observed."""
    if not isinstance(volume, Volume):
        raise TypeError("fusion.extract: volume must be a fusion.Volume")
    min_faces = _mesh._min_faces("fusion.extract", min_faces)
    min_weight = float(min_weight)
    if not (min_weight > 0.0):
        raise ValueError("fusion.extract: min_weight must be positive (got %r)" % min_weight)
    if not volume.tsdf.is_cuda:
        raise RuntimeError("fusion.extract: the volume is not on the GPU (the HIP path has no CPU fallback)")
    observed = volume.weight >= min_weight
    field = torch.where(observed, volume.tsdf, torch.full_like(volume.tsdf, -1.0))
    m = _mesh.extract(field, volume.lo, volume.hi, 0.0)
    m.vertices, m.faces, m.src, _ = filter_mesh(m.vertices, m.faces, m.src, observed)
    if volume.label is not None:
        sem, inst = unpack_label(volume.label)
        m.attributes["sem_label"], m.attributes["inst_label"] = m.labels(sem), m.labels(inst)
    if volume.rgb is not None:
        m.attributes["rgb"] = volume.colors().reshape(-1, 3)[m.src]
    return m.remove_small(min_faces) if min_faces else m


HIT, NO_RAY, MISSED, NO_SURFACE = ops.RAYCAST_HIT, ops.RAYCAST_NO_RAY, ops.RAYCAST_MISSED, ops.RAYCAST_NO_SURFACE


def raycast(volume, camera, c2w, near, far, step=None, min_weight=1.0, max_steps=None, normals=True, attributes=True):
    """Render `volume` into (camera, c2w): the way back from a fused volume to an image, in ONE launch (ops.tsdf_raycast; the rule
    is in include/pnr.h "volume ray casting").  camera: camera.Pinhole / Fisheye / Equirect; c2w: 3x4 camera-to-world.  A ray is
    marched through the lattice in steps of `step` (units of the ray parameter; None: half the volume's smallest lattice step)
    for at most max_steps samples (None: enough for the lattice's diagonal); the first crossing from in front of the surface to
    behind it, between two samples whose eight lattice points all have weight >= min_weight, is the hit.  Returns a maps dict
    of (height, width, ...) images on the volume's device, which (camera, c2w, maps) makes a view for consistency.reproject,
    pointcloud.lift and Evaluator.evaluate_depth:
        depth   float32   in render_view's convention (z-depth in a pinhole, range in a fisheye / equirect); 0 off the surface
        code    uint8     HIT, NO_RAY, MISSED or NO_SURFACE;  valid  bool = code == HIT
        src     int32     the flat index of the lattice point nearest the hit, -1 off the surface
        normal  float32 (., 3)  with normals: the world-space unit normal towards free space, 0 off the surface
        sem_label, inst_label int32 (-1 off the surface; volumes with labels) and rgb uint8 (0 off the surface; volumes with
        colour), with attributes: gathered at src with torch indexing.
    Nothing is synchronised; the launch can be captured in a graph, and a replay sees what was integrated since."""
    if not isinstance(volume, Volume):
        raise TypeError("fusion.raycast: volume must be a fusion.Volume")
    if not is_camera(camera):
        raise TypeError("fusion.raycast: camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect, not %r" % (camera,))
    if min(volume.res) < 2:
        raise ValueError("fusion.raycast: the volume is %d x %d x %d; ray casting needs every res >= 2" % volume.res)
    near, far, min_weight, dt, max_steps = ops.raycast_params("fusion.raycast", near, far, min_weight, step, max_steps, volume.res,
                                                              volume.step, dt_name="step")
    if not volume.tsdf.is_cuda:
        raise RuntimeError("fusion.raycast: the volume is not on the GPU (the HIP path has no CPU fallback)")
    dev, h, w = volume.device, int(camera.height), int(camera.width)
    maps = {"depth": torch.empty((h, w), dtype=torch.float32, device=dev), "code": torch.empty((h, w), dtype=torch.uint8, device=dev),
            "src": torch.empty((h, w), dtype=torch.int32, device=dev)}
    if normals:
        maps["normal"] = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    ops.tsdf_raycast(camera.model, camera.params, c2w, w, h, near, far, volume.lo32, volume.step, volume.tsdf, volume.weight,
                     maps["depth"], maps["code"], normal=maps.get("normal"), src=maps["src"], min_weight=min_weight, dt=dt,
                     max_steps=max_steps)
    maps["valid"] = maps["code"] == HIT
    if attributes:
        at = maps["src"].clamp(min=0).long()
        if volume.label is not None:
            for name, lab in zip(("sem_label", "inst_label"), unpack_label(volume.label)):
                maps[name] = torch.where(maps["valid"], lab.reshape(-1)[at], torch.full_like(maps["src"], -1))
        if volume.rgb is not None:
            maps["rgb"] = torch.where(maps["valid"][..., None], volume.colors().reshape(-1, 3)[at], torch.zeros((), dtype=torch.uint8, device=dev))
    return maps


MATCH, NO_DEPTH, OUTSIDE, NO_MODEL, TOO_FAR, BACK_FACING = (ops.ICP_MATCH, ops.ICP_NO_DEPTH, ops.ICP_OUTSIDE, ops.ICP_NO_MODEL,
                                                            ops.ICP_TOO_FAR, ops.ICP_BACK_FACING)
ICP_OK, ICP_TOO_FEW, ICP_DEGENERATE, ICP_STEP_TOO_LARGE = ops.ICP_OK, ops.ICP_TOO_FEW, ops.ICP_DEGENERATE, ops.ICP_STEP_TOO_LARGE


def track(model_view, camera, depth, c2w, iters=10, dist_max=0.25, min_matches=64, max_rot=0.25, max_trans=0.5, maps=True):
    """Refine the pose of a live depth frame against a model view by point-to-plane ICP with projective association (the rule is
    in include/pnr.h "pose tracking"): frame-to-model alignment, the step that closes raycast -> track -> set_pose -> integrate.
    model_view: (camera_M, c2w_M, maps) with maps["depth"] and the world-space maps["normal"], as `raycast` returns them (c2w_M: host
    values); camera, depth: the live frame, depth a (height, width) float32 GPU image in render_view's convention; c2w: the guess,
    3x4 (or 4x4) host values or a device tensor (a host guess is uploaded by a stream-ordered copy: inside a graph capture pass a
    device tensor).  Cameras of any model on either side.  Each of the `iters` iterations is one ops.icp_accumulate and one
    ops.icp_solve on a pose that stays in device memory; a last accumulate at the final pose fills history row `iters` and, with
    maps, the images.  dist_max: matches farther apart (world units) are dropped; an iteration with fewer than min_matches, a
    degenerate system, or a step beyond max_rot (radians, at most 0.5) / max_trans leaves the pose as it was.
    Returns (c2w, info): c2w a device (3, 4) float32; info["history"] a device (iters + 1, 5) float64 of count, E = sum r^2,
    |omega|^2, |v|^2, status (ICP_OK, ICP_TOO_FEW, ICP_DEGENERATE, ICP_STEP_TOO_LARGE) per iteration; with maps info["code"] uint8
    (MATCH, NO_DEPTH, OUTSIDE, NO_MODEL, TOO_FAR, BACK_FACING), info["residual"] float32 and info["valid"] = code == MATCH.
    Nothing is synchronised and nothing is read back: the 2 iters + 2 launches can be captured in a graph, and a replay sees the
    depth image's and the model maps' current contents."""
    try:
        cam_m, c2w_m, mmaps = model_view
    except (TypeError, ValueError):
        raise TypeError("fusion.track: model_view must be (camera, c2w, maps), a view as fusion.raycast makes it") from None
    if not is_camera(cam_m):
        raise TypeError("fusion.track: the model view's camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect, not %r" % (cam_m,))
    if not is_camera(camera):
        raise TypeError("fusion.track: camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect, not %r" % (camera,))
    if not hasattr(mmaps, "keys") or "depth" not in mmaps:
        raise ValueError("fusion.track: the model view's maps need 'depth'")
    if mmaps.get("normal") is None:
        raise ValueError("fusion.track: the model view's maps need 'normal' (fusion.raycast with normals=True)")
    c2w_m = torch.as_tensor(c2w_m, dtype=torch.float32).reshape(-1)
    if c2w_m.numel() not in (12, 16):
        raise ValueError("fusion.track: the model view's c2w must be a 3x4 (or 4x4) matrix")
    c2w_m = c2w_m[:12]
    iters = int(iters)
    if iters < 0:
        raise ValueError("fusion.track: iters must be >= 0 (got %d)" % iters)
    # the scalars the two ops would refuse, refused here: before anything is allocated or launched
    dist_max = ops.icp_accumulate_params("fusion.track", dist_max)
    min_matches, max_rot, max_trans = ops.icp_solve_params("fusion.track", min_matches, max_rot, max_trans)
    if not isinstance(depth, torch.Tensor):
        raise TypeError("fusion.track: depth must be a GPU tensor, got %s" % type(depth).__name__)
    if not depth.is_cuda:
        raise RuntimeError("fusion.track: depth is not on the GPU (the HIP path has no CPU fallback)")
    dev, h, w = depth.device, int(camera.height), int(camera.width)
    hm, wm = int(cam_m.height), int(cam_m.width)
    for name, t, shape in (("depth", depth, (h, w)), ("the model view's depth", mmaps["depth"], (hm, wm)),
                           ("the model view's normal", mmaps["normal"], (hm, wm, 3))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError("fusion.track: %s must be a float32 tensor of shape %s, got %s"
                             % (name, shape, "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        if not t.is_contiguous():
            raise ValueError("fusion.track: %s must be contiguous" % name)
        if t.device != dev:
            raise ValueError("fusion.track: %s is on %s, depth on %s" % (name, t.device, dev))
    if isinstance(c2w, torch.Tensor) and c2w.is_cuda:
        if c2w.numel() not in (12, 16):
            raise ValueError("fusion.track: c2w must be a 3x4 (or 4x4) matrix")
        pose = c2w.to(dev, torch.float32).reshape(-1)[:12].clone()
    else:
        host = torch.as_tensor(c2w, dtype=torch.float32).reshape(-1)
        if host.numel() not in (12, 16):
            raise ValueError("fusion.track: c2w must be a 3x4 (or 4x4) matrix")
        pose = host[:12].to(dev)
    ws = ops.icp_workspace(w * h, dev)
    history = torch.zeros((iters + 1, 5), dtype=torch.float64, device=dev)
    live = (camera.model, camera.params, w, h, depth, pose)
    model = (cam_m.model, cam_m.params, c2w_m, int(cam_m.width), int(cam_m.height), mmaps["depth"], mmaps["normal"])
    solve = dict(min_matches=min_matches, max_rot=max_rot, max_trans=max_trans)
    for k in range(iters):
        ops.icp_accumulate(*live, *model, dist_max, ws)
        ops.icp_solve(ws, w * h, pose, history[k], **solve)
    info = {"history": history}
    if maps:
        info["code"] = torch.empty((h, w), dtype=torch.uint8, device=dev)
        info["residual"] = torch.empty((h, w), dtype=torch.float32, device=dev)
    ops.icp_accumulate(*live, *model, dist_max, ws, code=info.get("code"), residual=info.get("residual"))
    ops.icp_solve(ws, w * h, pose, history[iters], update=False, **solve)
    if maps:
        info["valid"] = info["code"] == MATCH
    return pose.reshape(3, 4), info


def _compose(a, b):
    """a o b of two (3, 4) float64 device poses by elementwise arithmetic (the package calls no BLAS):
    R_ic = (a_i0 b_0c + a_i1 b_1c) + a_i2 b_2c, and the translation column with a's own added last"""
    out = (a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :]) + a[:, 2:3] * b[2:3, :]
    return torch.cat([out[:, :3], out[:, 3:] + a[:, 3:]], dim=1)


def odometry(camera, depths, c2w0=None, filter=None, guess="identity", **track_args):
    """Poses for a sequence of depth images of one camera, with no volume: frame k is tracked against the view of frame k - 1
    (depth.view of it in its OWN camera frame, pose identity -- so no host value depends on a device result), which gives the pose
    of camera k in camera k - 1; the absolute poses are composed on the device, in float64, by elementwise arithmetic.
    depths: a sequence of F >= 1 (height, width) float32 GPU images (or one (F, height, width) tensor); c2w0: the pose of frame 0,
    3x4 (or 4x4) host values or a device tensor (None: identity; inside a graph capture pass None or a device tensor); filter: None
    or depth.filter's arguments as a dict, applied to every frame -- the filtered image is both the live frame and the next model;
    guess: "identity" (every step starts from no motion) or "velocity" (from the previous step's relative pose); track_args:
    iters, dist_max, min_matches, max_rot, max_trans of `track`.
    Returns (poses, info): poses a device (F, 3, 4) float32; info["relative"] (F - 1, 3, 4) float32, row k - 1 the pose of camera k
    in camera k - 1, and info["history"] (F - 1, iters + 1, 5) float64, `track`'s history of every step.  A failed step keeps its
    guess: its status is not ICP_OK, its relative pose is the guess, and both are there to see in info.  Nothing is synchronised
    and nothing is read back: the whole call can be captured in a graph."""
    what = "fusion.odometry"
    if not is_camera(camera):
        raise TypeError("%s: camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect, not %r" % (what, camera))
    if guess not in ("identity", "velocity"):
        raise ValueError("%s: guess must be 'identity' or 'velocity', not %r" % (what, guess))
    ops._names(what, track_args, ("iters", "dist_max", "min_matches", "max_rot", "max_trans"),
               "unknown argument %(key)s (the arguments of fusion.track it passes on: %(known)s)")
    if isinstance(depths, torch.Tensor):
        if depths.dim() != 3:
            raise ValueError("%s: depths must be a sequence of (height, width) images or one (F, height, width) tensor, got %s" % (what, tuple(depths.shape)))
        depths = list(depths.unbind(0))
    try:
        depths = list(depths)
    except TypeError:
        raise TypeError("%s: depths must be a sequence of (height, width) images or one (F, height, width) tensor" % what) from None
    if not depths:
        raise ValueError("%s: depths is empty (at least one frame)" % what)
    _depth._filter_args(what, filter)
    iters = int(track_args.get("iters", 10))
    if iters < 0:
        raise ValueError("%s: iters must be >= 0 (got %d)" % (what, iters))
    ops.icp_accumulate_params(what, track_args.get("dist_max", 0.25))
    ops.icp_solve_params(what, track_args.get("min_matches", 64), track_args.get("max_rot", 0.25), track_args.get("max_trans", 0.5))
    for k, d in enumerate(depths):
        _depth._image("%s: frame %d" % (what, k), d, camera)
        if d.device != depths[0].device:
            raise ValueError("%s: frame %d is on %s, frame 0 on %s" % (what, k, d.device, depths[0].device))
    dev = depths[0].device
    if c2w0 is None:
        first = torch.eye(3, 4, dtype=torch.float64, device=dev)
    else:
        c2w0 = c2w0 if isinstance(c2w0, torch.Tensor) else torch.as_tensor(c2w0, dtype=torch.float32)
        if c2w0.numel() not in (12, 16):
            raise ValueError("%s: c2w0 must be a 3x4 (or 4x4) matrix" % what)
        first = c2w0.reshape(-1)[:12].reshape(3, 4).to(dev, torch.float64)
    eye = torch.eye(4)[:3]
    views = [_depth.view(camera, eye, d, filter=filter) for d in depths]
    ident = torch.eye(3, 4, dtype=torch.float32, device=dev)
    absolute, relative, history = [first], [], []
    start = ident
    for k in range(1, len(views)):
        rel, info = track(views[k - 1], camera, views[k][2]["depth"], start, maps=False, **track_args)
        relative.append(rel)
        history.append(info["history"])
        absolute.append(_compose(absolute[-1], rel.to(torch.float64)))
        if guess == "velocity":
            start = rel
    poses = torch.stack(absolute).to(torch.float32)
    info = {"relative": torch.stack(relative) if relative else torch.zeros((0, 3, 4), dtype=torch.float32, device=dev),
            "history": torch.stack(history) if history else torch.zeros((0, iters + 1, 5), dtype=torch.float64, device=dev)}
    return poses, info
