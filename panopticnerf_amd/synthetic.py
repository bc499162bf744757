"""Synthetic KITTI-360-shaped inputs: there is no dataset in this
environment, so rays come from a pinhole camera with KITTI-360-like rectified intrinsics and
the 3D bbox prior from seeded random oriented boxes.  CPU tensors; callers move them."""
import math

import torch

KITTI_W, KITTI_H = 1408, 376
KITTI_F, KITTI_CX, KITTI_CY = 552.554261, 682.049453, 238.769549

# KITTI-360-shaped fisheye (the side-facing 1400 x 1400 cameras; MEI model, include/pnr.h "cameras"): shaped, not a calibration file
FISHEYE_W, FISHEYE_H = 1400, 1400
FISHEYE_XI, FISHEYE_K1, FISHEYE_K2 = 2.2134, 0.016798, 1.6548
FISHEYE_GAMMA1, FISHEYE_GAMMA2, FISHEYE_U0, FISHEYE_V0 = 1336.3, 1335.8, 716.94, 705.76


# BASELINE.json `configs` as renderer / network config keys (SURVEY.md 8d "config mapping").  `bbox`: whether the 3D
# bbox prior is part of the workload.  C = 45 / K = 32 are this build's choices (the reference's are unverifiable,
# SURVEY.md 9 item 8); every consumer prints what it used.
BASELINE_CONFIGS = {
    1: dict(name="configs[0]: coarse-only 32 samples/ray, 4x128 MLP, appearance only",
            N_samples=32, N_importance=0, D=4, W=128, skips=[4], num_classes=0, num_instances=0, bbox=False),
    2: dict(name="configs[1]: coarse-only 64 samples/ray, 8x256 MLP, appearance only",
            N_samples=64, N_importance=0, D=8, W=256, skips=[4], num_classes=0, num_instances=0, bbox=False),
    3: dict(name="configs[2]: coarse+fine 64+128 (sample_pdf), 8x256 MLPs, appearance + depth",
            N_samples=64, N_importance=128, D=8, W=256, skips=[4], num_classes=0, num_instances=0, bbox=False),
    4: dict(name="configs[3]: + semantic head 45 (3D bbox prior + learned), panoptic logit compositing",
            N_samples=64, N_importance=128, D=8, W=256, skips=[4], num_classes=45, num_instances=0, bbox=True),
    5: dict(name="configs[4]: full panoptic (semantic 45 + instance 32 heads, 3D bbox prior)",
            N_samples=64, N_importance=128, D=8, W=256, skips=[4], num_classes=45, num_instances=32, bbox=True),
}


def baseline_cfg(n, **extra):
    """BASELINE config n (1..5) as an attribute-style cfg for make_network / make_renderer (+ overrides)."""
    from types import SimpleNamespace
    d = {k: v for k, v in BASELINE_CONFIGS[n].items() if k not in ("name", "bbox")}
    d.update(extra)
    return SimpleNamespace(**d)


def camera_rays(width=KITTI_W, height=KITTI_H, yaw=0.0, origin=(0.0, 1.55, 0.0), near=0.5, far=100.0):
    """(H*W, 8) rays: o(3), d(3) (unnormalised pixel directions, z forward), near, far."""
    j, i = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32),
                          indexing="ij")
    d = torch.stack([(i - KITTI_CX) / KITTI_F, (j - KITTI_CY) / KITTI_F, torch.ones_like(i)], -1).reshape(-1, 3)
    c, s = math.cos(yaw), math.sin(yaw)
    Rm = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    d = d @ Rm.T
    o = torch.tensor(origin, dtype=torch.float32).expand_as(d)
    nf = torch.tensor([near, far], dtype=torch.float32).expand(d.shape[0], 2)
    return torch.cat([o, d, nf], -1).contiguous()


def fisheye_camera(scale=1.0, yaw=math.pi / 2, origin=(0.0, 1.55, 0.0), mask=None):
    """(camera.Fisheye, c2w (3,4)) for tests and examples: the KITTI-360-shaped parameter set above and a sideways pose (the
    optical axis turned by `yaw` about y from camera_rays' forward axis).  scale < 1 shrinks the image with its intrinsics
    (pixel centres kept: u0 -> (u0 + 0.5) scale - 0.5), e.g. scale = 96 / 1400 for a 96 x 96 test frame."""
    from .camera import Fisheye
    w, h = int(round(FISHEYE_W * scale)), int(round(FISHEYE_H * scale))
    cam = Fisheye(FISHEYE_XI, FISHEYE_K1, FISHEYE_K2, FISHEYE_GAMMA1 * scale, FISHEYE_GAMMA2 * scale,
                  (FISHEYE_U0 + 0.5) * scale - 0.5, (FISHEYE_V0 + 0.5) * scale - 0.5, w, h, mask=mask)
    c, s = math.cos(yaw), math.sin(yaw)
    c2w = torch.tensor([[c, 0.0, s, origin[0]], [0.0, 1.0, 0.0, origin[1]], [-s, 0.0, c, origin[2]]], dtype=torch.float32)
    return cam, c2w


def equirect_camera(scale=1.0, yaw=0.0, origin=(0.0, 1.55, 0.0)):
    """(camera.Equirect, c2w (3,4)) for tests and examples: a full-sphere panorama at camera_rays' origin, 1408 x 704 at
    scale = 1 (the width of the perspective frames; 2 : 1 so that a pixel spans the same angle both ways), longitude 0 turned
    by `yaw` about y from camera_rays' forward axis."""
    from .camera import Equirect
    w = max(int(round(KITTI_W * scale)), 2)
    cam = Equirect(w, max(w // 2, 1))
    c, s = math.cos(yaw), math.sin(yaw)
    c2w = torch.tensor([[c, 0.0, s, origin[0]], [0.0, 1.0, 0.0, origin[1]], [-s, 0.0, c, origin[2]]], dtype=torch.float32)
    return cam, c2w


def lidar_scan(origin=(0.0, 1.55, 0.0), sphere=((0.0, 1.55, 10.0), 30.0), ground_y=None, n_azimuth=360, n_elevation=32,
               elevation=(-25.0, 15.0), azimuth=(-180.0, 180.0)):
    """A spinning-LiDAR-shaped cloud with known depth, for tests and examples: n_elevation rings of n_azimuth beams from
    `origin` -- 3 world coordinates, or a 3x4 / 4x4 sensor-to-world pose whose axes the beam angles then refer to -- hit an
    analytic scene: the inside of `sphere` = (centre, radius), which must enclose the origin, and optionally the plane
    y = ground_y (y points down, as in camera_rays).  Angles in degrees: azimuth 0 along +z, positive towards +x; elevation
    positive up.  Float64 closed forms, rounded once.  Returns points (n, 3) float32 in world space and range (n) float32."""
    o = torch.as_tensor(origin, dtype=torch.float64).reshape(-1)
    if o.numel() == 16:
        o = o[:12]
    if o.numel() == 12:
        Rm, o = o.reshape(3, 4)[:, :3], o.reshape(3, 4)[:, 3]
    elif o.numel() == 3:
        Rm = torch.eye(3, dtype=torch.float64)
    else:
        raise ValueError("lidar_scan: origin must be 3 coordinates or a 3x4 (4x4) pose")
    centre, radius = torch.as_tensor(sphere[0], dtype=torch.float64).reshape(3), float(sphere[1])
    oc = o - centre
    if not float(oc @ oc) < radius * radius:
        raise ValueError("lidar_scan: the origin must lie inside the sphere")
    if n_azimuth < 1 or n_elevation < 1:
        raise ValueError("lidar_scan: n_azimuth and n_elevation must be >= 1")
    az = torch.deg2rad(azimuth[0] + (azimuth[1] - azimuth[0]) * (torch.arange(n_azimuth, dtype=torch.float64) + 0.5) / n_azimuth)
    el = torch.deg2rad(elevation[0] + (elevation[1] - elevation[0]) * (torch.arange(n_elevation, dtype=torch.float64) + 0.5) / n_elevation)
    el, az = torch.meshgrid(el, az, indexing="ij")
    d = torch.stack([torch.cos(el) * torch.sin(az), -torch.sin(el), torch.cos(el) * torch.cos(az)], -1).reshape(-1, 3) @ Rm.T
    b = d @ oc
    t = -b + torch.sqrt(b * b - (oc @ oc - radius * radius))           # unit d: the far root, the origin is inside
    if ground_y is not None:
        tg = (float(ground_y) - o[1]) / d[:, 1]
        t = torch.where((d[:, 1] != 0) & (tg > 0) & (tg < t), tg, t)
    return (o + t[:, None] * d).float().contiguous(), t.float().contiguous()


def random_boxes(n_box=64, n_sem=45, n_inst=32, seed=1):
    """Seeded oriented boxes: (M,15) = centre, rotation rows (yaw about y), half extents; ids (M,2) int32."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
    ctr = torch.stack([u(-40, 40, n_box), u(-3, 3, n_box), u(2, 80, n_box)], -1)
    yaw = u(0, math.pi, n_box)
    c, s, z0, o1 = torch.cos(yaw), torch.sin(yaw), torch.zeros(n_box), torch.ones(n_box)
    rot = torch.stack([c, z0, s, z0, o1, z0, -s, z0, c], -1)
    ext = u(0.5, 4.0, n_box, 3)
    box = torch.cat([ctr, rot, ext], -1).float().contiguous()
    ids = torch.stack([torch.randint(0, max(n_sem, 1), (n_box,), generator=g),
                       torch.randint(0, max(n_inst, 1), (n_box,), generator=g)], -1).int().contiguous()
    return box, ids


# outlines of primitive_scene's two extruded pieces, in the object's local x-y plane (metres)
L_OUTLINE = ((-12.0, 4.0), (12.0, 4.0), (12.0, 40.0), (2.0, 40.0), (2.0, 18.0), (-12.0, 18.0))
U_OUTLINE = ((-20.0, 50.0), (20.0, 50.0), (20.0, 70.0), (14.0, 70.0), (14.0, 56.0), (-14.0, 56.0), (-14.0, 70.0), (-20.0, 70.0))


def primitive_scene(n_box=4, n_sem=45, n_inst=32, seed=1):
    """A small seeded scene of bounding primitives as one primitives.ConvexSet: n_box cuboids (random_boxes), an L-shaped
    ground slab below camera_rays' origin (4 prisms) and a U-shaped wall across the view (6 prisms).  The outlines lie in the
    world x-z plane and are extruded along y (the camera's down axis); the seed shifts them by up to a metre.  The extruded
    pieces' ids are (semantic, 0) with two seeded classes."""
    from .primitives import ConvexSet, extrude_polygon
    box, ids = random_boxes(n_box, n_sem, n_inst, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    dx, dz = (2.0 * torch.rand(2, generator=g) - 1.0).tolist()
    sem = torch.randint(0, max(n_sem, 1), (2,), generator=g).tolist()
    to_world = [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]         # local (x, y, z) -> world (x, z, y): orthogonal
    ground = extrude_polygon(L_OUTLINE, 3.0, 3.5, to_world, (dx, 0.0, dz), (sem[0], 0))
    wall = extrude_polygon(U_OUTLINE, -4.0, 3.0, to_world, (dx, 0.0, dz), (sem[1], 0))
    return ConvexSet.concat(ConvexSet.from_boxes(box.numpy(), ids.numpy()), ground, wall)


def trained_like_(net, sigma_bias=0.03, seed=0):
    """Shift the density bias so a useful fraction of samples has alpha > 0 (a freshly
    initialised NeRF composites to almost nothing)."""
    with torch.no_grad():
        for n in (net.nerf_0, net.nerf_1):
            if n is not None:
                n.alpha_linear.bias.fill_(sigma_bias)
    return net


STEREO_LAYERS = ((5, None), (17, (0.25, 0.75, 0.3, 0.7)))      # background at disparity 5, a central box at 17


def stereo_pair(height, width, layers=STEREO_LAYERS, seed=0, device=None):
    """A random-dot stereogram with integer-disparity layers, for tests and examples of `stereo`: a rectified pair whose true
    disparity is known.  layers: (disparity, rect) from back to front, rect = (top, bottom, left, right) as fractions of the
    LEFT image, None = the whole image; disparities must not decrease (a nearer layer hides a farther one).  The left image
    is uniform random bytes; a left pixel at x of a layer with disparity d is seen in the right image at x - d, nearer layers
    painted last; right pixels that no left pixel reaches keep random bytes of their own.  Made with numpy, seeded.  Returns
    (left, right, disparity, visible): (H, W) uint8 images, the left view's disparity as int32 and the bool mask of left
    pixels that are visible in both images -- CPU tensors, as this module's, or on `device`."""
    import numpy as np
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError("stereo_pair: height and width must be >= 1")
    layers = tuple(layers)
    if not layers or layers[0][1] is not None:
        raise ValueError("stereo_pair: the first layer must cover the image (rect None)")
    rng = np.random.default_rng(int(seed))
    left = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    right = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    disp = np.zeros((H, W), dtype=np.int32)
    last = None
    for d, rect in layers:
        d = int(d)
        if d < 0 or (last is not None and d < last):
            raise ValueError("stereo_pair: disparities must be >= 0 and must not decrease from back to front")
        last = d
        if rect is None:
            disp[:] = d
        else:
            t, b, l, r = rect
            disp[int(round(t * H)):int(round(b * H)), int(round(l * W)):int(round(r * W))] = d
    owner = np.full((H, W), -1, dtype=np.int64)             # the left column that each right pixel shows
    ys, xs = np.mgrid[0:H, 0:W]
    for d in sorted(set(int(v) for v in disp.reshape(-1))):
        sel = (disp == d) & (xs - d >= 0)
        right[ys[sel], xs[sel] - d] = left[ys[sel], xs[sel]]
        owner[ys[sel], xs[sel] - d] = xs[sel]
    xr = xs - disp
    visible = (xr >= 0) & (owner[ys, np.clip(xr, 0, W - 1)] == xs)
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (left, right, disp, visible))
    return out if device is None else tuple(t.to(device) for t in out)


def blobs(shape, seed=0, n=6, radius=(1, 4), gap=2):
    """Non-touching balls (discs in 2-D) in a lattice, for tests and timings of `components`: a bool mask with a known answer.
    shape: (height, width) or (res_z, res_y, res_x).  Up to n balls of integer radius within `radius` (inclusive) are placed
    at seeded random integer centres, whole inside the lattice; a ball that would come within `gap` cells (Chebyshev, between
    bounding boxes) of an earlier one is dropped, so no two touch at any connectivity.  A ball is the cells with squared
    distance <= r^2 from its centre: connected at the 4 / 6 connectivity.  Returns (mask bool tensor, count, sizes): count the
    number of balls placed and sizes (count,) int64 numpy, in the order components numbers them (raster order of the first
    cell).  CPU tensor; numpy, seeded."""
    import numpy as np
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError("blobs: shape must be (height, width) or (res_z, res_y, res_x), every size >= 1")
    r_lo, r_hi = int(radius[0]), int(radius[1])
    if not 0 <= r_lo <= r_hi or int(gap) < 1:
        raise ValueError("blobs: radius must be (lo, hi) with 0 <= lo <= hi, gap >= 1")
    rng = np.random.default_rng(int(seed))
    mask = np.zeros(shape, dtype=bool)
    placed = []
    grids = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    for _ in range(int(n)):
        r = int(rng.integers(r_lo, r_hi + 1))
        if any(s < 2 * r + 1 for s in shape):
            continue
        c = [int(rng.integers(r, s - r)) for s in shape]
        if any(all(abs(c[k] - q[k]) <= r + rq + int(gap) for k in range(len(shape))) for q, rq in placed):
            continue
        placed.append((c, r))
        mask |= sum((g - ck) ** 2 for g, ck in zip(grids, c)) <= r * r
    firsts = []
    for c, r in placed:
        ball = sum((g - ck) ** 2 for g, ck in zip(grids, c)) <= r * r
        firsts.append((int(np.flatnonzero(ball.reshape(-1))[0]), int(ball.sum())))
    firsts.sort()
    return torch.from_numpy(mask), len(placed), np.asarray([s for _, s in firsts], dtype=np.int64)


SDF_KINDS = ("sphere", "torus", "box", "plane")


def sdf_grid(kind, lo, hi, res, center=(0.0, 0.0, 0.0), radius=0.7, minor=0.25, half=(0.5, 0.5, 0.5), axis=0, offset=0.0, device=None):
    """An analytic field on the lattice `Network.query_grid` defines over the box [lo, hi] (res an int or (res_x, res_y, res_z)),
    for tests and examples of `mesh`: POSITIVE INSIDE, the negated signed distance, so its surface is the level 0.
      sphere: radius - |p - center|;      torus: minor - the distance to the circle of `radius` round the z axis through center;
      box: the negated signed distance of the axis-aligned box center +- half;      plane: p[axis] - offset.
    The coordinates are query_grid's float32 cell centres, lo + (i + 0.5) * step (a multiply, then an add); the field is made
    from them with numpy in float32, op by op.  Returns a (res_z, res_y, res_x) float32 tensor, on the CPU or on `device`."""
    import numpy as np
    if kind not in SDF_KINDS:
        raise ValueError("sdf_grid: unknown kind %r (%s)" % (kind, ", ".join(SDF_KINDS)))
    r = (int(res),) * 3 if isinstance(res, int) else tuple(int(v) for v in res)
    if len(r) != 3 or min(r) < 1:
        raise ValueError("sdf_grid: res must be a positive int or (res_x, res_y, res_z)")
    lo32, hi32 = np.asarray(lo, dtype=np.float32).reshape(-1), np.asarray(hi, dtype=np.float32).reshape(-1)
    if lo32.shape != (3,) or hi32.shape != (3,):
        raise ValueError("sdf_grid: lo and hi must be 3-vectors")
    if axis not in (0, 1, 2):
        raise ValueError("sdf_grid: axis must be 0, 1 or 2")
    step = (hi32 - lo32) / np.asarray(r, dtype=np.float32)
    ax = [(np.arange(r[a]).astype(np.float32) + np.float32(0.5)) * step[a] + lo32[a] for a in range(3)]
    c = np.asarray(center, dtype=np.float32).reshape(3)
    Z, Y, X = np.meshgrid(ax[2] - c[2], ax[1] - c[1], ax[0] - c[0], indexing="ij")
    if kind == "sphere":
        f = np.float32(radius) - np.sqrt(X * X + Y * Y + Z * Z)
    elif kind == "torus":
        q = np.sqrt(X * X + Y * Y) - np.float32(radius)
        f = np.float32(minor) - np.sqrt(q * q + Z * Z)
    elif kind == "box":
        h = np.asarray(half, dtype=np.float32).reshape(3)
        d = [np.abs(X) - h[0], np.abs(Y) - h[1], np.abs(Z) - h[2]]
        out = np.sqrt(sum(np.maximum(v, np.float32(0.0)) ** 2 for v in d))
        f = -(out + np.minimum(np.maximum(np.maximum(d[0], d[1]), d[2]), np.float32(0.0)))
    else:
        f = (X, Y, Z)[axis] + c[axis] - np.float32(offset)
    t = torch.from_numpy(np.ascontiguousarray(f.astype(np.float32)))
    return t if device is None else t.to(device)


def camera_directions(camera):
    """(height, width, 3) float64 camera-space ray directions of a camera.Pinhole / Fisheye / Equirect and (height, width) bool
    = the pixel sees anything, in closed form on the CPU (the fisheye polynomial by Newton's method run until nothing moves): a
    pinhole direction has z = 1 (its parameter is z-depth), a fisheye or equirect direction is unit length (its parameter is
    range), the conventions of render_view.  For analytic test scenes; the GPU rays are ops.gen_rays*."""
    h, w = int(camera.height), int(camera.width)
    j, i = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    # the float32 parameters the kernels get (ops._host_floats), widened: the scene is exact for the camera the GPU sees
    par = [float(v) for v in torch.tensor(camera.params, dtype=torch.float32).tolist()]
    if camera.model == "pinhole":
        fx, fy, cx, cy = par
        return torch.stack([(i - cx) / fx, (j - cy) / fy, torch.ones_like(i)], -1), torch.ones((h, w), dtype=torch.bool)
    if camera.model == "equirect":
        lon0, dlon, lat0, dlat = par
        lam, psi = math.pi * (lon0 + (i + 0.5) * dlon), math.pi * (lat0 + (j + 0.5) * dlat)
        return torch.stack([torch.cos(psi) * torch.sin(lam), torch.sin(psi), torch.cos(psi) * torch.cos(lam)], -1), torch.ones((h, w), dtype=torch.bool)
    if camera.model != "fisheye":
        raise ValueError("camera_directions: unknown camera model %r" % (camera.model,))
    xi, k1, k2, g1, g2, u0, v0 = par
    x, y = (i - u0) / g1, (j - v0) / g2
    rd = torch.sqrt(x * x + y * y)
    r = rd.clone()
    for _ in range(100):
        r2 = r * r
        step = (r * (1.0 + k1 * r2 + k2 * r2 * r2) - rd) / (1.0 + 3.0 * k1 * r2 + 5.0 * k2 * r2 * r2)
        r = r - step
        if not bool((step.abs() > 1e-16 * r.abs().clamp(min=1.0)).any()):
            break
    sc = torch.where(rd > 0, r / rd.clamp(min=1e-300), torch.ones_like(rd))
    x, y = x * sc, y * sc
    r2 = x * x + y * y
    disc = 1.0 + (1.0 - xi * xi) * r2
    ok = disc >= 0
    lam = (xi + torch.sqrt(disc.clamp(min=0.0))) / (r2 + 1.0)
    d = torch.stack([lam * x, lam * y, lam - xi], -1)
    return torch.where(ok[..., None], d, torch.zeros_like(d)), ok


def room_depth(camera, c2w, lo, hi, normals=False):
    """The analytic depth image of the axis-aligned box [lo, hi] seen from INSIDE, for a camera of any model at the 3x4 (or 4x4)
    pose c2w: (height, width) float32 in render_view's convention (z-depth in a pinhole, range in a fisheye / equirect frame), 0
    where a fisheye pixel sees nothing.  A room is not symmetric, so -- unlike a sphere -- it pins all six degrees of freedom of
    a pose: the scene of the tracking tests.  Float64 closed form on the CPU, rounded once.  normals=True: also the (height,
    width, 3) float32 world-space unit normal of the wall each pixel sees, pointing into the room (0 where depth is 0)."""
    m = torch.as_tensor(c2w, dtype=torch.float64).reshape(-1)
    if m.numel() == 16:
        m = m[:12]
    if m.numel() != 12:
        raise ValueError("room_depth: c2w must be a 3x4 (or 4x4) matrix")
    m = m.reshape(3, 4)
    lo64, hi64 = torch.as_tensor(lo, dtype=torch.float64).reshape(-1), torch.as_tensor(hi, dtype=torch.float64).reshape(-1)
    if lo64.numel() != 3 or hi64.numel() != 3:
        raise ValueError("room_depth: lo and hi must be 3-vectors")
    o = m[:, 3]
    if not bool(((lo64 < o) & (o < hi64)).all()):
        raise ValueError("room_depth: the camera centre %r must lie strictly inside the box" % (o.tolist(),))
    dc, ok = camera_directions(camera)
    d = dc @ m[:, :3].T
    wall = torch.where(d > 0, hi64, lo64)                                # the wall each axis' component runs towards
    t = torch.where(d != 0, (wall - o) / torch.where(d != 0, d, torch.ones_like(d)), torch.full_like(d, float("inf")))
    depth, axis = t.min(dim=-1)
    depth = torch.where(ok, depth, torch.zeros_like(depth)).to(torch.float32)
    if not normals:
        return depth
    n = torch.zeros_like(d)
    n.scatter_(-1, axis[..., None], -torch.sign(torch.gather(d, -1, axis[..., None])))
    return depth, torch.where(ok[..., None], n, torch.zeros_like(n)).to(torch.float32)


def icosphere(subdiv=2, radius=1.0, center=(0.0, 0.0, 0.0), device=None):
    """A closed triangle mesh of the sphere, for tests and examples of `mesh.raycast`: the icosahedron, every face split in
    four `subdiv` times with the new vertices pushed out to the sphere -- 20 * 4^subdiv faces wound so that the normals point
    outwards, every edge shared by exactly two faces.  Float64 on the host, then center + radius * v rounded to float32 once.
    Returns a mesh.Mesh.from_arrays mesh, on the CPU or on `device`."""
    import numpy as np
    from .mesh import Mesh
    subdiv = int(subdiv)
    if not 0 <= subdiv <= 7:
        raise ValueError("icosphere: subdiv must be within 0 .. 7 (got %d)" % subdiv)
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def middle(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.asarray(center, np.float64).reshape(1, 3) + float(radius) * np.asarray(v)).astype(np.float32)
    return Mesh.from_arrays(verts, np.asarray(f, np.int32), device=device)


def box_mesh(lo, hi, device=None):
    """The axis-aligned box [lo, hi] as 8 vertices and 12 faces wound so that the normals point INTO the room: the mesh of the
    scene `room_depth` renders in closed form.  Vertex i has the hi coordinate on axis k where bit k of i is set.  Returns a
    mesh.Mesh.from_arrays mesh, on the CPU or on `device`."""
    import numpy as np
    from .mesh import Mesh
    lo32, hi32 = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
    if lo32.shape != (3,) or hi32.shape != (3,) or not (np.isfinite(lo32).all() and np.isfinite(hi32).all() and (lo32 < hi32).all()):
        raise ValueError("box_mesh: lo and hi must be finite 3-vectors with lo < hi on every axis")
    verts = np.asarray([[(hi32 if (i >> k) & 1 else lo32)[k] for k in range(3)] for i in range(8)], np.float32)
    faces = []
    for k in range(3):
        u, w = (k + 1) % 3, (k + 2) % 3                  # e_u x e_w = e_k: this order winds a wall's normal along +k
        for top in (0, 1):
            q = [(top << k) | (a << u) | (b << w) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
            q = q[::-1] if top else q
            faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return Mesh.from_arrays(verts, np.asarray(faces, np.int32), device=device)
