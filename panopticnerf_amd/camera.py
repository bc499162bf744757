"""Camera models behind one interface: Pinhole (the rectified perspective pair), Fisheye (the side-facing cameras of a
360 rig) and Equirect (a panorama over longitude x latitude).  All make rays on the GPU (`rays`), say which pixels see anything
(`valid_pix`) and carry 3D points into the image (`project`); `Renderer.render_view` renders a frame of any, and
`consistency.reproject` joins two such frames.

The fisheye model is the unified omnidirectional (MEI) model with two radial terms as the public KITTI-360 calibration files
parametrise it, written out in include/pnr.h ("cameras") and DESIGN.md ("Fisheye cameras"); like every convention of this
build it is unpinned against the reference's own 360 code.  Fisheye and Equirect rays are UNIT LENGTH (depth along them is
range); pinhole rays keep `ops.gen_rays`' convention (z_cam = 1, depth is z-depth).
"""
import math

import numpy as np
import torch

from . import _lib, ops


def _rows3(t, msg):
    """the 12 values of a 3x4 pose, or the first 12 of a 4x4 one, flat; anything else is refused with `msg`"""
    t = t.reshape(-1)
    if t.numel() == 16:
        t = t[:12]
    if t.numel() != 12:
        raise ValueError(msg)
    return t


def _pose12(m, what):
    return _rows3(torch.as_tensor(m, dtype=torch.float32), f"{what}: expected a 3x4 (or 4x4) matrix")


def invert_pose(c2w):
    """w2c (3, 4) float32 of a rigid c2w = [R | t] (3x4 or 4x4): [R^T | -R^T t], computed in float64 on the host and rounded to
    float32 once.  Every w2c of the cross-view code (consistency.py, Evaluator.evaluate_pair) is made this way, so a pose
    pair means the same bits everywhere."""
    if isinstance(c2w, torch.Tensor):
        m = c2w.detach().cpu().to(torch.float64)
    else:
        m = torch.as_tensor(np.asarray(c2w, dtype=np.float64))     # (torch would read python floats as float32)
    m = _rows3(m, "invert_pose: expected a 3x4 (or 4x4) matrix").reshape(3, 4)
    rt = m[:, :3].T
    return torch.cat([rt, -(rt @ m[:, 3:])], 1).to(torch.float32)


def is_camera(cam):
    """a Pinhole / Fisheye / Equirect, or an object with what the ops and their wrappers read of one (the attributes below)"""
    return all(hasattr(cam, k) for k in ("model", "word", "params", "width", "height"))


class _Camera:
    """Shared half of the models: the per-device cache of valid pixels, the GPU-device check and projection.  A model adds
    `model` (its name), `word` (the model word of include/pnr.h PNR_CAMERA_*), `params` (the camera floats that go with the
    word), `rays` and, where not every pixel sees something, `all_valid = False` and `_find_valid`."""
    all_valid = True

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise ValueError("camera: width and height must be >= 1")
        self._valid_pix = {}

    @staticmethod
    def _device(device, pix=None):
        dev = pix.device if pix is not None else torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("camera: expected a GPU device (the HIP path has no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    def valid_pix(self, device=None):
        """Sorted int32 linear indices (j * width + i) of the pixels that see anything, on `device`.  Depends on the intrinsics
        (and the user mask) only, never on the pose: computed once per camera and device, then the SAME tensor is returned, so
        after the first frame a frame costs no host synchronisation."""
        dev = self._device(device)
        if dev not in self._valid_pix:
            self._valid_pix[dev] = self._find_valid(dev)
        return self._valid_pix[dev]

    def _find_valid(self, dev):
        return torch.arange(self.width * self.height, dtype=torch.int32, device=dev)

    def project(self, points, w2c):
        """World points (P, 3) on the GPU -> uv (P, 2), range (P) = distance from the camera centre, valid (P) bool: inside
        the model's domain (its class docstring) and inside the image."""
        name = type(self).__name__
        uv, rng, valid = ops.project_points(self.model, self.params, _pose12(w2c, f"{name}.project: w2c"), self.width, self.height, points)
        return uv, rng, valid.bool()


class Pinhole(_Camera):
    """fx, fy, cx, cy as `ops.gen_rays`: d = R ((i - cx)/fx, (j - cy)/fy, 1), every pixel valid.  `project`: valid where z_cam > 0
    and inside the image; z-depth is range times the z of the unit direction, or uv back through the intrinsics."""
    model, word = "pinhole", _lib.CAMERA_PINHOLE

    def __init__(self, fx, fy, cx, cy, width, height):
        super().__init__(width, height)
        self.intr = self.params = (float(fx), float(fy), float(cx), float(cy))
        if self.intr[0] == 0.0 or self.intr[1] == 0.0:
            raise ValueError("Pinhole: zero focal length")

    def rays(self, c2w, near, far, pix=None, device=None):
        """(R, 8) rays of the whole frame or of the int32 GPU pixel indices `pix` (ops.gen_rays)."""
        return ops.gen_rays(self.intr, _pose12(c2w, "Pinhole.rays: c2w"), self.width, self.height, near, far, pix=pix,
                            device=None if pix is not None else self._device(device))


class Fisheye(_Camera):
    """xi, k1, k2, gamma1, gamma2, u0, v0 of the MEI model (include/pnr.h "cameras").  mask: optional (height, width) bool /
    0-1 array, True where the pixel is to be used (e.g. the dataset's mask of the car body); it only narrows `valid_pix`.
    `project`: range is what depth_* of a fisheye render holds; valid for a direction the lens sees and inside the image (the
    user mask is not consulted)."""
    model, word, all_valid = "fisheye", _lib.CAMERA_FISHEYE, False

    def __init__(self, xi, k1, k2, gamma1, gamma2, u0, v0, width, height, mask=None):
        super().__init__(width, height)
        self.cam = self.params = tuple(float(v) for v in (xi, k1, k2, gamma1, gamma2, u0, v0))
        if not all(math.isfinite(v) for v in self.cam):
            raise ValueError("Fisheye: non-finite parameter")
        if self.cam[0] < 0.0:
            raise ValueError("Fisheye: xi must be >= 0")
        if self.cam[3] == 0.0 or self.cam[4] == 0.0:
            raise ValueError("Fisheye: zero gamma")
        self._check_monotone()
        self.mask = None
        if mask is not None:
            m = torch.as_tensor(mask).detach().cpu() != 0
            if tuple(m.shape) != (self.height, self.width):
                raise ValueError("Fisheye: mask must be (height, width) = (%d, %d), not %s" % (self.height, self.width, tuple(m.shape)))
            self.mask = m.reshape(-1)

    def _check_monotone(self):
        """The un-projection inverts r (1 + k1 r^2 + k2 r^4) by Newton's method, which needs the polynomial strictly increasing
        (derivative g = 1 + 3 k1 r^2 + 5 k2 r^4 > 0) from the centre up to the rim: r^2 = 1/(xi^2 - 1) for xi > 1, else the
        radius of the farthest image corner."""
        xi, k1, k2, g1, g2, u0, v0 = self.cam
        g = lambda t: 1.0 + 3.0 * k1 * t + 5.0 * k2 * t * t         # t = r^2
        poly = lambda r: r * (1.0 + k1 * r * r + k2 * r ** 4)
        if xi > 1.0:
            r_hi = 1.0 / math.sqrt(xi * xi - 1.0)
        else:
            rd_max = max(math.hypot((i - u0) / g1, (j - v0) / g2) for i in (0, self.width - 1) for j in (0, self.height - 1))
            r_hi, n = max(rd_max, 1e-6), 0
            while poly(r_hi) < rd_max and g(r_hi * r_hi) > 0.0 and n < 64:
                r_hi, n = r_hi * 1.5, n + 1
            if poly(r_hi) < rd_max and g(r_hi * r_hi) > 0.0:
                raise ValueError("Fisheye: the radial polynomial never reaches the image corners")
        T = r_hi * r_hi
        cand = [T * k / 1024.0 for k in range(1025)]
        if k2 != 0.0:
            cand.append(min(max(-3.0 * k1 / (10.0 * k2), 0.0), T))   # the vertex of g, where it lies inside
        worst = min(g(t) for t in cand)
        if not worst > 0.0:
            raise ValueError("Fisheye: the radial polynomial 1 + k1 r^2 + k2 r^4 times r is not strictly increasing up to the rim "
                             "(r = %.4g): its derivative falls to %.3g -- k1 = %g, k2 = %g cannot be un-projected" % (r_hi, worst, k1, k2))

    def _find_valid(self, dev):
        eye = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        _, valid = ops.gen_rays_fisheye(self.cam, eye, self.width, self.height, 0.0, 1.0, device=dev)
        valid = valid != 0
        if self.mask is not None:
            valid &= self.mask.to(dev)
        return torch.nonzero(valid).reshape(-1).to(torch.int32)      # (the camera's one host synchronisation per device)

    def rays(self, c2w, near, far, pix=None, device=None):
        """(R, 8) rays of the whole frame or of the int32 GPU pixel indices `pix` (ops.gen_rays_fisheye): unit-length d; a
        pixel outside the lens gets d = 0, near = far = 0 -- pass pix = valid_pix() to leave those out."""
        return ops.gen_rays_fisheye(self.cam, _pose12(c2w, "Fisheye.rays: c2w"), self.width, self.height, near, far, pix=pix,
                                    device=None if pix is not None else self._device(device), want_valid=False)[0]


class Equirect(_Camera):
    """A panoramic camera: columns are longitudes, rows latitudes (include/pnr.h "cameras", DESIGN.md "Panoramic camera").
    lon = (left edge, right edge) and lat = (top edge, bottom edge) in DEGREES, longitude 0 along the camera's +z and positive
    towards +x, latitude positive up; the default is the full sphere.  A right edge below the left one mirrors the image, a
    left edge of e.g. 90 with a right edge of 270 crosses the +-180 degree seam.  Unit-length rays (depth is range), every pixel
    valid; projection wraps longitude round the circle.  `project`: range is what depth_* of an equirect render holds; valid for
    any point but the camera centre itself whose direction falls inside the image."""
    model, word = "equirect", _lib.CAMERA_EQUIRECT

    def __init__(self, width, height, lon=(-180.0, 180.0), lat=(90.0, -90.0)):
        super().__init__(width, height)
        lon_l, lon_r = (float(v) for v in lon)
        lat_t, lat_b = (float(v) for v in lat)
        if not all(math.isfinite(v) for v in (lon_l, lon_r, lat_t, lat_b)):
            raise ValueError("Equirect: non-finite angle")
        if lon_l == lon_r or lat_t == lat_b:
            raise ValueError("Equirect: zero span (lon and lat are (left, right) and (top, bottom) edges in degrees)")
        if abs(lon_r - lon_l) > 360.0:
            raise ValueError("Equirect: a longitude span above 360 degrees")
        if abs(lat_t) > 90.0 or abs(lat_b) > 90.0:
            raise ValueError("Equirect: latitude outside +-90 degrees")
        if abs(lon_l) > 180.0:
            raise ValueError("Equirect: the left edge must lie in +-180 degrees")
        self.lon, self.lat = (lon_l, lon_r), (lat_t, lat_b)
        # half-turns, pitch positive DOWN: float64 on the host, rounded to float32 once (ops._host_floats)
        cam64 = (lon_l / 180.0, (lon_r - lon_l) / 180.0 / self.width, -lat_t / 180.0, (lat_t - lat_b) / 180.0 / self.height)
        self.cam = self.params = tuple(float(torch.tensor(v, dtype=torch.float64).to(torch.float32)) for v in cam64)
        if self.cam[1] == 0.0 or self.cam[3] == 0.0:
            raise ValueError("Equirect: zero span (the step per pixel underflows float32)")

    def rays(self, c2w, near, far, pix=None, device=None):
        """(R, 8) rays of the whole frame or of the int32 GPU pixel indices `pix` (ops.gen_rays_equirect): unit-length d."""
        return ops.gen_rays_equirect(self.cam, _pose12(c2w, "Equirect.rays: c2w"), self.width, self.height, near, far, pix=pix,
                                     device=None if pix is not None else self._device(device))
