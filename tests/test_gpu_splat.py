"""Point splatting and the depth metrics on an MI355X: k_splat_points / k_splat_resolve / k_depth_metrics (csrc/pnr_splat.hip)
against tests/_splat_ref.py's restatement of the rule (include/pnr.h "point splatting").  The z-buffer, the two resolved images
and every counter are integers or float32 words that must be EQUAL; only the metric sums (float64, another summation order
than math.fsum) carry a bound, the one _splat_ref.metrics32_64 derives per term (test_depth_metrics prints the largest share of
it that each case uses), and the four sums without a logarithm also equal _reduce_ref's restatement of the kernel's order of
additions bit for bit.  tests/test_splat_ref.py pins the restatement on the CPU."""
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _camera_ref as cr
import _pano_ref as pr
import _reduce_ref as rr
import _splat_ref as sr
from panopticnerf_amd import Equirect, Fisheye, Pinhole, camera, make_network, make_renderer, ops, pointcloud, synthetic
from panopticnerf_amd.evaluate import Evaluator

pytestmark = pytest.mark.gpu

XI, K1, K2 = 2.2134, 0.016798, 1.6548
# the three models x two (size, pose) each: 64 x 48 and 37 x 19 (odd, no multiple of anything)
VIEWS = {"pinhole_a": (Pinhole(40.0, 41.0, 31.5, 23.5, 64, 48), cr.pose(0.3, 0.0, (0.0, 1.55, 0.0))),
         "pinhole_b": (Pinhole(30.0, 31.0, 18.2, 9.1, 37, 19), cr.pose(-2.2, 0.35, (-2.5, 0.8, 4.25))),
         "fisheye_a": (Fisheye(XI, K1, K2, 91.0, 90.5, 31.2, 23.6, 64, 48), cr.pose(np.pi / 2, 0.0, (1.0, 1.55, -0.5))),
         "fisheye_b": (Fisheye(XI, K1, K2, 50.0, 50.5, 18.4, 8.9, 37, 19), cr.pose(0.6, -0.1, (0.5, 1.4, -1.0))),
         "equirect_a": (Equirect(64, 48), cr.pose(0.3, 0.0, (0.0, 1.55, 0.0))),
         "equirect_b": (Equirect(37, 19, lon=(100.0, 250.0), lat=(60.0, -40.0)), cr.pose(1.2, 0.1, (-2.0, 1.0, 1.0)))}      # crosses the seam
CONTENDED = 210         # points forced onto one pixel: 150 distinct depths + 60 at one depth, nearer than anything else


def N_(t):
    return t.detach().cpu().numpy()


def T(a, dev):
    return None if a is None else torch.as_tensor(a).to(dev)


def words(cam):
    return {"pinhole": (sr.PINHOLE, getattr(cam, "intr", None)), "fisheye": (sr.FISHEYE, getattr(cam, "cam", None)),
            "equirect": (sr.EQUIRECT, getattr(cam, "cam", None))}[cam.model]


def ref_view(cam, pose):
    m, w = words(cam)
    return (m, np.asarray(w, np.float32), np.asarray(pose, np.float32), cam.width, cam.height)


def w2c_of(c2w):
    return N_(camera.invert_pose(np.asarray(c2w, np.float32)))


def bits(zbuf):
    return N_(zbuf).reshape(-1).view(np.uint64)


def cloud(cam, c2w, n, seed=0):
    """(n, 3) float32 world points around the camera: random ones (inside, outside, behind), NaN / Inf coordinates, the camera
    centre, the rays of the four corner pixels (the footprint meets the border there), and CONTENDED points along the ray of
    one pixel centre, at distinct depths and at one repeated depth.  Returns (points, the contended pixel or None)."""
    g = np.random.default_rng(seed)
    c2w = np.asarray(c2w, np.float32)
    o = c2w[:, 3].astype(np.float64)
    pts = o + g.normal(size=(n, 3)) * g.uniform(1.0, 12.0, (n, 1))
    hot = None
    if n >= 255:
        w, h = cam.width, cam.height
        src = ref_view(cam, c2w)
        pix = np.array([(h // 2 + 1) * w + w // 2 - 2, 0, w - 1, (h - 1) * w, h * w - 1], np.int64)
        _, d, ok = pr._rays(np.float64, src, pix)
        assert ok.all()
        hot = int(pix[0])
        t = np.concatenate([np.linspace(3.0, 20.0, CONTENDED - 60), np.full(60, 0.05)])
        g.shuffle(t)
        k = 20
        pts[k:k + CONTENDED] = o + t[:, None] * d[0]
        pts[k + CONTENDED:k + CONTENDED + 4] = o + 6.0 * d[1:]
        pts[:8] = [[np.nan, 0, 5], [0, np.inf, 5], [-np.inf, 1, 1], [1e38, -1e38, 1e38], o, o, o - 5.0 * c2w[:, 2], o - 0.5 * c2w[:, 2]]
    return pts.astype(np.float32), hot


# ------------------------------------------------------------------------------------------------ 1: the main sweep
@pytest.mark.parametrize("name", list(VIEWS))
def test_splat_bit_for_bit(dev, name):
    cam, c2w = VIEWS[name]
    w2c = w2c_of(c2w)
    m, cw = words(cam)
    landed_any = 0
    for n, radius, far in itertools.product((0, 1, 255, 4097), (0, 1, 2), (9.0, np.inf)):
        pts, hot = cloud(cam, c2w, n, seed=n)
        if n == 1:
            pts[0] = np.asarray(c2w, np.float32)[:, 3] + 4.0 * np.asarray(c2w, np.float32)[:, 2]          # on the optical axis
        near = 2.75 if far < np.inf else 0.0
        want, wst = sr.splat32(m, np.asarray(cw, np.float32), w2c, cam.width, cam.height, pts, near=near, far=far, radius=radius)
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        z = ops.splat_points(cam, w2c, T(pts, dev).reshape(-1, 3), near=near, far=far, radius=radius, stats=stats)
        what = (name, n, radius, far)
        assert z.dtype == torch.int64 and tuple(z.shape) == (cam.height, cam.width)
        assert np.array_equal(bits(z), want), what
        assert np.array_equal(N_(stats), wst) and int(stats.sum()) == n, what
        landed_any += int(wst[0])
        if n >= 255:
            # the contended cell: at least CONTENDED points of the cloud sit on it, at distinct depths and at one repeated depth
            # (0.05 m: clipped by near in the finite runs, the winner of the cell in the others -- by its lowest index)
            lands, _, iu, iv, e = sr.points32(ref_view(cam, w2c), pts)
            on = np.flatnonzero(lands & (iv * cam.width + iu == hot))
            depths, times = np.unique(e[on], return_counts=True)
            assert on.size >= CONTENDED and depths.size >= 150 and times.max() == 60, what
            assert wst[0] > 0 and wst[1] > 0 and (far == np.inf or wst[2] > 0), what
            if far == np.inf:
                d, idx = sr.resolve(want)
                assert idx[hot] == on[e[on] == depths[0]].min() and times[0] == 60 and d[hot] == depths[0], what
    assert landed_any > 1000


def test_ops_check_dtype_contiguity_and_device(dev):
    cam, c2w = VIEWS["pinhole_a"]
    pts = torch.zeros(5, 3, device=dev)
    with pytest.raises(TypeError, match="points: expected torch.float32"):
        ops.splat_points(cam, c2w, pts.double())
    with pytest.raises(ValueError, match="points: tensor must be contiguous"):
        ops.splat_points(cam, c2w, torch.zeros(3, 5, device=dev).T)
    with pytest.raises(TypeError, match="zbuf: expected torch.int64"):
        ops.splat_points(cam, c2w, pts, zbuf=torch.zeros(48, 64, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.splat_points(cam, c2w, pts, zbuf=torch.zeros(48, 64, dtype=torch.int64))
    with pytest.raises(TypeError, match="stats: expected torch.int64"):
        ops.splat_points(cam, c2w, pts, stats=torch.zeros(3, device=dev))
    with pytest.raises(TypeError, match="zbuf: expected torch.int64"):
        ops.splat_resolve(torch.zeros(48, 64, device=dev))
    with pytest.raises(ValueError, match="zbuf: tensor must be contiguous"):
        ops.splat_resolve(torch.zeros(64, 48, dtype=torch.int64, device=dev).T)
    with pytest.raises(ValueError, match="depth: out must be"):
        ops.splat_resolve(torch.zeros(48, 64, dtype=torch.int64, device=dev), out={"depth": torch.zeros(48, 64, dtype=torch.int32, device=dev)})
    d = torch.ones(4, device=dev)
    with pytest.raises(TypeError, match="gt: expected torch.float32"):
        ops.depth_metrics(d, d.double())
    with pytest.raises(TypeError, match="mask"):
        ops.depth_metrics(d, d, mask=d)
    with pytest.raises(TypeError, match="sums: expected torch.float64"):
        ops.depth_metrics(d, d, sums=torch.zeros(5, device=dev))
    with pytest.raises(TypeError, match="counts: expected torch.int64"):
        ops.depth_metrics(d, d, counts=torch.zeros(5, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_metrics(d.cpu(), d)


# ------------------------------------------------------------------------------------------------ 2: order independence
@pytest.mark.parametrize("name", ["pinhole_b", "fisheye_a", "equirect_b"])
def test_result_does_not_depend_on_order_or_chunking(dev, name):
    cam, c2w = VIEWS[name]
    w2c = w2c_of(c2w)
    pts, hot = cloud(cam, c2w, 4097, seed=11)
    P = T(pts, dev)
    kw = dict(near=0.0, far=30.0, radius=1)
    s0 = torch.zeros(3, dtype=torch.int64, device=dev)
    whole = ops.splat_points(cam, w2c, P, stats=s0, **kw)
    # the same cloud permuted: the winner of every cell is the same POINT (same depth bits, same coordinates; among bit-equal
    # points the lowest index of the order given, so the index itself is carried back through the permutation by coordinates)
    perm = np.random.default_rng(5).permutation(len(pts))
    zp = ops.splat_points(cam, w2c, T(pts[perm], dev), **kw)
    d0, i0 = (N_(t) for t in ops.splat_resolve(whole))
    d1, i1 = (N_(t) for t in ops.splat_resolve(zp))
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(i0 >= 0, i1 >= 0) and (i0 >= 0).sum() > 100
    f = i0 >= 0
    back = perm[i1[f]]
    assert np.array_equal(pts[back].view(np.uint32), pts[i0[f]].view(np.uint32))
    uniq = np.array([np.all(pts == pts[k], 1).sum() == 1 for k in i0[f]])
    assert np.array_equal(back[uniq], i0[f][uniq]) and uniq.sum() > 100
    # three chunks with index_base, in both orders: the same bits as the single call
    cuts = [0, 1000, 1001, len(pts)]
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        z, st = None, torch.zeros(3, dtype=torch.int64, device=dev)
        for k in order:
            z = ops.splat_points(cam, w2c, P[cuts[k]:cuts[k + 1]].contiguous(), zbuf=z, index_base=cuts[k], stats=st, **kw)
        assert torch.equal(z, whole) and torch.equal(st, s0), order


# ------------------------------------------------------------------------------------------------ 3: grid-stride trips
def test_large_cloud_equals_its_slices_and_the_reference(dev):
    """a cloud of 3 x CUs x 8 x 256 + 1000 points (every thread takes 3 or 4): launched whole it equals the union of its slice
    launches into one buffer, and the float32 reference -- on 64 x 48 pixels, so every cell is contended by hundreds of points"""
    cam, c2w = VIEWS["fisheye_a"]
    w2c = w2c_of(c2w)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = 3 * cus * 8 * 256 + 1000
    g = torch.Generator().manual_seed(7)
    pts = (torch.as_tensor(np.asarray(c2w, np.float32)[:, 3]) + torch.randn(n, 3, generator=g) * (1.0 + 9.0 * torch.rand(n, 1, generator=g))).contiguous()
    P = pts.to(dev)
    for radius in (2, 0):
        s0 = torch.zeros(3, dtype=torch.int64, device=dev)
        whole = ops.splat_points(cam, w2c, P, radius=radius, far=25.0, stats=s0)
        cuts = [0, 1, 500001, n - 7, n]
        z, st = None, torch.zeros(3, dtype=torch.int64, device=dev)
        for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
            z = ops.splat_points(cam, w2c, P[a:b].contiguous(), zbuf=z, index_base=a, radius=radius, far=25.0, stats=st)
        assert torch.equal(z, whole) and torch.equal(st, s0) and int(s0.sum()) == n
    m, cw = words(cam)
    want, wst = sr.splat32(m, np.asarray(cw, np.float32), w2c, cam.width, cam.height, pts.numpy(), far=25.0, radius=0)
    assert np.array_equal(bits(whole), want) and np.array_equal(N_(s0), wst) and (wst > 1000).all()


# ------------------------------------------------------------------------------------------------ 4: resolve
def test_resolve_every_output_subset_with_canaries(dev):
    cam, c2w = VIEWS["equirect_a"]
    pts, _ = cloud(cam, c2w, 4097, seed=2)
    z = ops.splat_points(cam, w2c_of(c2w), T(pts, dev), radius=0)
    wd, wi = sr.resolve(N_(z))
    assert (wi >= 0).sum() > 100 and (wi < 0).sum() > 100
    npix = z.numel()
    for want in (("depth", "index"), ("depth",), ("index",), ()):
        fd = torch.full((npix + 16,), 7.5, device=dev)
        fi = torch.full((npix + 16,), 12345, dtype=torch.int32, device=dev)
        out = {}
        if "depth" in want:
            out["depth"] = fd[8:8 + npix].view(cam.height, cam.width)
        if "index" in want:
            out["index"] = fi[8:8 + npix].view(cam.height, cam.width)
        d, i = ops.splat_resolve(z, want=(), out=out)
        assert (d is None) == ("depth" not in want) and (i is None) == ("index" not in want)
        if d is not None:
            assert d.data_ptr() == out["depth"].data_ptr() and np.array_equal(N_(d).view(np.uint32), wd.view(np.uint32))
        if i is not None:
            assert i.data_ptr() == out["index"].data_ptr() and np.array_equal(N_(i), wi)
        for buf, v in ((fd, 7.5), (fi, 12345)):
            assert (buf[:8] == v).all() and (buf[-8:] == v).all()
        if "depth" not in want:
            assert (fd == 7.5).all()
        if "index" not in want:
            assert (fi == 12345).all()
    d, i = ops.splat_resolve(z)                               # fresh outputs
    assert np.array_equal(N_(d).view(np.uint32), wd.view(np.uint32)) and np.array_equal(N_(i), wi)
    d, i = ops.splat_resolve(z, want=("index",))
    assert d is None and np.array_equal(N_(i), wi)
    # an all-empty buffer
    d, i = ops.splat_resolve(torch.full((19, 37), -1, dtype=torch.int64, device=dev))
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and not d.any() and (i == -1).all()
    # the resolved depth goes straight into reprojection as the target's depth: holes are "unknown" (-3), never NaN
    assert not torch.isnan(ops.splat_resolve(z)[0]).any()


# ------------------------------------------------------------------------------------------------ 5: the pointcloud module
def test_pointcloud_splat_gathers_labels_and_colours(dev):
    cam, c2w = VIEWS["fisheye_b"]
    w2c = w2c_of(c2w)
    m, cw = words(cam)
    pts, _ = cloud(cam, c2w, 4097, seed=4)
    g = np.random.default_rng(1)
    lab = g.integers(0, 45, len(pts)).astype(np.int32)
    rgb = g.random((len(pts), 3)).astype(np.float32)
    out = pointcloud.splat(cam, np.asarray(c2w, np.float32), T(pts, dev), labels=T(lab, dev), colors=T(rgb, dev), near=1.0, far=20.0, radius=1)
    want, _ = sr.splat32(m, np.asarray(cw, np.float32), w2c, cam.width, cam.height, pts, near=1.0, far=20.0, radius=1)
    wd, wi = sr.resolve(want.reshape(cam.height, cam.width))
    assert set(out) == {"depth", "index", "valid", "zbuf", "label", "rgb"}
    assert np.array_equal(bits(out["zbuf"]), want) and np.array_equal(N_(out["index"]), wi) and np.array_equal(N_(out["valid"]), wi >= 0)
    assert np.array_equal(N_(out["depth"]).view(np.uint32), wd.view(np.uint32))
    assert np.array_equal(N_(out["label"]), np.where(wi >= 0, lab[np.maximum(wi, 0)], -1)) and out["label"].dtype == torch.int32
    assert np.array_equal(N_(out["rgb"]), np.where((wi >= 0)[..., None], rgb[np.maximum(wi, 0)], 0)) and (wi >= 0).sum() > 50
    # a second scan fused into the first: the tables are the concatenated ones
    pts2, _ = cloud(cam, c2w, 255, seed=9)
    lab2 = g.integers(0, 45, len(pts2)).astype(np.int32)
    both = pointcloud.splat(cam, np.asarray(c2w, np.float32), T(pts2, dev), labels=T(np.concatenate([lab, lab2]), dev), near=1.0, far=20.0, radius=1, into=out["zbuf"],
                            index_base=len(pts))
    want2, _ = sr.splat32(m, np.asarray(cw, np.float32), w2c, cam.width, cam.height, pts2, near=1.0, far=20.0, radius=1, zbuf=want, index_base=len(pts))
    assert both["zbuf"].data_ptr() == out["zbuf"].data_ptr() and np.array_equal(bits(both["zbuf"]), want2) and "rgb" not in both
    wi2 = sr.resolve(want2.reshape(cam.height, cam.width))[1]
    assert np.array_equal(N_(both["label"]), np.where(wi2 >= 0, np.concatenate([lab, lab2])[np.maximum(wi2, 0)], -1)) and (wi2 >= len(pts)).any()


def _sphere(cam, c2w, centre, radius):
    m, cw = words(cam)
    cw, c2w = np.asarray(cw, np.float32), np.asarray(c2w, np.float32)
    if m == sr.EQUIRECT:
        return pr.sphere_depth(cw, c2w, cam.width, cam.height, centre, radius)
    import _warp_ref as wr
    return wr.sphere_depth(m, cw, c2w, cam.width, cam.height, centre, radius)


def _lift32(src, depth):
    w, h = src[3], src[4]
    pc = np.arange(w * h, dtype=np.int64)
    o, d, ok = pr._rays(np.float32, src, pc)
    t = np.asarray(depth, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        have = ok & (t > 0) & (np.abs(t) <= sr.FMAX)
    return np.stack([o[k] + t[have] * d[have, k] for k in range(3)], -1).astype(np.float32), pc[have]


@pytest.mark.parametrize("a,b", [("pinhole_a", "fisheye_a"), ("fisheye_a", "equirect_a"), ("equirect_a", "pinhole_a"), ("fisheye_a", "pinhole_b")])
def test_forward_warp_against_the_reference_and_reprojection(dev, a, b):
    cam_a, cam_b = VIEWS[a][0], VIEWS[b][0]
    ca, cb = np.asarray(cr.pose(0.3, 0.0, (0.0, 1.55, 0.0)), np.float32), np.asarray(cr.pose(0.38, -0.04, (0.4, 1.5, 0.3)), np.float32)
    depth = _sphere(cam_a, ca, (0.5, 1.0, 2.0), 12.0)
    depth[5:9, 11:15] = 0.0
    depth[3, 4], depth[3, 5], depth[3, 6] = np.nan, np.inf, -1.5
    maps = {"depth_1": T(depth, dev)}
    g = np.random.default_rng(6)
    lab = g.integers(0, 9, (cam_a.height, cam_a.width)).astype(np.int32)
    rgb = g.random((cam_a.height, cam_a.width, 3)).astype(np.float32)
    # lift: bit for bit reprojection's steps 1-3
    X, pix = pointcloud.lift((cam_a, ca, maps))
    wX, wpix = _lift32(ref_view(cam_a, ca), depth)
    assert np.array_equal(N_(pix), wpix) and pix.dtype == torch.int32 and np.array_equal(N_(X).view(np.uint32), wX.view(np.uint32))
    wb = w2c_of(cb)
    mb, cwb = words(cam_b)
    for radius in (0, 1):
        out = pointcloud.forward_warp((cam_a, ca, maps), cam_b, cb, radius=radius, images={"label": T(lab, dev), "rgb": T(rgb, dev)})
        want, _ = sr.splat32(mb, np.asarray(cwb, np.float32), wb, cam_b.width, cam_b.height, wX, radius=radius)
        wd, wi = sr.resolve(want.reshape(cam_b.height, cam_b.width))
        assert np.array_equal(bits(out["zbuf"]), want) and np.array_equal(N_(out["depth"]).view(np.uint32), wd.view(np.uint32))
        src = np.where(wi >= 0, wpix[np.maximum(wi, 0)], -1)
        assert np.array_equal(N_(out["source"]), src) and (wi >= 0).sum() > 100
        assert (wi < 0).any() or radius or b == "pinhole_b"                                               # a forward scatter leaves holes
        assert np.array_equal(N_(out["images"]["label"]), np.where(src >= 0, lab.reshape(-1)[np.maximum(src, 0)], -1))
        assert np.array_equal(N_(out["images"]["rgb"]), np.where((src >= 0)[..., None], rgb.reshape(-1, 3)[np.maximum(src, 0)], 0))
    # the cross-kernel property with the real k_reproject (radius 0): every source pixel it sends to q is beaten or met there,
    # and every cell's winner is a source pixel it sends there, at the depth it expects
    out = pointcloud.forward_warp((cam_a, ca, maps), cam_b, cb)
    match = N_(ops.reproject(cam_a, ca, maps["depth_1"], cam_b, wb)["match"])
    assert np.array_equal(np.flatnonzero(match != -1), wpix)
    z = bits(out["zbuf"])
    idx = N_(out["index"]).reshape(-1)
    lands, _, _, _, e = sr.points32(ref_view(cam_b, wb), wX)          # (e: the kernel's own depth words -- zbuf was equal above)
    assert np.array_equal(lands, match[wpix] >= 0)
    r = np.flatnonzero(lands)
    assert (z[match[wpix[r]]] <= np.array([sr.key(e[k], k) for k in r], np.uint64)).all()
    q = np.flatnonzero(idx >= 0)
    assert set(q) == set(match[wpix[r]]) and np.array_equal(match[wpix[idx[q]]], q)
    # the splatted depth as reprojection's own target depth, tolerance 0: every winner is visible (e == depth[q] to the bit),
    # every other landed pixel is visible too (a tie lost on the index) or occluded by its nearer winner
    vis = N_(ops.reproject(cam_a, ca, maps["depth_1"], cam_b, wb, out["depth"], tol=(0.0, 0.0))["match"])
    assert np.array_equal(vis[wpix[idx[q]]], q)
    lost = np.setdiff1d(wpix[r], wpix[idx[q]])
    assert ((vis[lost] == -4) | (vis[lost] == match[lost])).all()


# ------------------------------------------------------------------------------------------------ 6: stream capture
def test_splat_and_resolve_replay_from_a_captured_graph(dev):
    """one stream, no parallel branches; camera, pose, near / far are baked into the capture, the points are read at replay and
    the buffer is reset inside the capture"""
    cam, c2w = VIEWS["pinhole_a"]
    w2c = w2c_of(c2w)
    pts, _ = cloud(cam, c2w, 4097, seed=3)
    P = T(pts, dev)
    z = torch.full((cam.height, cam.width), -1, dtype=torch.int64, device=dev)
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    out = {"depth": torch.empty((cam.height, cam.width), device=dev), "index": torch.empty((cam.height, cam.width), dtype=torch.int32, device=dev)}

    def run(p, zb, st, o=None):
        zb.fill_(-1)
        ops.splat_points(cam, w2c, p, zbuf=zb, far=15.0, radius=1, stats=st)
        return ops.splat_resolve(zb, out=o)

    run(P, z.clone(), stats.clone())                          # warm call: module loading is not capturable
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        run(P, z, stats, out)
    stats.zero_()
    es = torch.zeros_like(stats)
    seen = []
    for k in range(3):
        P[100 * k:100 * k + 2000] += 0.25 * (k + 1)           # edited in place between replays
        g.replay()
        torch.cuda.synchronize()
        ez = torch.empty_like(z)
        ed, ei = run(P.clone(), ez, es)
        assert torch.equal(z, ez) and torch.equal(out["depth"], ed) and torch.equal(out["index"], ei) and torch.equal(stats, es)
        seen.append(z.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and int(stats.sum()) == 3 * len(pts)


# ------------------------------------------------------------------------------------------------ 7: depth metrics
def _depth_pair(n, seed):
    g = np.random.default_rng(seed)
    gt = g.uniform(0.2, 95.0, n).astype(np.float32)
    pred = (gt * g.uniform(0.6, 1.7, n)).astype(np.float32)
    k = g.integers(0, n, max(n // 9, 1))
    gt[k[0::6]], gt[k[1::6]], gt[k[2::6]] = np.nan, np.inf, 0.0
    pred[k[3::6]], pred[k[4::6]], pred[k[5::6]] = 0.0, np.nan, -3.0
    pw = k[::5]
    gt[pw] = np.float32(2.0) ** g.integers(-2, 6, pw.size)        # exactly ON the strict thresholds
    pred[pw] = gt[pw] * np.float32(g.choice([1.25, 1.5625, 1.953125, 0.8, 0.64], pw.size))
    mask = (g.random(n) < 0.8).astype(np.uint8) * g.integers(1, 255, n).astype(np.uint8)
    return pred, gt, mask


def test_depth_metrics(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    trips3 = 3 * min(1024, 4 * cus) * 256 + 77
    worst = 0.0
    for n, with_mask in list(itertools.product((1, 255, 4097), (False, True))) + [(trips3, True)]:
        pred, gt, mask = _depth_pair(n, n)
        if n == 1:
            pred[:], gt[:], mask[:] = 12.5, 10.0, 1
        ws, wc, wb = sr.metrics32_64(pred, gt, mask if with_mask else None)
        P, G, M = T(pred, dev), T(gt, dev), T(mask, dev) if with_mask else None
        s, c = ops.depth_metrics(P, G, M)
        assert s.dtype == torch.float64 and c.dtype == torch.int64 and tuple(s.shape) == tuple(c.shape) == (5,)
        assert np.array_equal(N_(c), wc), (n, with_mask)
        err = np.abs(N_(s) - ws)
        share = float(np.max(np.where(wb > 0, err / np.where(wb > 0, wb, 1.0), np.where(err > 0, np.inf, 0.0))))
        worst = max(worst, share)
        print("n = %d, mask %s: counts %s, largest |sum - reference| / bound = %.3g" % (n, with_mask, wc.tolist(), share))
        assert (err <= wb).all(), (n, with_mask, err, wb)
        if n > 1:
            assert wc[0] > n // 3 and wc[4] >= 1 and wc[1] < wc[2] < wc[3] < wc[0]
        # two calls on the same input: the same bits (no floating atomics)
        s2, c2 = ops.depth_metrics(P, G, M)
        assert torch.equal(s, s2) and torch.equal(c, c2)
        # a bool mask is the uint8 mask; accumulation over two frames
        if with_mask:
            s3, c3 = ops.depth_metrics(P, G, M != 0)
            assert torch.equal(s, s3) and torch.equal(c, c3)
        pred_b, gt_b, _ = _depth_pair(255, 99)
        sb, cb = ops.depth_metrics(T(pred_b, dev), T(gt_b, dev))
        acc_s, acc_c = ops.depth_metrics(T(pred_b, dev), T(gt_b, dev), sums=s.clone(), counts=c.clone())
        assert torch.equal(acc_c, c + cb) and torch.equal(acc_s, s + sb)
    print("largest share of the derived bound used: %.3g" % worst)
    # an image-shaped input and another range
    pred, gt, _ = _depth_pair(48 * 64, 5)
    s, c = ops.depth_metrics(T(pred.reshape(48, 64), dev), T(gt.reshape(48, 64), dev), d_range=(2.0, 30.0))
    ws, wc, wb = sr.metrics32_64(pred, gt, None, (2.0, 30.0))
    assert np.array_equal(N_(c), wc) and (np.abs(N_(s) - ws) <= wb).all()


# 1 .. 1000: one lane, a wave less one, a wave, two waves, a block less one, a block, two blocks, four; then a second trip
ORDER_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, "second trip")


@pytest.mark.parametrize("n", ORDER_SIZES)
def test_depth_metrics_sums_in_the_stated_order_to_the_bit(dev, n):
    """sums 0 .. 3 (|d|, d^2, |d| / gt, d^2 / gt) equal _reduce_ref's restatement of the order (a thread's stride order, the
    butterfly, the four waves, the rows in block order) bit for bit, for the grid the entry point derives from the device;
    "second trip": just past 256 x the full grid + 1, so threads add a second item.  Their terms are single IEEE + - * / on
    doubles made from float32 inputs, which numpy float64 reproduces exactly.  Sum 4 goes through the device's double log,
    which nobody has shown to be correctly rounded: it stays under the derived bound of _splat_ref.metrics32_64 only.
    Accumulating into given sums is old + new to the bit."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if n == "second trip":
        n = 256 * min(1024, 4 * cus) + 77
    grid = rr.blocks_for(n, 1024, cus, 4)
    pred, gt, mask = _depth_pair(n, 1000 + n)
    if n == 1:
        pred[:], gt[:], mask[:] = 12.5, 10.0, 1
    terms, active = sr.metric_terms(pred, gt, mask)
    assert active.any() and (n < 63 or not active.all())
    want = rr.total(terms[:, :4], active, grid)
    P, G, M = T(pred, dev), T(gt, dev), T(mask, dev)
    s, c = ops.depth_metrics(P, G, M)
    assert int(c[0]) == int(active.sum())
    assert np.array_equal(N_(s)[:4].view(np.uint64), want.view(np.uint64)), (n, grid, N_(s)[:4], want)
    ws, _, wb = sr.metrics32_64(pred, gt, mask)
    assert abs(float(s[4]) - ws[4]) <= wb[4]
    old = torch.tensor([0.1, 1e6 / 3.0, 7.0, 1e-9, 2.5], dtype=torch.float64, device=dev)
    acc_s, acc_c = ops.depth_metrics(P, G, M, sums=old.clone(), counts=c.clone())
    assert np.array_equal(N_(acc_s)[:4].view(np.uint64), (N_(old)[:4] + want).view(np.uint64)) and torch.equal(acc_c, 2 * c)
    assert torch.equal(acc_s[4:], old[4:] + s[4:])


@pytest.fixture(scope="module")
def renderer(dev):
    cfg = NS(D=4, W=128, skips=[2], N_samples=32, N_importance=32, num_classes=5, num_instances=0, precision="bf16")
    torch.manual_seed(3)
    net = make_network(cfg).eval()
    synthetic.trained_like_(net, 0.3)
    return make_renderer(cfg, net.to(dev))


@pytest.mark.parametrize("name", ["pinhole_a", "fisheye_a"])
def test_evaluate_depth_end_to_end(dev, renderer, name):
    """a rendered frame against the depth image a LiDAR scan makes in the same view (pointcloud.splat): summarize() reports
    the reference's metrics of the two images"""
    cam, c2w = VIEWS[name]
    c2w = torch.as_tensor(np.asarray(c2w, np.float32))
    with torch.no_grad():
        out = renderer.render_view(cam, c2w, 0.5, 30.0)
    scan, _ = synthetic.lidar_scan(origin=(0.2, 1.3, -0.1), sphere=((0.0, 1.55, 2.0), 9.0), ground_y=3.0, n_azimuth=720, n_elevation=64,
                                   elevation=(-40.0, 40.0))
    gt = pointcloud.splat(cam, c2w, scan.to(dev), radius=1)
    assert int(gt["valid"].sum()) > 200
    ev = Evaluator()
    assert ev.evaluate_depth(out, gt["depth"], valid=out.get("valid")) == "depth_1"
    ws, wc, wb = sr.metrics32_64(N_(out["depth_1"]), N_(gt["depth"]), None if out.get("valid") is None else N_(out["valid"]))
    assert np.array_equal(N_(ev.depth_counts), wc) and (np.abs(N_(ev.depth_sums) - ws) <= wb).all() and wc[0] > 200
    got, want = ev.summarize(), sr.summary(ws, wc)
    print(name, got)
    assert set(got) == set(want) and ev.summarize() == {}
    n = wc[0]
    for k in ("depth_n", "depth_missing", "depth_d1", "depth_d2", "depth_d3"):
        assert got[k] == want[k]
    for k, j, sq in (("depth_mae", 0, False), ("depth_rmse", 1, True), ("depth_abs_rel", 2, False), ("depth_sq_rel", 3, False), ("depth_rmse_log", 4, True)):
        a, b = (got[k] ** 2, want[k] ** 2) if sq else (got[k], want[k])
        assert abs(a - b) <= wb[j] / n + 4 * np.spacing(b), k
    # the coarse level on request, another range; accumulation over two frames
    assert ev.evaluate_depth(out, gt["depth"], level=0, d_range=(1.0, 8.0)) == "depth_0"
    ev.evaluate_depth(out, gt["depth"], level=0, d_range=(1.0, 8.0))
    ws0, wc0, _ = sr.metrics32_64(N_(out["depth_0"]), N_(gt["depth"]), None, (1.0, 8.0))
    assert np.array_equal(N_(ev.depth_counts), 2 * wc0)
    two = ev.summarize()
    assert two["depth_n"] == 2 * wc0[0] and two["depth_d1"] == sr.summary(ws0, wc0)["depth_d1"]
