"""The panoramic camera on an MI355X: k_gen_rays_equirect, k_project_points / k_reproject / k_sample_batch with model word 3
against tests/_pano_ref.py's float32 restatement of the rule (include/pnr.h "cameras"), BIT FOR BIT -- the rule's sine, cosine
and arctangent are written-out float32 arithmetic, so rays, uv, ranges, match codes and counters must be equal and there are no
tolerances -- then the layers above: FrameSet, Renderer.render_view, consistency / Evaluator.evaluate_pair, stream capture.
tests/test_pano_ref.py pins the restatement (exact values, closed forms, corrupted variants, float64) on the CPU.

The two figures that are not equalities: the round trip pixel -> ray -> point -> projection on the device within 1e-3 px (the
condition of test_pano_ref.py; measured there 1.2e-4 px), and the cross-camera depth convention within twice what the oracle
gives for the same comparison (the bound of test_gpu_camera.py's convention test)."""
import ctypes
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _batch_ref as br
import _camera_ref as cr
import _pano_ref as pr
import _warp_ref as wr
from oracle import torch_oracle as to
from panopticnerf_amd import ConvexSet, Equirect, FrameSet, Pinhole, _lib, camera, consistency, make_network, make_renderer, ops, synthetic
from panopticnerf_amd.evaluate import Evaluator

pytestmark = pytest.mark.gpu

F = lambda *v: (ctypes.c_float * len(v))(*v)
CAMS = {"full": Equirect(64, 32), "odd": Equirect(37, 19), "seam": Equirect(40, 20, lon=(150.0, 260.0), lat=(40.0, -75.0)),
        "mirror": Equirect(40, 20, lon=(100.0, -120.0), lat=(-60.0, 60.0)), "frame": Equirect(128, 64), "full_b": Equirect(80, 40),
        "pinhole": Pinhole(40.0, 41.0, 31.5, 23.5, 64, 48), "fisheye": synthetic.fisheye_camera(96 / 1400)[0]}
EQUI = ("full", "odd", "seam", "mirror")


def N_(t):
    return t.detach().cpu().numpy()


def T(a, dev):
    return None if a is None else torch.as_tensor(a).to(dev)


def same_bits(got, want):
    return np.array_equal(N_(got).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))


def words(cam):
    return {"pinhole": lambda: (pr.PINHOLE, cam.intr), "fisheye": lambda: (pr.FISHEYE, cam.cam), "equirect": lambda: (pr.EQUIRECT, cam.cam)}[cam.model]()


def ref_view(cam, pose):
    m, w = words(cam)
    return (m, np.asarray(w, np.float32), np.asarray(pose, np.float32), cam.width, cam.height)


# ------------------------------------------------------------------------------------------------ 1: rays
@pytest.mark.parametrize("pname", list(cr.POSES))
@pytest.mark.parametrize("name", EQUI)
def test_rays_whole_frames_bit_for_bit(dev, name, pname):
    cam, c2w = CAMS[name], cr.POSES[pname]
    rays = cam.rays(c2w, 0.5, 100.0, device=dev)
    want = pr.unproject32(cam.cam, c2w, cam.width, cam.height, 0.5, 100.0)
    assert rays.shape == (cam.width * cam.height, 8) and rays.dtype == torch.float32
    assert same_bits(rays, want)
    assert torch.equal(cam.valid_pix(dev), torch.arange(cam.width * cam.height, dtype=torch.int32, device=dev)) and cam.valid_pix(dev) is cam.valid_pix(dev)
    d = N_(rays)[:, 3:6].astype(np.float64)
    assert np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max() <= 4 * pr.U32


def _raw_rays(dev, cam, c2w, pix, R):
    """pnr_gen_rays_equirect into the middle of a caller-owned buffer: (rays, the buffer)"""
    buf = torch.full((R * 8 + 128,), -77.0, device=dev)
    rc = _lib.load().pnr_gen_rays_equirect(F(*cam.cam), F(*np.asarray(c2w, np.float32).reshape(-1).tolist()), cam.width, cam.height, 0.25, 80.0,
                                           ops._p(pix), R, ctypes.c_void_p(buf.data_ptr() + 256), ops._stream())
    assert rc == 0, _lib.load().pnr_last_error()
    return buf[64:64 + R * 8].view(R, 8), buf


@pytest.mark.parametrize("R", [1, 255, 4097])
def test_rays_of_pixel_lists_with_canaries(dev, R):
    cam = CAMS["frame"]
    g = np.random.default_rng(R)
    pix = g.integers(0, cam.width * cam.height, R).astype(np.int32)            # unsorted, repeated
    pix[:1] = cam.width * cam.height - 1
    for c2w in cr.POSES.values():
        want = pr.unproject32(cam.cam, c2w, cam.width, cam.height, 0.25, 80.0, pix=pix)
        rays, buf = _raw_rays(dev, cam, c2w, T(pix, dev), R)
        assert same_bits(rays, want)
        assert bool((buf[:64] == -77.0).all()) and bool((buf[64 + R * 8:] == -77.0).all())
        assert torch.equal(cam.rays(c2w, 0.25, 80.0, pix=T(pix, dev)), rays)
    whole, buf = _raw_rays(dev, CAMS["odd"], cr.POSES["oblique"], None, 37 * 19)
    assert same_bits(whole, pr.unproject32(CAMS["odd"].cam, cr.POSES["oblique"], 37, 19, 0.25, 80.0))
    assert bool((buf[:64] == -77.0).all()) and bool((buf[64 + 37 * 19 * 8:] == -77.0).all())
    e = cam.rays(cr.POSES["identity"], 0.5, 100.0, pix=torch.zeros(0, dtype=torch.int32, device=dev))
    assert e.shape == (0, 8)
    with pytest.raises(TypeError, match="int32"):
        cam.rays(cr.POSES["identity"], 0.5, 100.0, pix=torch.zeros(4, dtype=torch.int64, device=dev))


def test_rays_of_a_large_frame_grid_stride_and_equal_their_slices(dev):
    """2048 x 1024 = 2,097,152 rays on at most 256 CUs x 8 workgroups x 256 threads: every thread takes at least 3 rays"""
    cam, c2w = Equirect(2048, 1024), cr.POSES["sideways"]
    npix = 2048 * 1024
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert npix >= 3 * cus * 8 * 256
    whole = cam.rays(c2w, 0.5, 100.0, device=dev)
    cuts = [0, 1, 500001, 1234567, npix]
    parts = [cam.rays(c2w, 0.5, 100.0, pix=torch.arange(a, b, dtype=torch.int32, device=dev)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(whole, torch.cat(parts))
    sub = np.arange(0, npix, 97, dtype=np.int32)
    assert same_bits(whole[T(sub, dev).long()], pr.unproject32(cam.cam, c2w, 2048, 1024, 0.5, 100.0, pix=sub))


# ------------------------------------------------------------------------------------------------ 2: projection
def _points(seed, P, cam, c2w):
    """points all around a camera at c2w; then the special ones: on the seam (either side and on it), both poles, the axis
    x = z = 0, the camera centre, NaN / Inf, a range that overflows, tiny offsets"""
    g = np.random.default_rng(seed)
    d = g.normal(0, 1, (P, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    p = c2w[:, 3] + d * np.exp(g.uniform(np.log(0.05), np.log(200.0), (P, 1)))
    Rm, o = c2w[:, :3], c2w[:, 3]
    lon_seam = (cam.cam[0] + 1.0) * np.pi if cam.cam[0] != -1.0 else np.pi              # the image's left edge (or +-180 degrees)
    special = [[0.0, 0.0, -2.0], [1e-3, 0.0, -2.0], [-1e-3, 0.0, -2.0], [-0.0, 0.0, -2.0],
               [np.sin(lon_seam), 0.0, np.cos(lon_seam)], [np.sin(lon_seam) * 3, 0.4, np.cos(lon_seam) * 3],
               [0.0, -3.0, 0.0], [0.0, 3.0, 0.0], [0.0, -1e-3, 0.0], [1e-9, -3.0, 1e-9], [-1e-9, 3.0, 0.0],
               [0.0, 0.0, 0.0], [1e-30, 0.0, 0.0], [0.0, 1e-30, 0.0], [0.0, 0.0, 5.0], [5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]]
    p[:len(special)] = o + np.asarray(special) @ Rm.T
    p = p.astype(np.float32)
    k = len(special)
    p[k:k + 6] = [[np.nan, 0, 1], [0, np.nan, 1], [np.inf, 0, 1], [0, -np.inf, 0], [1e30, -1e30, 1e30], [3e38, 3e38, 3e38]]
    return p, k + 6


@pytest.mark.parametrize("pname", list(cr.POSES))
def test_projection_bit_for_bit(dev, pname):
    c2w = cr.POSES[pname]
    w2c = cr.invert_pose(c2w).astype(np.float32)
    for name in EQUI:
        cam = CAMS[name]
        pts, n_special = _points(5, 100003, cam, c2w)
        uv, rng, valid = (N_(x) for x in cam.project(T(pts, dev), w2c))
        wuv, wrng, wvalid = pr.project32(cam.cam, w2c, cam.width, cam.height, pts)
        assert np.isfinite(uv).all()                                                    # never NaN, whatever the point
        assert np.array_equal(valid, wvalid != 0), name
        assert np.array_equal(uv.view(np.uint32), wuv.view(np.uint32)), name
        nan = np.isnan(wrng)
        assert np.array_equal(np.isnan(rng), nan) and np.array_equal(rng[~nan].view(np.uint32), wrng[~nan].view(np.uint32))
        assert nan.sum() >= 2 and np.isinf(wrng).sum() >= 2 and not valid[np.isnan(wrng) | np.isinf(wrng)].any()
        if name in ("full", "odd"):
            assert valid[n_special:].all()                  # a full sphere sees every point but its own centre ...
            assert (uv[n_special:, 0] >= -0.5).all() and (uv[n_special:, 0] < cam.width - 0.5).all()
        else:
            assert 0.02 < valid.mean() < 0.9
    if pname == "identity":         # ... -z with x = +-0 is longitude +1: wrapped back onto the left edge of pixel 0
        uv, rng, valid = (N_(x) for x in CAMS["full"].project(T(pts, dev), w2c))
        assert uv[0].tolist() == [-0.5, 15.5] and uv[3].tolist() == [-0.5, 15.5] and valid[0] and abs(uv[1, 0] - 63.5) < 0.01 and abs(uv[2, 0] + 0.5) < 0.01
        assert uv[6].tolist()[1] == -0.5 and valid[6] and not valid[7] and uv[7].tolist()[1] == 31.5 and not valid[11] and uv[11].tolist() == [0.0, 0.0]
    e = CAMS["full"].project(torch.zeros((0, 3), device=dev), w2c)
    assert e[0].shape == (0, 2) and e[1].shape == (0,) and e[2].shape == (0,)


def test_projection_every_subset_of_outputs_with_canaries(dev):
    cam, c2w = CAMS["seam"], cr.POSES["sideways"]
    w2c = cr.invert_pose(c2w).astype(np.float32)
    pts, _ = _points(9, 4097, cam, c2w)
    P = len(pts)
    wuv, wrng, wvalid = pr.project32(cam.cam, w2c, cam.width, cam.height, pts)
    tp = T(pts, dev)
    lib = _lib.load()
    for r in range(4):
        for names in itertools.combinations(("uv", "range", "valid"), r):
            ubuf = torch.full((2 * P + 128,), -77.0, device=dev)
            rbuf = torch.full((P + 128,), -77.0, device=dev)
            vbuf = torch.full((P + 128,), 201, dtype=torch.uint8, device=dev)
            ptr = lambda b, on, off: ctypes.c_void_p(b.data_ptr() + off if on else 0)
            rc = lib.pnr_project_points(3, F(*cam.cam), F(*w2c.reshape(-1).tolist()), cam.width, cam.height, ops._p(tp), P,
                                        ptr(ubuf, "uv" in names, 256), ptr(rbuf, "range" in names, 256), ptr(vbuf, "valid" in names, 64), ops._stream())
            assert rc == 0, lib.pnr_last_error()
            for buf, n, canary in ((ubuf, 2 * P, -77.0), (rbuf, P, -77.0), (vbuf, P, 201)):
                assert bool((buf[:64] == canary).all()) and bool((buf[64 + n:] == canary).all()), names
            assert same_bits(ubuf[64:64 + 2 * P].view(P, 2), wuv) if "uv" in names else bool((ubuf == -77.0).all())
            fin = ~np.isnan(wrng)
            assert same_bits(rbuf[64:64 + P][T(fin, dev)], wrng[fin]) if "range" in names else bool((rbuf == -77.0).all())
            assert np.array_equal(N_(vbuf[64:64 + P]), wvalid) if "valid" in names else bool((vbuf == 201).all())


def test_round_trip_on_the_device_returns_the_pixel(dev):
    """identity pose, the benchmark panorama: the condition of tests/test_pano_ref.py (1e-3 px; why the identity pose: there)"""
    cam, _ = synthetic.equirect_camera()
    assert (cam.width, cam.height) == (1408, 704)
    c2w = cr.POSES["identity"]
    i, j = cr.pixel_grid(cam.width, cam.height)
    rays = cam.rays(c2w, 0.5, 100.0, device=dev)
    for t in (0.5, 7.3, 100.0):
        pts = ops.points(rays, torch.full((rays.shape[0], 1), t, device=dev)).reshape(-1, 3)        # o + d * t (pnr_points)
        uv, rng, ok = (N_(x) for x in cam.project(pts, cr.invert_pose(c2w)))
        e = np.maximum(np.abs(uv[:, 0] - i), np.abs(uv[:, 1] - j)).max()
        print("round trip t = %5.1f: max %.3e px" % (t, e))
        assert ok.all() and e <= 1e-3
        assert np.abs(rng / np.float32(t) - 1.0).max() < 8 * pr.U32


# ------------------------------------------------------------------------------------------------ 3: reprojection
PAIRINGS = {"equi_equi": ("full", "full_b"), "equi_seam": ("full_b", "seam"), "mirror_equi": ("mirror", "full"), "equi_pin": ("full", "pinhole"),
            "equi_fish": ("full_b", "fisheye"), "pin_equi": ("pinhole", "full"), "fish_equi": ("fisheye", "full_b")}
POSE_PAIRS = {"near": (cr.pose(0.3, 0.0, (0.0, 1.55, 0.0)), cr.pose(0.35, -0.03, (0.3, 1.5, 0.4))),
              "yawed": (cr.pose(0.1, 0.0, (0.0, 1.55, 0.0)), cr.pose(0.1 + 0.97 * np.pi, 0.02, (0.2, 1.5, -0.3)))}


def _depth(cam, c2w, centre, radius):
    m, w = words(cam)
    if m == pr.EQUIRECT:
        return pr.sphere_depth(w, c2w, cam.width, cam.height, centre, radius)
    return wr.sphere_depth(m, np.asarray(w, np.float32), c2w, cam.width, cam.height, centre, radius)


def scene(pairing, poses):
    """as test_gpu_reproject.scene: both cameras inside a sphere, each depth image in its model's convention, with a zero patch,
    NaN, Inf and a negative value on both sides, an occluding slab and a band 4 % too far in the target"""
    cs, ct = CAMS[PAIRINGS[pairing][0]], CAMS[PAIRINGS[pairing][1]]
    ca, cb = (np.asarray(p, np.float32) for p in POSE_PAIRS[poses])
    centre = (ca[:, 3].astype(np.float64) + cb[:, 3]) / 2 + np.array([1.0, -0.5, 2.0])
    out = []
    for cam, c2w in ((cs, ca), (ct, cb)):
        d = _depth(cam, c2w, centre, 12.0)
        d[5:9, 11:15] = 0.0
        d[3, 4], d[3, 5], d[3, 6] = np.nan, np.inf, -1.5
        out.append(d)
    h, w = out[1].shape
    out[1][h // 4:h // 2, w // 3:w // 2] *= 0.5
    out[1][:, w - 10:w - 4] *= 1.04
    return cs, ca, out[0], ct, cb, N_(camera.invert_pose(cb)), out[1]


def labels(seed, cam, n_classes):
    return np.random.default_rng(seed).integers(-1, n_classes + 2, (cam.height, cam.width)).astype(np.int32)


@pytest.mark.parametrize("poses", list(POSE_PAIRS))
@pytest.mark.parametrize("pairing", list(PAIRINGS))
def test_reproject_bit_for_bit(dev, pairing, poses):
    cs, ca, ds, ct, cb, w2c, dt = scene(pairing, poses)
    src, tgt = ref_view(cs, ca), ref_view(ct, w2c)
    npix = cs.width * cs.height
    g = np.random.default_rng(3)
    pix_lists = [None] + [g.integers(-2, npix + 2, R).astype(np.int32) for R in (1, 255, 4097)]       # unsorted, repeated, some outside
    for pix, with_dt in itertools.product(pix_lists, (True, False)):
        want = pr.reproject32(src, ds, tgt, dt if with_dt else None, pix=pix)
        for nc in ((1, 45, 129) if pix is None else (45,)):
            ls, lt = labels(1, cs, nc), labels(2, ct, nc)
            wl = pr.reproject32(src, ds, tgt, dt if with_dt else None, pix=pix, label_src=ls, label_tgt=lt, n_classes=nc)
            got = ops.reproject(cs, ca, T(ds, dev), ct, w2c, T(dt, dev) if with_dt else None, pix=T(pix, dev), label_src=T(ls, dev),
                                label_tgt=T(lt, dev), n_classes=nc, want=("match", "uv", "agree", "stats"))
            what = (pairing, poses, None if pix is None else pix.size, with_dt, nc)
            assert np.array_equal(N_(got["match"]), want["match"]), what
            assert same_bits(got["uv"], want["uv"]), what
            assert np.array_equal(N_(got["agree"]), wl["agree"]), what
            assert np.array_equal(N_(got["stats"]), want["stats"]) and int(got["stats"].sum()) == want["match"].size, what
        if pix is None and with_dt:
            st = want["stats"]
            print("%s / %s: matched / -1 / -2 / -3 / -4 = %s" % (pairing, poses, st.tolist()))
            assert st[0] > 100 and st[1] >= 19 and st[4] > 0 and (st[3] > 0 or cs.model == "pinhole"), st     # (the pinhole's narrow field misses the target's zero patch)
            assert (st[2] == 0) == (PAIRINGS[pairing][1] in ("full", "full_b"))         # nothing leaves a full sphere
            if ct.model == "equirect" and PAIRINGS[pairing][1] != "seam" and poses == "yawed":
                cols = want["match"][want["match"] >= 0] % ct.width
                assert (cols == 0).any() and (cols == ct.width - 1).any()              # matches on both sides of the seam
    if PAIRINGS[pairing][1] == "seam":            # the partial range crossing +-180 degrees is matched on both sides of it
        uv = pr.reproject32(src, ds, tgt, None)
        lam = CAMS["seam"].cam[0] + (uv["uv"][uv["match"] >= 0, 0] + 0.5) * CAMS["seam"].cam[1]
        assert (lam < 1.0).any() and (lam > 1.0).any()


def test_a_view_onto_itself_matches_every_pixel_to_itself(dev):
    for name, pname in itertools.product(("full", "odd", "seam", "mirror", "full_b"), ("identity", "oblique")):
        cam, c2w = CAMS[name], np.asarray(cr.POSES[pname], np.float32)
        n = cam.width * cam.height
        depth = torch.full((cam.height, cam.width), 5.0, device=dev)
        got = ops.reproject(cam, c2w, depth, cam, N_(camera.invert_pose(c2w)), depth, want=("match", "stats"))
        assert torch.equal(got["match"], torch.arange(n, dtype=torch.int32, device=dev)), (name, pname)
        assert got["stats"].tolist() == [n, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 4: FrameSet
SEED = 77
KEYS = (("rays", "rays"), ("rgb", "rgb"), ("depth", "depth"), ("pseudo_label", "sem"), ("instance_label", "inst"), ("frame", "frame"),
        ("pix", "pix"))


def _images(g, H, W, C=19, K=12):
    return {"rgb": torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8), "depth": torch.rand(H, W, generator=g) * 60 - 5,
            "pseudo_label": torch.randint(-1, C, (H, W), generator=g), "instance_label": torch.randint(-1, K, (H, W), generator=g)}


@pytest.fixture(scope="module")
def mixed(dev):
    """pinhole 64 x 48 (everything), fisheye 96 x 96 (depth), full panorama 64 x 32 (everything), seam-crossing panorama (rgb)"""
    g = torch.Generator().manual_seed(3)
    fs, ref = FrameSet(dev, capacity=8, seed=SEED), []
    for name, c2w, near, far, keys in (("pinhole", cr.pose(0.2, 0.05, (1.0, 1.55, -3.0)), 0.5, 100.0, None),
                                       ("fisheye", synthetic.fisheye_camera(96 / 1400)[1].numpy(), 0.25, 80.0, ("rgb", "depth")),
                                       ("full", cr.POSES["oblique"], 0.5, 60.0, None),
                                       ("seam", cr.pose(-2.0, 0.0, (-4.0, 1.4, 12.0)), 1.0, 120.0, ("rgb",))):
        cam = CAMS[name]
        im = _images(g, cam.height, cam.width)
        im = im if keys is None else {k: im[k] for k in keys}
        fs.add(cam, c2w, near, far, im["rgb"], im.get("depth"), im.get("pseudo_label"), im.get("instance_label"))
        host = [N_(im["rgb"])] + [None if im.get(k) is None else N_(im[k]) for k in ("depth", "pseudo_label", "instance_label")]
        c2w32 = N_(torch.as_tensor(c2w, dtype=torch.float32))
        if cam.model == "equirect":
            ref.append(pr.ref_frame(cam.cam, cam.width, cam.height, c2w32, near, far, *host))
        else:
            ref.append(br.ref_frame(cam.model, cam.intr if cam.model == "pinhole" else cam.cam, cam.width, cam.height, c2w32, near, far, *host))
    assert fs.n_pixels == br.cum_of(ref)[-1] and fs.frames[2]["pix"] is None and fs.frames[3]["n_valid"] == 800
    return fs, ref


@pytest.mark.parametrize("mode", ["pooled", "frame"])
@pytest.mark.parametrize("R", [1, 255, 4097])
def test_frameset_batches_equal_the_reference(dev, mixed, R, mode):
    fs, ref = mixed
    picked = set()
    for off in range(10, 18):
        fs.rng_state.copy_(torch.tensor([SEED, off], dtype=torch.int64))
        batch = fs.sample(R, mode)
        want = pr.sample(ref, SEED, off, R, 0 if mode == "pooled" else 1)
        for k, n in KEYS:
            got = N_(batch[k]).reshape(want[n].shape)
            assert got.dtype == want[n].dtype, (k, got.dtype)
            a, b = np.ascontiguousarray(got), np.ascontiguousarray(want[n])
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b), (R, mode, off, k)
        picked |= set(want["frame"].tolist())
    assert {2, 3} & picked, picked                # a panoramic frame was drawn from
    if R >= 255:
        assert picked == {0, 1, 2, 3}, picked


def test_frame_batch_of_a_panorama_is_the_cameras_frame(dev, mixed):
    fs, ref = mixed
    for i in (2, 3):
        fr = fs.frames[i]
        b = fs.frame_batch(i)
        cam = fr["camera"]
        n = cam.width * cam.height
        assert torch.equal(b["rays"][0], cam.rays(fr["c2w"], fr["near"], fr["far"], device=dev))          # what render_view renders
        assert same_bits(b["rays"][0], pr.rays_of(ref[i], np.arange(n)))
        assert torch.equal(b["pix"], torch.arange(n, dtype=torch.int32, device=dev)) and b["rgb"].shape == (1, n, 3)
        assert np.array_equal(N_(b["pseudo_label"][0]), ref[i]["sem"].reshape(-1) if ref[i]["sem"] is not None else np.full(n, -1))


# ------------------------------------------------------------------------------------------------ 5: render_view
def test_render_view_of_a_panorama_equals_the_plain_render(dev):
    cfg = synthetic.baseline_cfg(5, precision="bf16")
    torch.manual_seed(0)
    net = make_network(cfg).eval()
    synthetic.trained_like_(net)
    rend = make_renderer(cfg, net.to(dev))
    cam, c2w = synthetic.equirect_camera(64 / 1408)
    assert (cam.width, cam.height) == (64, 32)
    box, ids = synthetic.random_boxes(32, 45, 32)
    bx, bi = box.to(dev), ids.to(dev)
    cs = ConvexSet.from_boxes(box, ids)
    with torch.no_grad():
        rays = cam.rays(c2w, 0.5, 100.0, device=dev)
        for kw, batch in ((dict(bbox=bx, bbox_ids=bi), dict(bbox=bx, bbox_ids=bi)), (dict(prims=cs), None)):
            out = rend.render_view(cam, c2w, 0.5, 100.0, **kw)
            ref = rend.render({"rays": rays, **(cs.batch() if batch is None else batch)})
            assert out["valid"].dtype == torch.bool and out["valid"].shape == (32, 64) and bool(out["valid"].all())
            assert set(out) == set(ref) | {"valid"}
            for k, v in ref.items():
                assert torch.equal(out[k], v.reshape(32, 64, *v.shape[1:])), (sorted(kw), k)
            assert float(out["fix_semantic_1"].sum()) > 0.1                 # the prior is seen
    assert same_bits(rays, pr.unproject32(cam.cam, N_(c2w), 64, 32, 0.5, 100.0))
    assert 0.4 < (N_(rays[:, 3:6]) @ N_(c2w)[:, 2] < 0).mean() < 0.6        # half the panorama looks backwards


# ------------------------------------------------------------------------------------------------ 6: one convention
def _cross_camera_figures(raysE, depthE, semE, depthP, semP, c2w, project):
    """as test_gpu_camera._cross_camera_figures: panorama pixels whose ray falls inside the pinhole image -- the point o + range d
    projected into the pinhole image, its z-depth (range times d_cam.z) against the pinhole depth at the nearest pixel"""
    pts = raysE[:, :3] + raysE[:, 3:6] * depthE[:, None]
    uv, rng, ok = project(pts)
    ok = ok != 0
    u = np.floor(uv[ok, 0] + 0.5).astype(np.int64)
    v = np.floor(uv[ok, 1] + 0.5).astype(np.int64)
    zc = raysE[ok, 3:6].astype(np.float64) @ np.asarray(c2w, dtype=np.float64)[:, 2]
    rel = np.abs(rng[ok] * zc - depthP[v, u]) / depthP[v, u]
    agree = (semE[ok].argmax(-1) == semP[v, u].argmax(-1)).mean()
    return int(ok.sum()), float(rel.mean()), float(agree)


def test_panorama_and_pinhole_share_axes_signs_and_depth_convention(dev):
    """A pinhole and a panoramic camera at ONE pose, fp32, the field of test_gpu_camera's convention test.  (a) the point o + t d
    of a panorama ray, projected into the pinhole image, lands on a pixel whose own ray is within half a pixel diagonal of it;
    (b) depth_pinhole = depth_equirect * d_cam.z and the semantic argmax at the nearest pixel, within twice what
    torch_oracle.render_rays gives for the same comparison on the same rays (the bound of that test)."""
    cfg = NS(D=4, W=128, skips=[2], N_samples=32, N_importance=32, num_classes=19, num_instances=0, precision="fp32")
    torch.manual_seed(3)
    net = make_network(cfg).eval()
    synthetic.trained_like_(net, 0.3)
    rend = make_renderer(cfg, net.to(dev))
    _, c2w = synthetic.fisheye_camera(96 / 1400, yaw=0.3, origin=(0.5, 1.55, -1.0))
    equi = Equirect(80, 64, lon=(-40.0, 40.0), lat=(32.0, -32.0))           # one degree a pixel, about the pinhole's field
    pin = Pinhole(40.0, 40.0, 31.5, 23.5, 64, 48)
    w2c = cr.invert_pose(c2w.numpy())
    with torch.no_grad():
        outE = rend.render_view(equi, c2w, 0.5, 30.0)
        outP = rend.render_view(pin, c2w, 0.5, 30.0)
        raysE = equi.rays(c2w, 0.5, 30.0, device=dev)
        raysP = pin.rays(c2w, 0.5, 30.0, device=dev)
    rE, rP = N_(raysE), N_(raysP).reshape(48, 64, 8)
    half_diag = np.degrees(np.arctan(0.5 * np.sqrt(2.0) / 40.0))
    for t in (0.5, 7.0):
        uv, _, ok = (N_(x) for x in pin.project(ops.points(raysE, torch.full((rE.shape[0], 1), t, device=dev)).reshape(-1, 3), w2c))
        u, v = np.floor(uv[ok, 0] + 0.5).astype(np.int64), np.floor(uv[ok, 1] + 0.5).astype(np.int64)
        dp = rP[v, u, 3:6].astype(np.float64)
        cosang = (dp * rE[ok, 3:6]).sum(-1) / np.linalg.norm(dp, axis=-1)
        worst = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))).max()
        print("cross-camera geometry t = %.1f: %d panorama rays inside the pinhole image, worst angle %.3f deg (half a pixel diagonal: %.3f)"
              % (t, int(ok.sum()), worst, half_diag))
        assert ok.sum() > 1000 and worst <= half_diag * 1.001
    gpu_project = lambda pts: tuple(N_(x) for x in pin.project(torch.as_tensor(pts).to(dev), w2c))
    got = _cross_camera_figures(rE, N_(outE["depth_1"]).reshape(-1), N_(outE["semantic_1"]).reshape(80 * 64, -1),
                                N_(outP["depth_1"]), N_(outP["semantic_1"]), c2w.numpy(), gpu_project)
    params = {"coarse": {k: v.detach().cpu() for k, v in net.nerf_0.state_dict().items()},
              "fine": {k: v.detach().cpu() for k, v in net.nerf_1.state_dict().items()}}
    oc = to.mlp_config(D=4, W=128, skips=(2,), n_sem=19, n_inst=0)
    with torch.no_grad():
        oE = to.render_rays(params, oc, raysE.cpu(), 32, 32)
        oP = to.render_rays(params, oc, raysP.cpu(), 32, 32)
    cpu_project = lambda pts: cr.project32(cr.PINHOLE, pin.intr, w2c, 64, 48, pts)
    want = _cross_camera_figures(rE, oE["depth_1"].numpy(), oE["semantic_1"].numpy(), oP["depth_1"].numpy().reshape(48, 64),
                                 oP["semantic_1"].numpy().reshape(48, 64, -1), c2w.numpy(), cpu_project)
    print("cross-camera maps: GPU %d pixels, mean relative depth difference %.3e, argmax agreement %.4f; oracle %d, %.3e, %.4f" % (got + want))
    assert got[0] > 1000 and want[0] > 1000
    assert got[1] <= 2.0 * want[1]
    assert 1.0 - got[2] <= 2.0 * (1.0 - want[2])


# ------------------------------------------------------------------------------------------------ 7: stream capture
def test_rays_projection_and_reprojection_replay_from_a_captured_graph(dev):
    cam, tgt = CAMS["frame"], CAMS["fisheye"]
    c2w = np.asarray(cr.POSES["oblique"], np.float32)
    w2c = cr.invert_pose(c2w).astype(np.float32)
    w2c_t = N_(camera.invert_pose(cr.pose(-2.1, 0.3, (-12.3, 0.8, 40.0))))
    n = cam.width * cam.height
    g0 = torch.Generator().manual_seed(2)
    pix_a = torch.randint(0, n, (5000,), generator=g0, dtype=torch.int32).to(dev)
    pix_b = torch.randint(0, n, (5000,), generator=g0, dtype=torch.int32).to(dev)
    static_pix = pix_a.clone()
    depth = torch.full((cam.height, cam.width), 6.0, device=dev)
    dtgt = torch.full((96, 96), 6.0, device=dev)
    stats = torch.zeros(5, dtype=torch.int64, device=dev)

    def chain(p, d, s):
        rays = cam.rays(c2w, 0.5, 100.0, pix=p)
        pts = ops.points(rays, rays[:, 7:8].contiguous()).reshape(-1, 3)              # o + far * d, on the same stream
        m = ops.reproject(cam, c2w, d, tgt, w2c_t, dtgt, pix=p, stats=s, want=("match", "uv"))
        back = ops.reproject(tgt, N_(camera.invert_pose(w2c_t)), dtgt, cam, w2c, d, want=("match",))
        return (rays,) + tuple(cam.project(pts, w2c)) + (m["match"], m["uv"], back["match"])

    chain(static_pix, depth, stats.clone())               # warm call: module loading is not capturable
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        static_out = chain(static_pix, depth, stats)
    stats.zero_()
    static_pix.copy_(pix_b)
    depth[10:30, :] *= 1.3                                # edited in place: read at replay
    g.replay()
    torch.cuda.synchronize()
    got = [v.clone() for v in static_out]
    es = torch.zeros_like(stats)
    ref = chain(pix_b, depth.clone(), es)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert torch.equal(stats, es) and int(stats.sum()) == 5000 and int(stats[0]) > 100
    assert not torch.equal(got[0], chain(pix_a, depth, es)[0])


# ------------------------------------------------------------------------------------------------ 8: end to end
def _mc(agree):
    rows = agree.sum(1)
    with np.errstate(all="ignore"):
        return float(np.trace(agree) / agree.sum()), np.where(rows > 0, np.diag(agree) / np.maximum(rows, 1), np.nan)


def test_evaluate_pair_on_two_rendered_panoramas(dev):
    cfg = NS(D=4, W=128, skips=[2], N_samples=32, N_importance=32, num_classes=5, num_instances=0, precision="bf16")
    torch.manual_seed(3)
    net = make_network(cfg).eval()
    synthetic.trained_like_(net, 0.3)
    rend = make_renderer(cfg, net.to(dev))
    cam_a, cam_b = CAMS["full"], CAMS["full_b"]
    # (fog, not surfaces: 4 cm and 2 degrees apart, as test_gpu_reproject's end-to-end test)
    ca, cb = (torch.as_tensor(p, dtype=torch.float32) for p in (cr.pose(0.3, 0.0, (0.0, 1.55, 0.0)), cr.pose(0.33, -0.02, (0.03, 1.55, 0.02))))
    with torch.no_grad():
        oa = rend.render_view(cam_a, ca, 0.5, 30.0)
        ob = rend.render_view(cam_b, cb, 0.5, 30.0)
    assert bool(oa["valid"].all()) and oa["depth_1"].shape == (32, 64)
    ev = Evaluator(n_classes=5)
    res = ev.evaluate_pair(oa, (cam_a, ca), ob, (cam_b, cb))
    la, lb = (N_(o["semantic_1"]).argmax(-1).astype(np.int32) for o in (oa, ob))
    assert np.array_equal(N_(res["semantic_label_a"]), la) and np.array_equal(N_(res["semantic_label_b"]), lb)
    wa, wb = N_(camera.invert_pose(ca)), N_(camera.invert_pose(cb))
    ab = pr.reproject32(ref_view(cam_a, ca), N_(oa["depth_1"]), ref_view(cam_b, wb), N_(ob["depth_1"]), label_src=la, label_tgt=lb, n_classes=5)
    ba = pr.reproject32(ref_view(cam_b, cb), N_(ob["depth_1"]), ref_view(cam_a, wa), N_(oa["depth_1"]), label_src=lb, label_tgt=la, n_classes=5)
    assert np.array_equal(N_(res["match_ab"]).reshape(-1), ab["match"]) and np.array_equal(N_(res["match_ba"]).reshape(-1), ba["match"])
    assert np.array_equal(N_(ev.mc_agree), ab["agree"] + ba["agree"]) and np.array_equal(N_(ev.mc_stats), ab["stats"] + ba["stats"])
    got = ev.summarize()
    mc, per = _mc(ab["agree"] + ba["agree"])
    print("panorama pair: mc = %.4f, stats %s" % (got["mc"], got["mc_stats"]))
    assert got["mc"] == mc and got["mc_stats"] == (ab["stats"] + ba["stats"]).tolist() and int((ab["agree"] + ba["agree"]).sum()) > 0
    assert np.array_equal(np.asarray(got["mc_per_class"]), per, equal_nan=True)
    m = consistency.reproject((cam_a, ca, oa), (cam_b, cb, ob))
    assert torch.equal(m, res["match_ab"])
    warped = N_(consistency.warp(res["semantic_label_b"], m, fill=-1))
    assert np.array_equal(warped, np.where(ab["match"] >= 0, lb.reshape(-1)[np.maximum(ab["match"], 0)], -1).reshape(32, 64))
    # a panorama against itself: every pixel with depth lands on itself, MC is 1
    ev.evaluate_pair(oa, (cam_a, ca), oa, (cam_a, ca))
    same = ev.summarize()
    seen = int(((oa["depth_1"] > 0) & torch.isfinite(oa["depth_1"])).sum())
    assert same["mc"] == 1.0 and same["mc_stats"] == [2 * seen, 2 * (64 * 32 - seen), 0, 0, 0] and seen > 0
