"""Cross-view reprojection on an MI355X: k_reproject (csrc/pnr_warp.hip) against tests/_warp_ref.py's float32 restatement of
the rule (include/pnr.h "cross-view reprojection"), BIT FOR BIT -- match codes, uv, the cross-view confusion matrix and the
five counters are integers or float32 words that must be equal, so there are no tolerances here.  tests/test_warp_ref.py
pins that restatement (closed forms, corrupted variants, float64) on the CPU."""
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _camera_ref as cr
import _warp_ref as wr
from panopticnerf_amd import Pinhole, camera, consistency, make_network, make_renderer, ops, synthetic
from panopticnerf_amd.evaluate import Evaluator

pytestmark = pytest.mark.gpu


def N_(t):
    return t.detach().cpu().numpy()


def _mask():
    m = np.ones((96, 96), bool)
    m[70:, :] = False
    m[10, 20] = False
    return m


CAMS = {"pinhole": Pinhole(40.0, 41.0, 31.5, 23.5, 64, 48), "pinhole_b": Pinhole(55.0, 54.0, 39.5, 19.5, 80, 40),
        "fisheye": synthetic.fisheye_camera(96 / 1400)[0], "fisheye_b": synthetic.fisheye_camera(64 / 1400, mask=None)[0],
        "fisheye_m": synthetic.fisheye_camera(96 / 1400, mask=_mask())[0]}
# source, target: all four model pairings, different sizes on the two sides, one camera with a user mask
PAIRINGS = {"pin_pin": ("pinhole", "pinhole_b"), "fish_fish": ("fisheye_m", "fisheye_b"), "fish_pin": ("fisheye", "pinhole"),
            "pin_fish": ("pinhole_b", "fisheye_m")}
POSE_PAIRS = {"near": (cr.pose(0.3, 0.0, (0.0, 1.55, 0.0)), cr.pose(0.35, -0.03, (0.3, 1.5, 0.4))),
              "turned": (cr.pose(1.2, 0.1, (-2.0, 1.0, 1.0)), cr.pose(0.6, -0.1, (0.5, 1.4, -1.0))),
              "far_opposed": (cr.POSES["oblique"], cr.pose(0.8, 0.35, (-12.0, 0.8, 40.0)))}


def words(cam):
    return (wr.PINHOLE, cam.intr) if cam.model == "pinhole" else (wr.FISHEYE, cam.cam)


def ref_view(cam, pose):
    m, w = words(cam)
    return (m, np.asarray(w, np.float32), np.asarray(pose, np.float32), cam.width, cam.height)


def scene(pairing, poses):
    """(cam_s, c2w_s, depth_s, cam_t, c2w_t, w2c_t, depth_t): both cameras inside a sphere, each depth image in its model's own
    convention, with a zero patch, one NaN, one Inf and one negative value; the target's also with an occluding slab (half the
    depth) and a band 4 % too far; a masked camera's depth is 0 under its mask, as render_view leaves it."""
    cs, ct = CAMS[PAIRINGS[pairing][0]], CAMS[PAIRINGS[pairing][1]]
    ca, cb = (np.asarray(p, np.float32) for p in POSE_PAIRS[poses])
    centre = (ca[:, 3].astype(np.float64) + cb[:, 3]) / 2 + np.array([1.0, -0.5, 2.0])
    out = []
    for cam, c2w in ((cs, ca), (ct, cb)):
        m, w = words(cam)
        d = wr.sphere_depth(m, np.asarray(w, np.float32), c2w, cam.width, cam.height, centre, 12.0)
        d[5:9, 11:15] = 0.0
        d[3, 4], d[3, 5], d[3, 6] = np.nan, np.inf, -1.5
        if getattr(cam, "mask", None) is not None:
            d[~N_(cam.mask).reshape(cam.height, cam.width)] = 0.0
        out.append(d)
    out[1][12:30, 20:38] *= 0.5
    out[1][:, 50:58] *= 1.04
    w2c = N_(camera.invert_pose(cb))
    return cs, ca, out[0], ct, cb, w2c, out[1]


def labels(seed, cam, n_classes):
    """labels in [-1, n_classes + 1]: -1 (ignore) and out-of-range values included"""
    return np.random.default_rng(seed).integers(-1, n_classes + 2, (cam.height, cam.width)).astype(np.int32)


def T(a, dev):
    return None if a is None else torch.as_tensor(a).to(dev)


def same_bits(got, want):
    return np.array_equal(N_(got).view(np.uint32), np.asarray(want, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 1: the main sweep
@pytest.mark.parametrize("poses", list(POSE_PAIRS))
@pytest.mark.parametrize("pairing", list(PAIRINGS))
def test_reproject_bit_for_bit(dev, pairing, poses):
    cs, ca, ds, ct, cb, w2c, dt = scene(pairing, poses)
    src, tgt = ref_view(cs, ca), ref_view(ct, w2c)
    npix = cs.width * cs.height
    g = np.random.default_rng(3)
    pix_lists = [None] + [g.integers(0, npix, R).astype(np.int32) for R in (1, 255, 4097)]       # unsorted, repeated
    seen_codes = set()
    for pix, with_dt in itertools.product(pix_lists, (True, False)):
        want = wr.reproject32(src, ds, tgt, dt if with_dt else None, pix=pix)
        for nc in ((1, 45, 128, 129) if pix is None else (45,)):
            ls, lt = labels(1, cs, nc), labels(2, ct, nc)
            wl = wr.reproject32(src, ds, tgt, dt if with_dt else None, pix=pix, label_src=ls, label_tgt=lt, n_classes=nc)
            assert np.array_equal(wl["match"], want["match"])
            got = ops.reproject(cs, ca, T(ds, dev), ct, w2c, T(dt, dev) if with_dt else None, pix=T(pix, dev), label_src=T(ls, dev),
                                label_tgt=T(lt, dev), n_classes=nc, want=("match", "uv", "agree", "stats"))
            what = (pairing, poses, None if pix is None else pix.size, with_dt, nc)
            assert got["match"].dtype == torch.int32 and got["agree"].dtype == torch.int64 and got["stats"].dtype == torch.int64
            assert np.array_equal(N_(got["match"]), want["match"]), what
            assert same_bits(got["uv"], want["uv"]), what
            assert np.array_equal(N_(got["agree"]), wl["agree"]), what
            assert np.array_equal(N_(got["stats"]), want["stats"]) and int(got["stats"].sum()) == want["match"].size, what
        if pix is None:
            seen_codes |= set(np.unique(np.minimum(want["match"], 0)).tolist())
            if with_dt:
                print("%s / %s: matched / -1 / -2 / -3 / -4 = %s, agree cells > 0: %d" % (pairing, poses, want["stats"].tolist(), int((wl["agree"] > 0).sum())))
    assert -1 in seen_codes and len(seen_codes) >= 2, seen_codes           # (the next test: every code occurs over the sweep)


def test_every_code_and_every_path_is_exercised_by_the_sweep():
    """the sweep above is not vacuous: over its cases every code occurs in numbers, the LDS histogram and the global-atomic
    path both count, and labels outside [0, n_classes) are dropped"""
    total = np.zeros(5, np.int64)
    for pairing, poses in itertools.product(PAIRINGS, POSE_PAIRS):
        cs, ca, ds, ct, cb, w2c, dt = scene(pairing, poses)
        out = wr.reproject32(ref_view(cs, ca), ds, ref_view(ct, w2c), dt, label_src=labels(1, cs, 129), label_tgt=labels(2, ct, 129), n_classes=129)
        total += out["stats"]
        assert out["agree"].sum() < out["stats"][0] or out["stats"][0] == 0
    print("sweep totals: matched / -1 / -2 / -3 / -4 =", total.tolist())
    assert (total > 200).all()


# ------------------------------------------------------------------------------------------------ 2: NULL outputs, canaries
def test_every_subset_of_outputs_with_canaries(dev):
    cs, ca, ds, ct, cb, w2c, dt = scene("fish_pin", "near")
    nc = 45
    ls, lt = labels(1, cs, nc), labels(2, ct, nc)
    g = np.random.default_rng(5)
    for pix in (None, g.integers(0, cs.width * cs.height, 255).astype(np.int32)):
        want = wr.reproject32(ref_view(cs, ca), ds, ref_view(ct, w2c), dt, pix=pix, label_src=ls, label_tgt=lt, n_classes=nc)
        R = want["match"].size
        args = dict(pix=T(pix, dev), label_src=T(ls, dev), label_tgt=T(lt, dev), n_classes=nc)
        for r in range(5):
            for names in itertools.combinations(("match", "uv", "agree", "stats"), r):
                mbuf = torch.full((R + 128,), -77, dtype=torch.int32, device=dev)
                ubuf = torch.full((2 * R + 128,), -77.0, dtype=torch.float32, device=dev)
                out = {}
                if "match" in names:
                    out["match"] = mbuf[64:64 + R]
                if "uv" in names:
                    out["uv"] = ubuf[64:64 + 2 * R].view(R, 2)
                got = ops.reproject(cs, ca, T(ds, dev), ct, w2c, T(dt, dev), want=names, out=out, **args)
                assert set(got) == set(names), names
                assert bool((mbuf[:64] == -77).all()) and bool((mbuf[64 + R:] == -77).all()) and bool((ubuf[:64] == -77).all()) and bool((ubuf[64 + 2 * R:] == -77).all())
                if "match" in names:
                    assert got["match"].data_ptr() == mbuf[64:].data_ptr() and np.array_equal(N_(got["match"]), want["match"])
                else:
                    assert bool((mbuf == -77).all())
                if "uv" in names:
                    assert got["uv"].data_ptr() == ubuf[64:].data_ptr() and same_bits(got["uv"], want["uv"])
                else:
                    assert bool((ubuf == -77.0).all())
                if "agree" in names:
                    assert np.array_equal(N_(got["agree"]), want["agree"])
                if "stats" in names:
                    assert np.array_equal(N_(got["stats"]), want["stats"])
    # no label images: match and stats alone; an empty pixel list is a no-op
    got = ops.reproject(cs, ca, T(ds, dev), ct, w2c, T(dt, dev), want=("match", "stats"))
    assert np.array_equal(N_(got["match"]), wr.reproject32(ref_view(cs, ca), ds, ref_view(ct, w2c), dt)["match"])
    e = ops.reproject(cs, ca, T(ds, dev), ct, w2c, T(dt, dev), pix=torch.zeros(0, dtype=torch.int32, device=dev), want=("match", "uv", "stats"))
    assert e["match"].shape == (0,) and e["uv"].shape == (0, 2) and int(e["stats"].sum()) == 0
    # pixel indices outside the source image have nothing to reproject (and read nothing)
    odd = torch.tensor([-1, cs.width * cs.height, 2 ** 31 - 1, -2 ** 31, 17], dtype=torch.int32, device=dev)
    got = ops.reproject(cs, ca, T(ds, dev), ct, w2c, T(dt, dev), pix=odd, want=("match", "stats"))
    assert N_(got["match"])[:4].tolist() == [-1] * 4 and int(got["stats"][1]) >= 4
    # dtype, contiguity and shape of tensors on the GPU
    with pytest.raises(TypeError, match="depth_src"):
        ops.reproject(cs, ca, T(ds, dev).double(), ct, w2c)
    with pytest.raises(TypeError, match="label_tgt"):
        ops.reproject(cs, ca, T(ds, dev), ct, w2c, label_src=T(ls, dev), label_tgt=T(lt, dev).long(), n_classes=nc)
    with pytest.raises(TypeError, match="pix"):
        ops.reproject(cs, ca, T(ds, dev), ct, w2c, pix=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="contiguous"):
        ops.reproject(cs, ca, T(np.ascontiguousarray(ds.T), dev).T, ct, w2c)
    with pytest.raises(ValueError, match=r"agree must be \(n_classes, n_classes\)"):
        ops.reproject(cs, ca, T(ds, dev), ct, w2c, label_src=T(ls, dev), label_tgt=T(lt, dev), n_classes=nc,
                      agree=torch.zeros((4, 4), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match=r"stats must be \(5,\)"):
        ops.reproject(cs, ca, T(ds, dev), ct, w2c, stats=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="out must be a contiguous"):
        ops.reproject(cs, ca, T(ds, dev), ct, w2c, out={"match": torch.zeros(7, dtype=torch.int32, device=dev)})
    with pytest.raises(ValueError, match="only 'match' and 'uv'"):
        ops.reproject(cs, ca, T(ds, dev), ct, w2c, out={"stats": torch.zeros(5, dtype=torch.int64, device=dev)})


# ------------------------------------------------------------------------------------------------ 3: accumulation, grid-stride
def test_accumulation_over_pairs_equals_the_sum_of_fresh_calls(dev):
    nc = 45
    agree = torch.zeros((nc, nc), dtype=torch.int64, device=dev)
    stats = torch.zeros(5, dtype=torch.int64, device=dev)
    fresh_a, fresh_s, want_a, want_s = 0, 0, 0, 0
    for pairing, poses in (("fish_pin", "near"), ("pin_fish", "turned"), ("fish_fish", "near")):
        cs, ca, ds, ct, cb, w2c, dt = scene(pairing, poses)
        ls, lt = labels(1, cs, nc), labels(2, ct, nc)
        args = (cs, ca, T(ds, dev), ct, w2c, T(dt, dev))
        kw = dict(label_src=T(ls, dev), label_tgt=T(lt, dev), n_classes=nc)
        got = ops.reproject(*args, agree=agree, stats=stats, want=(), **kw)
        assert got["agree"] is agree and got["stats"] is stats and set(got) == {"agree", "stats"}
        f = ops.reproject(*args, want=("agree", "stats"), **kw)
        fresh_a, fresh_s = fresh_a + f["agree"], fresh_s + f["stats"]
        w = wr.reproject32(ref_view(cs, ca), ds, ref_view(ct, w2c), dt, label_src=ls, label_tgt=lt, n_classes=nc)
        want_a, want_s = want_a + w["agree"], want_s + w["stats"]
    assert torch.equal(agree, fresh_a) and torch.equal(stats, fresh_s)
    assert np.array_equal(N_(agree), want_a) and np.array_equal(N_(stats), want_s) and want_a.sum() > 1000


def test_whole_benchmark_frame_grid_strides_and_equals_its_slices(dev):
    """1400 x 1400 fisheye -> 1408 x 376 pinhole: 1,960,000 source pixels on at most 256 CUs x 8 workgroups x 256 threads, so
    every thread takes 3 or 4 pixels; the frame launched whole must equal its slices launched one by one (match: the
    concatenation; agree, stats: the sum) on the LDS-histogram path and on the global-atomic path, and a strided subset of
    it the float32 reference."""
    fish = camera.Fisheye(*cr.KITTI_FISHEYE, 1400, 1400)
    pin = Pinhole(552.554261, 552.554261, 682.049453, 238.769549, 1408, 376)
    ca, cb = (np.asarray(p, np.float32) for p in POSE_PAIRS["near"])
    w2c = N_(camera.invert_pose(cb))
    npix = 1400 * 1400
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert npix >= 3 * cus * 8 * 256
    j, i = torch.meshgrid(torch.arange(1400, device=dev, dtype=torch.float32), torch.arange(1400, device=dev, dtype=torch.float32), indexing="ij")
    ds = (20.0 + 0.3 * torch.sin(i / 50.0) * torch.cos(j / 70.0)).contiguous()        # range: a rippled sphere around A
    ds[200:260, 300:420] = 0.0
    j, i = torch.meshgrid(torch.arange(376, device=dev, dtype=torch.float32), torch.arange(1408, device=dev, dtype=torch.float32), indexing="ij")
    x, y = (i - pin.intr[2]) / pin.intr[0], (j - pin.intr[3]) / pin.intr[1]
    dt = (20.0 / torch.sqrt(1.0 + x * x + y * y)).contiguous()                       # z-depth of a sphere around B, 0.5 m from A: the 2 % test passes and fails
    dt[100:300, 400:900] = 0.0
    g = torch.Generator().manual_seed(4)
    cuts = [0, 1, 500001, 1234567, npix]
    for nc in (45, 129):
        ls = torch.randint(-1, nc + 1, (1400, 1400), generator=g, dtype=torch.int32).to(dev)
        lt = torch.randint(-1, nc + 1, (376, 1408), generator=g, dtype=torch.int32).to(dev)
        kw = dict(label_src=ls, label_tgt=lt, n_classes=nc)
        whole = ops.reproject(fish, ca, ds, pin, w2c, dt, want=("match", "uv", "agree", "stats"), **kw)
        parts = [ops.reproject(fish, ca, ds, pin, w2c, dt, pix=torch.arange(a, b, dtype=torch.int32, device=dev), want=("match", "uv", "agree", "stats"), **kw)
                 for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(whole["match"], torch.cat([p["match"] for p in parts]))
        assert torch.equal(whole["uv"], torch.cat([p["uv"] for p in parts]))
        assert torch.equal(whole["agree"], sum(p["agree"] for p in parts)) and torch.equal(whole["stats"], sum(p["stats"] for p in parts))
        st = N_(whole["stats"])
        print("whole frame, %d classes: matched / -1 / -2 / -3 / -4 = %s, agree total %d" % (nc, st.tolist(), int(whole["agree"].sum())))
        assert st.sum() == npix and (st > 10000).all() and int(whole["agree"].sum()) > 10000
    sub = np.arange(0, npix, 97, dtype=np.int32)
    want = wr.reproject32(ref_view(fish, ca), N_(ds), ref_view(pin, w2c), N_(dt), pix=sub)
    assert np.array_equal(N_(whole["match"])[sub], want["match"]) and same_bits(whole["uv"][torch.as_tensor(sub).long().to(dev)], want["uv"])


# ------------------------------------------------------------------------------------------------ 4: stream capture
def test_reproject_replays_from_a_captured_graph(dev):
    """one stream, no parallel branches; host values (cameras, poses, tolerances) are baked into the capture, the depth image
    is read at replay"""
    cs, ca, ds, ct, cb, w2c, dt = scene("fish_pin", "near")
    nc = 45
    ls, lt = T(labels(1, cs, nc), dev), T(labels(2, ct, nc), dev)
    depth, dtgt = T(ds, dev), T(dt, dev)
    agree = torch.zeros((nc, nc), dtype=torch.int64, device=dev)
    stats = torch.zeros(5, dtype=torch.int64, device=dev)
    out = {"match": torch.empty(cs.width * cs.height, dtype=torch.int32, device=dev), "uv": torch.empty((cs.width * cs.height, 2), device=dev)}

    def call(d, a, s, o=None):
        return ops.reproject(cs, ca, d, ct, w2c, dtgt, label_src=ls, label_tgt=lt, n_classes=nc, agree=a, stats=s, want=("match", "uv"), out=o)

    call(depth, agree.clone(), stats.clone())                 # warm call: module loading is not capturable
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        call(depth, agree, stats, out)
    agree.zero_()
    stats.zero_()
    ea, es = torch.zeros_like(agree), torch.zeros_like(stats)
    seen = []
    for k in range(3):
        depth[20 + 10 * k:40 + 10 * k, :] *= 1.0 + 0.1 * (k + 1)          # edited in place between replays
        g.replay()
        torch.cuda.synchronize()
        eager = call(depth.clone(), ea, es)
        assert torch.equal(out["match"], eager["match"]) and torch.equal(out["uv"], eager["uv"])
        assert torch.equal(agree, ea) and torch.equal(stats, es)
        seen.append(out["match"].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and int(stats.sum()) == 3 * cs.width * cs.height


# ------------------------------------------------------------------------------------------------ 5: end to end
@pytest.fixture(scope="module")
def renderer(dev):
    cfg = NS(D=4, W=128, skips=[2], N_samples=32, N_importance=32, num_classes=5, num_instances=0, precision="bf16")
    torch.manual_seed(3)
    net = make_network(cfg).eval()
    synthetic.trained_like_(net, 0.3)
    return make_renderer(cfg, net.to(dev))


def _host_labels(out):
    lab = N_(out["semantic_1"]).argmax(-1).astype(np.int32)
    return np.where(N_(out["valid"]), lab, -1)


def _mc(agree):
    rows = agree.sum(1)
    with np.errstate(all="ignore"):
        return float(np.trace(agree) / agree.sum()), np.where(rows > 0, np.diag(agree) / np.maximum(rows, 1), np.nan)


@pytest.mark.parametrize("kind", ["pinhole", "fisheye_m", "mixed"])
def test_evaluate_pair_end_to_end(dev, renderer, kind):
    cam_a = CAMS["fisheye" if kind == "mixed" else kind]
    cam_b = CAMS["pinhole" if kind == "mixed" else kind]
    # the field is fog, not surfaces: its rendered depth follows the camera, so the pair stands 4 cm and 2 degrees apart
    # (a step of the 2 % depth test at the fog's few metres); how many pixels then match is printed, the assertions are
    # equality with the reference and that MC is defined (at least one matched pixel with labels on both sides)
    ca, cb = (torch.as_tensor(p, dtype=torch.float32) for p in (cr.pose(0.3, 0.0, (0.0, 1.55, 0.0)), cr.pose(0.33, -0.02, (0.03, 1.55, 0.02))))
    with torch.no_grad():
        oa = renderer.render_view(cam_a, ca, 0.5, 30.0)
        ob = renderer.render_view(cam_b, cb, 0.5, 30.0)
    ev = Evaluator(n_classes=5)
    res = ev.evaluate_pair(oa, (cam_a, ca), ob, (cam_b, cb))
    la, lb = _host_labels(oa), _host_labels(ob)
    assert np.array_equal(N_(res["semantic_label_a"]), la) and np.array_equal(N_(res["semantic_label_b"]), lb)
    va, vb = ref_view(cam_a, ca), ref_view(cam_b, cb)
    wa, wb = N_(camera.invert_pose(ca)), N_(camera.invert_pose(cb))
    ab = wr.reproject32(va, N_(oa["depth_1"]), ref_view(cam_b, wb), N_(ob["depth_1"]), label_src=la, label_tgt=lb, n_classes=5)
    ba = wr.reproject32(vb, N_(ob["depth_1"]), ref_view(cam_a, wa), N_(oa["depth_1"]), label_src=lb, label_tgt=la, n_classes=5)
    assert np.array_equal(N_(res["match_ab"]).reshape(-1), ab["match"]) and np.array_equal(N_(res["match_ba"]).reshape(-1), ba["match"])
    assert res["match_ab"].shape == (cam_a.height, cam_a.width) and res["match_ba"].shape == (cam_b.height, cam_b.width)
    agree_dev, stats_dev = N_(ev.mc_agree), N_(ev.mc_stats)
    got = ev.summarize()
    mc, per = _mc(ab["agree"] + ba["agree"])
    print("%s: mc = %.4f, stats %s" % (kind, got["mc"], got["mc_stats"]))
    assert np.array_equal(agree_dev, ab["agree"] + ba["agree"]) and np.array_equal(stats_dev, ab["stats"] + ba["stats"])
    assert got["mc"] == mc and got["mc_stats"] == (ab["stats"] + ba["stats"]).tolist() and int(agree_dev.sum()) > 0
    assert np.array_equal(np.asarray(got["mc_per_class"]), per, equal_nan=True)
    assert set(got) == {"mc", "mc_per_class", "mc_stats"} and ev.summarize() == {}
    # symmetric = the two one-way calls
    ev.evaluate_pair(oa, (cam_a, ca), ob, (cam_b, cb), symmetric=False)
    assert np.array_equal(N_(ev.mc_agree), ab["agree"]) and np.array_equal(N_(ev.mc_stats), ab["stats"])
    one = ev.evaluate_pair(ob, (cam_b, cb), oa, (cam_a, ca), symmetric=False)
    assert set(one) == {"semantic_label_a", "semantic_label_b", "match_ab"} and torch.equal(one["match_ab"], res["match_ba"])
    two = ev.summarize()
    assert two["mc"] == got["mc"] and two["mc_stats"] == got["mc_stats"] and set(two) == set(got)
    assert np.array_equal(np.asarray(two["mc_per_class"]), per, equal_nan=True)           # (NaN for unseen classes: no list ==)
    # consistency.reproject is the same match; warp carries B's label map into A's pixel grid
    m = consistency.reproject((cam_a, ca, oa), (cam_b, cb, ob))
    assert torch.equal(m, res["match_ab"])
    warped = N_(consistency.warp(res["semantic_label_b"], m, fill=-1))
    assert np.array_equal(warped, np.where(ab["match"] >= 0, lb.reshape(-1)[np.maximum(ab["match"], 0)], -1).reshape(cam_a.height, cam_a.width))
    wrgb = consistency.warp(ob["rgb_1"], m)
    assert wrgb.shape == (cam_a.height, cam_a.width, 3) and torch.equal(wrgb[m >= 0], ob["rgb_1"].reshape(-1, 3)[m[m >= 0].long()]) and not wrgb[m < 0].any()
    free = consistency.reproject((cam_a, ca, oa), (cam_b, cb, ob), occlusion=False)
    assert np.array_equal(N_(free).reshape(-1), wr.reproject32(va, N_(oa["depth_1"]), ref_view(cam_b, wb), None)["match"])
    # the same view against itself: every pixel with depth lands on itself, nothing is occluded, MC is 1
    ev.evaluate_pair(oa, (cam_a, ca), oa, (cam_a, ca))
    same = ev.summarize()
    seen = int(((oa["depth_1"] > 0) & torch.isfinite(oa["depth_1"]) & oa["valid"]).sum())
    assert same["mc"] == 1.0 and same["mc_stats"] == [2 * seen, 2 * (cam_a.width * cam_a.height - seen), 0, 0, 0] and seen > 0
