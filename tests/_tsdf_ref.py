"""CPU references of depth fusion (csrc/pnr_fusion.hip; the rule is include/pnr.h "depth fusion").

(a) integrate_loops: the rule as plain Python loops over lattice points and frames on numpy.float32 scalars -- the text of the
    header, step by step.
(b) integrate32: the same in vectorised numpy float32, in the rule's operation order.  k_tsdf_integrate must equal it bit for
    bit.  Both take the projection (steps 2, 3 and the depth e of step 5) from _splat_ref.points32, already pinned bit for bit
    against the kernels for all three camera models.  `variant`: deliberately WRONG rules (test_tsdf_ref.py: its checks can fail).
(c) integrate64: the rule in float64 on _splat_ref.splat64, with the per-point quantities a float32 comparison needs.
(d) unobserved_near / filter_mesh: numpy restatement of fusion.extract's filter.

A frame is a dict: view = (model, cam, w2c, width, height) as in _splat_ref, depth (H, W) float32 or None, rgb (H, W, 3) uint8 or
None, sem / inst (H, W) int16 or None.  A state is a dict of flat arrays over the lattice: tsdf, weight (float32), optionally
rgb (N, 3), rgb_weight (float32) and label, conf (int32).
"""
import numpy as np

import _camera_ref as cr
import _mesh_ref as mr
import _pano_ref as pr
import _splat_ref as sr
import _warp_ref as wr

PINHOLE, FISHEYE, EQUIRECT = sr.PINHOLE, sr.FISHEYE, sr.EQUIRECT
VARIANTS = ("sign", "ge", "weight_first", "trunc_pixel", "z_fisheye", "vote_replace")
CONF_MAX = 2 ** 30
FMAX = sr.FMAX
U32 = sr.U32


def frame(view, depth=None, rgb=None, sem=None, inst=None):
    m, cam, w2c, w, h = view
    img = lambda a, dt, tail=(): None if a is None else np.ascontiguousarray(np.asarray(a, dt).reshape((h, w) + tail))
    return {"view": (m, np.asarray(cam, np.float32), np.asarray(w2c, np.float32).reshape(3, 4), int(w), int(h)),
            "depth": img(depth, np.float32), "rgb": img(rgb, np.uint8, (3,)), "sem": img(sem, np.int16), "inst": img(inst, np.int16)}


def points(lo, hi, res):
    """(N, 3) float32 lattice positions in flat order n = (iz res_y + iy) res_x + ix; res = (res_x, res_y, res_z)"""
    x, y, z = mr.positions(lo, hi, res)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)


def new_state(n, color=False, labels=False, dtype=np.float32):
    st = {"tsdf": np.zeros(n, dtype), "weight": np.zeros(n, dtype)}
    if color:
        st.update(rgb=np.zeros((n, 3), dtype), rgb_weight=np.zeros(n, dtype))
    if labels:
        st.update(label=np.full(n, -1, np.int32), conf=np.zeros(n, np.int32))
    return st


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def pack(sem, inst):
    """the vote's key of a (sem >= 0, inst) pair, as a Python integer"""
    return (int(sem) << 16) | (int(inst) & 0xFFFF)


def unpack(label):
    """(sem, inst) int32 arrays of packed keys; -1 where nothing voted"""
    lab = np.asarray(label, np.int32)
    inst = (((lab & 0xFFFF) ^ 0x8000) - 0x8000).astype(np.int32)
    return np.where(lab < 0, -1, lab >> 16).astype(np.int32), np.where(lab < 0, -1, inst).astype(np.int32)


def _projection(fr, pts, variant):
    """steps 2, 3 and e of step 5 from _splat_ref.points32: seen (N) bool, q (N) int64 (0 where not seen), e (N) float32"""
    m, _, _, w, _ = fr["view"]
    pv = "trunc" if variant == "trunc_pixel" else ("range_pinhole" if variant == "z_fisheye" and m != PINHOLE else None)
    _, left, iu, iv, e = sr.points32(fr["view"], pts, variant=pv)
    seen = ~left
    return seen, np.where(seen, iv * w + iu, 0), e


# ------------------------------------------------------------------------------------------------ analytic scenes
SPHERE = ((0.2, 1.0, 0.5), 6.0)             # centre, radius: every camera below stands inside it
_FISH = tuple(v * s for v, s in zip(cr.KITTI_FISHEYE, (1, 1, 1, 80 / 1400, 80 / 1400, 80 / 1400, 80 / 1400)))
# name -> (model, cam, c2w float64, width, height): the three models x two poses at small images
CAMERAS = {
    "pinhole_a": (PINHOLE, (60.0, 61.0, 47.5, 31.5), cr.pose(0.1, 0.05, (0.0, 1.2, 0.3)), 96, 64),
    "pinhole_b": (PINHOLE, (45.0, 44.0, 50.2, 29.1), cr.pose(-0.5, -0.1, (1.5, 0.6, 1.0)), 96, 64),
    "fisheye_a": (FISHEYE, _FISH, cr.pose(0.0, 0.0, (0.3, 1.0, 0.0)), 80, 80),
    "fisheye_b": (FISHEYE, _FISH, cr.pose(0.7, 0.2, (-1.0, 1.5, 0.8)), 80, 80),
    "equirect_a": (EQUIRECT, pr.equirect_cam(128, 64), cr.pose(0.3, 0.0, (0.0, 1.07, 0.5)), 128, 64),
    "equirect_b": (EQUIRECT, pr.equirect_cam(128, 64, lon=(100.0, 250.0), lat=(60.0, -40.0)),       # its columns cross +-180 degrees
                   cr.pose(3.0, 0.1, (0.8, 0.7, -0.4)), 128, 64),
}
EQUIRECT_B_DEGREES = {"lon": (100.0, 250.0), "lat": (60.0, -40.0)}          # camera.Equirect's arguments for equirect_b


def w2c32(c2w):
    """camera.invert_pose in numpy: float64 inverse of the float32 pose, rounded once"""
    return cr.invert_pose(np.asarray(c2w, np.float32).astype(np.float64)).astype(np.float32)


def sphere_frame(name, seed=0, depth=True, rgb=True, sem=True, inst=True, w2c=None, sphere=SPHERE, n_sem=5, n_inst=300, c2w=None):
    """A frame of CAMERAS[name] looking at SPHERE from inside: analytic depth in the model's convention (0 outside a fisheye
    lens), random uint8 colour, random int16 labels in [-1, n_sem) and [-1, n_inst).  c2w: another pose than the camera's own;
    w2c: the float32 world-to-camera to use (the device table's row), else w2c32 of the pose."""
    m, cam, own, w, h = CAMERAS[name]
    c2w = np.asarray(own if c2w is None else c2w, np.float32)
    g = np.random.default_rng(seed)
    d = pr.sphere_depth(cam, c2w, w, h, *sphere) if m == EQUIRECT else wr.sphere_depth(m, cam, c2w, w, h, *sphere)
    lab = lambda hi: g.integers(-1, hi, (h, w)).astype(np.int16)
    view = (m, np.asarray(cam, np.float32), w2c32(c2w) if w2c is None else np.asarray(w2c, np.float32).reshape(3, 4), w, h)
    fr = frame(view, d if depth else None, g.integers(0, 256, (h, w, 3)).astype(np.uint8) if rgb else None,
               lab(n_sem) if sem else None, lab(n_inst) if inst else None)
    fr["c2w"], fr["name"] = c2w, name
    return fr


# ------------------------------------------------------------------------------------------------ (a) loops
def integrate_loops(state, frames, pts, trunc, max_depth=np.inf, w_max=np.inf, f0=0, f1=None, variant=None):
    """The rule, one lattice point and one frame at a time, on numpy.float32 scalars.  Returns a new state."""
    assert variant is None or variant in VARIANTS
    f = np.float32
    st = copy_state(state)
    trunc, max_depth, w_max, one = f(trunc), f(max_depth), f(w_max), f(1.0)
    f1 = len(frames) if f1 is None else f1
    proj = {k: _projection(frames[k], pts, variant) for k in range(f0, f1) if frames[k]["depth"] is not None}
    with np.errstate(all="ignore"):
        for n in range(len(pts)):
            t, w = st["tsdf"][n], st["weight"][n]
            for k in range(f0, f1):
                fr = frames[k]
                if fr["depth"] is None:                                             # 1
                    continue
                seen, q, e = proj[k]
                if not seen[n]:                                                     # 2
                    continue
                p = int(q[n])                                                       # 3
                d = fr["depth"].reshape(-1)[p]                                      # 4
                if not (d > 0 and np.abs(d) <= FMAX and d <= max_depth):
                    continue
                s = (d - e[n]) if variant == "sign" else (e[n] - d)                 # 5
                if (s >= trunc) if variant == "ge" else (s > trunc):
                    continue
                phi = f(-1.0) if s < -trunc else s / trunc                          # 6
                if variant == "weight_first":
                    w = w + one
                t = (t * w + phi) / (w + one)                                       # 7
                if variant != "weight_first":
                    w = min(w + one, w_max)
                if not s >= -trunc:
                    continue
                if "rgb" in st and fr["rgb"] is not None:                           # 8
                    cw = st["rgb_weight"][n]
                    for c in range(3):
                        st["rgb"][n, c] = (st["rgb"][n, c] * cw + f(fr["rgb"].reshape(-1, 3)[p, c])) / (cw + one)
                    st["rgb_weight"][n] = min(cw + one, w_max)
                if "label" in st and fr["sem"] is not None:                         # 9
                    ls = int(fr["sem"].reshape(-1)[p])
                    if ls >= 0:
                        key = pack(ls, fr["inst"].reshape(-1)[p] if fr["inst"] is not None else -1)
                        lab, cf = int(st["label"][n]), int(st["conf"][n])
                        if lab == key:
                            cf = min(cf + 1, CONF_MAX)
                        elif cf == 0 or (variant == "vote_replace" and cf == 1):
                            lab, cf = key, 1
                        else:
                            cf -= 1
                        st["label"][n], st["conf"][n] = lab, cf
            st["tsdf"][n], st["weight"][n] = t, w
    return st


# ------------------------------------------------------------------------------------------------ (b) vectorised float32
def integrate32(state, frames, pts, trunc, max_depth=np.inf, w_max=np.inf, f0=0, f1=None, variant=None):
    """The rule in vectorised numpy float32 (k_tsdf_integrate, bit for bit).  Returns a new state."""
    assert variant is None or variant in VARIANTS
    f = np.float32
    st = copy_state(state)
    trunc, max_depth, w_max, one = f(trunc), f(max_depth), f(w_max), f(1.0)
    f1 = len(frames) if f1 is None else f1
    with np.errstate(all="ignore"):
        for k in range(f0, f1):
            fr = frames[k]
            if fr["depth"] is None:
                continue
            seen, q, e = _projection(fr, pts, variant)
            d = fr["depth"].reshape(-1)[q]
            s = ((d - e) if variant == "sign" else (e - d)).astype(f)
            use = seen & (d > 0) & (np.abs(d) <= FMAX) & (d <= max_depth) & ~((s >= trunc) if variant == "ge" else (s > trunc))
            phi = np.where(s < -trunc, f(-1.0), s / trunc).astype(f)
            t, w = st["tsdf"], st["weight"]
            if variant == "weight_first":
                w1 = (w + one).astype(f)
                t_new, w_new = ((t * w1 + phi) / (w1 + one)).astype(f), w1
            else:
                t_new, w_new = ((t * w + phi) / (w + one)).astype(f), np.minimum(w + one, w_max).astype(f)
            st["tsdf"], st["weight"] = np.where(use, t_new, t), np.where(use, w_new, w)
            band = use & (s >= -trunc)
            if "rgb" in st and fr["rgb"] is not None:
                cw = st["rgb_weight"]
                byte = fr["rgb"].reshape(-1, 3)[q].astype(f)
                c_new = ((st["rgb"] * cw[:, None] + byte) / (cw + one)[:, None]).astype(f)
                st["rgb"] = np.where(band[:, None], c_new, st["rgb"])
                st["rgb_weight"] = np.where(band, np.minimum(cw + one, w_max).astype(f), cw)
            if "label" in st and fr["sem"] is not None:
                ls = fr["sem"].reshape(-1)[q].astype(np.int64)
                li = (fr["inst"].reshape(-1)[q] if fr["inst"] is not None else np.full(len(q), -1)).astype(np.int64)
                key = ((np.maximum(ls, 0) << 16) | (li & 0xFFFF)).astype(np.int32)
                vote = band & (ls >= 0)
                lab, cf = st["label"], st["conf"]
                same = vote & (lab == key)
                take = vote & ~same & ((cf == 0) | ((cf == 1) if variant == "vote_replace" else False))
                drop = vote & ~same & ~take
                st["label"] = np.where(take, key, lab).astype(np.int32)
                st["conf"] = np.where(same, np.minimum(cf + 1, CONF_MAX), np.where(take, 1, np.where(drop, cf - 1, cf))).astype(np.int32)
    return st


# ------------------------------------------------------------------------------------------------ (c) float64
def integrate64(state, frames, pts, trunc, max_depth=np.inf, w_max=np.inf, f0=0, f1=None):
    """The rule in float64 (the inputs -- points, poses, cameras, depth, trunc -- are the same float32 numbers).  Returns
    (state, per-frame list of dicts: ref64 of _splat_ref.splat64, q, d, s, use, band) for the frames that have depth."""
    st = copy_state(state)
    trunc, max_depth, w_max = float(np.float32(trunc)), float(np.float32(max_depth)), float(np.float32(w_max))
    f1 = len(frames) if f1 is None else f1
    info = []
    with np.errstate(all="ignore"):
        for k in range(f0, f1):
            fr = frames[k]
            if fr["depth"] is None:
                continue
            w_ = fr["view"][3]
            ref = sr.splat64(fr["view"], pts)
            seen = ref["inside"]
            q = np.where(seen, ref["iv"] * w_ + ref["iu"], 0)
            d = fr["depth"].reshape(-1)[q].astype(np.float64)
            s = ref["e"] - d
            use = seen & (d > 0) & np.isfinite(d) & (d <= max_depth) & ~(s > trunc)
            phi = np.where(s < -trunc, -1.0, s / trunc)
            t, w = st["tsdf"], st["weight"]
            st["tsdf"] = np.where(use, (t * w + phi) / (w + 1.0), t)
            st["weight"] = np.where(use, np.minimum(w + 1.0, w_max), w)
            band = use & (s >= -trunc)
            if "rgb" in st and fr["rgb"] is not None:
                cw = st["rgb_weight"]
                byte = fr["rgb"].reshape(-1, 3)[q].astype(np.float64)
                st["rgb"] = np.where(band[:, None], (st["rgb"] * cw[:, None] + byte) / (cw + 1.0)[:, None], st["rgb"])
                st["rgb_weight"] = np.where(band, np.minimum(cw + 1.0, w_max), cw)
            info.append({"frame": k, "ref": ref, "q": q, "d": d, "s": s, "use": use, "band": band, "phi": phi})
    return st, info


def single_frame_bound(fr, pts, trunc, info, inflate=1.0 + 2.0 ** -4):
    """For ONE frame fused into an empty volume (tsdf = phi exactly: (0 * 0 + phi) / 1): (bound (N) on |tsdf32 - tsdf64|,
    excluded (N) bool).  With de = _splat_ref.project_bound's bound on the depth e and u = 2^-24:
        s = e - d commits u |s| on top of de (d is the same float32 number);  phi = s / trunc commits u |phi| (trunc is exact):
        |phi32 - phi64| <= (de + u |s|) / trunc + u |phi|.
    Excluded: the points whose pixel choice may differ (_splat_ref.near_decision: u + 0.5 or v + 0.5 within its bound of an
    integer, or the domain decision itself in doubt) and the points whose s lies within de + u |s| of +trunc or -trunc (seen or
    hidden, clamped or not, are decided there).  Points both evaluations leave out of the view decide nothing."""
    trunc = float(np.float32(trunc))
    du, dv, de = sr.project_bound(fr["view"], pts)
    ref, s, phi = info["ref"], info["s"], info["phi"]
    with np.errstate(all="ignore"):
        out = sr.near_decision(ref, fr["view"], 0.0, np.inf, du, dv, de, inflate)
        ds = de + U32 * np.abs(s)
        known = ref["inside"] & (info["d"] > 0) & np.isfinite(info["d"])
        for lim in (trunc, -trunc):
            out |= known & ~(np.abs(s - lim) > inflate * ds)
        bound = inflate * (ds / trunc + U32 * np.abs(phi))
    return np.where(info["use"], bound, 0.0), out


# ------------------------------------------------------------------------------------------------ (d) the extract filter
def unobserved_near(observed):
    """(res_z, res_y, res_x) bool: points with an unobserved lattice point within +-1 per axis; a loop over the 27 offsets"""
    obs = np.asarray(observed, bool)
    rz, ry, rx = obs.shape
    pad = np.ones((rz + 2, ry + 2, rx + 2), bool)             # beyond the lattice: does not count
    pad[1:-1, 1:-1, 1:-1] = obs
    bad = np.zeros(obs.shape, bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                bad |= ~pad[dz:dz + rz, dy:dy + ry, dx:dx + rx]
    return bad


def filter_mesh(verts, faces, src, observed):
    """fusion.filter_mesh in numpy, with explicit loops over faces and vertices: (verts, faces, src, index)"""
    bad = unobserved_near(observed).reshape(-1)
    keep_v = [not bad[int(s)] for s in src]
    kept_faces = [tuple(int(v) for v in fc) for fc in faces if all(keep_v[int(v)] for v in fc)]
    used = sorted({v for fc in kept_faces for v in fc})
    new = {v: i for i, v in enumerate(used)}
    index = np.asarray(used, np.int64)
    out_faces = np.asarray([[new[v] for v in fc] for fc in kept_faces], np.int32).reshape(-1, 3)
    return np.asarray(verts)[index], out_faces, np.asarray(src)[index], index
