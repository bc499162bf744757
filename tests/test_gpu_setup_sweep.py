"""The per-ray preamble (panopticnerf_amd/csrc/pnr_sampling.hip: k_stratified, k_points, k_sample_labels, k_bbox_hits,
k_restrict_rays, k_embed and the fused k_ray_setup; COVERAGE.md rows a3, a4, a8) against the C oracle BIT FOR BIT -- outputs
compared as uint32 / int32 words, NaNs by position only -- at every sample count, around every tile edge of the fused kernel,
on degenerate rays and boxes, and across three trips of every grid-stride loop.  tests/test_setup_ref.py (CPU) holds the C oracle
to the float64 references of tests/_setup_ref.py inside derived bounds; test_frame_rays_against_float64 below repeats that
comparison on the kernels' own output, so the figures of the table are the device's.

Every call goes through the C entry point.  All outputs of a call live in ONE buffer pre-filled with a canary word, 64 words of
guard around each: every case checks that the guards are intact and that no canary is left inside an output.

Measured on an MI355X (PNR_SWEEP_REPORT=<file.json> writes the figures), against float64 on the same float32 inputs:

  quantity                             bound (tests/_setup_ref.py)                        worst error   worst / bound
  hit depths t_in, t_out               5 u (O + e + |t| D) / |dl| at the binding axis     1.08e-4       0.368
  z, [near, far] and hull, linear      5 u (|near| + |far|);  23 u (..) with jitter       1.13e-5       0.380
  z, lindisp                           (z^2 delta + u z) / (1 - delta z);  3 max + 8 u z  8.69e-6       0.402
  embed bands k < 10                   TRIG_BOUND = 2.78e-7                               6.87e-8       0.247
  embed bands 10 <= k < 16             TRIG_BOUND = 2.78e-7                               6.70e-8       0.241

(hits and z: test_frame_rays_against_float64, depths up to 100; bands: test_embed_every_band_count_against_float64, arguments up
to 150 * 2^15.)  The device's sinf / cosf keep their accuracy on bands 10 .. 15, so those bands are held to the bound measured
on bands < 10.

Found by this file: the C oracle took fminf / fmaxf from the host's libm, which answers min(-0, +0) by operand order where the
device's v_min_f32 orders -0 below +0 -- on the edge rays below 9 words of hit_t and 20 of z differed in the sign of a zero.  The
rule is now written in include/pnr.h ("a8: min / max") and the oracle spells it out (pnro_fminf / pnro_fmaxf)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _mlp32_ref as m32
import _setup_ref as sr
from oracle import c_oracle as co
from panopticnerf_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

CANARY = np.int32(-1515870811)          # 0xA5A5A5A5: as a float -2.9e-16, never a depth; as an int never a label or a count
GUARD = 64                              # words around every output (256 bytes: every output stays 16-byte aligned)

_REPORT = os.environ.get("PNR_SWEEP_REPORT")
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _REPORT:
        with open(_REPORT, "w") as f:
            json.dump({k: _WORST[k] for k in sorted(_WORST)}, f, indent=1)


def _note(key, value):
    _WORST[key] = max(_WORST.get(key, 0.0), float(value))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def put(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Arena:
    """the outputs of one case inside one guarded device buffer: name -> number of 32-bit words"""

    def __init__(self, dev, **words):
        self.off, at = {}, GUARD
        for k, n in words.items():
            self.off[k] = (at, int(n))
            at += (int(n) + GUARD + 63) // 64 * 64
        self.buf = torch.full((at,), int(CANARY), dtype=torch.int32, device=dev)

    def ptr(self, k):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * self.off[k][0])

    def view(self, k, dtype=torch.float32):
        o, n = self.off[k]
        return self.buf[o:o + n].view(dtype)

    def read(self, unwritten=()):
        """(name -> int32 words as numpy, problems): guards intact, every output word written"""
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        guard = np.ones(h.size, bool)
        out, bad = {}, []
        for k, (o, n) in self.off.items():
            guard[o:o + n] = False
            out[k] = h[o:o + n].copy()
            if k not in unwritten and (out[k] == CANARY).any():
                bad.append(f"{k}: {int((out[k] == CANARY).sum())} words never written")
            if k in unwritten and (out[k] != CANARY).any():
                bad.append(f"{k}: written although not asked for")
        if (h[guard] != CANARY).any():
            bad.append(f"guard touched at words {np.flatnonzero(guard & (h != CANARY))[:8]}")
        return out, bad


def diff(got, ref, what):
    """'' when the words of got are ref's bit for bit (NaNs: by position only), else a message"""
    ref = np.ascontiguousarray(ref)
    g = got.reshape(-1)
    if g.size != ref.size:
        return f"{what}: {g.size} words against {ref.size}"
    if ref.dtype == np.float32:
        gf, rf = g.view(np.float32), ref.reshape(-1)
        gn, rn = np.isnan(gf), np.isnan(rf)
        ne = (gn != rn) | (~gn & ~rn & (g.view(np.uint32) != rf.view(np.uint32)))
    else:
        assert ref.dtype == np.int32
        gf, rf = g.view(np.int32), ref.reshape(-1)
        ne = gf != rf
    if ne.any():
        i = int(np.flatnonzero(ne)[0])
        return f"{what}: {int(ne.sum())} of {ne.size} words differ, first at {i}: kernel {gf[i]!r} oracle {rf[i]!r}"
    return ""


def check(bad, *msgs):
    bad += [m for m in msgs if m]


# ------------------------------------------------------------------------------------------------------------------ inputs
def ray_pool(n, seed=0):
    """n pinhole rays of the synthetic camera with their own near / far"""
    rays = synthetic.camera_rays(origin=(0.3, -0.2, 0.1))
    rays = rays[:: rays.shape[0] // n][:n].numpy().copy()
    rng = np.random.default_rng(seed)
    rays[:, 6] = rng.uniform(0.2, 2.0, n)
    rays[:, 7] = rng.uniform(20.0, 120.0, n)
    return rays


def big_boxes(M, seed=5, scale=6.0):
    """a seeded table of boxes large enough that a street ray crosses more of them than a short list holds"""
    if M == 0:
        return np.zeros((0, 15), np.float32), np.zeros((0, 2), np.int32)
    box, ids = synthetic.random_boxes(M, 45, 32, seed=seed)
    box, ids = box.numpy().copy(), ids.numpy().copy()
    box[:, 12:15] *= scale
    return box, ids


POOL = ray_pool(4099)
TRAND = np.random.default_rng(77).random(1000 * 257).astype(np.float32)
TRAND[5], TRAND[6] = 0.0, np.float32(1.0 - 2.0 ** -24)
_HITS = {}


def oracle_hits(R, M, mh):
    key = (R, M, mh)
    if key not in _HITS:
        box, ids = big_boxes(M)
        _HITS[key] = co.bbox_hits(POOL[:R], box, mh)
    return _HITS[key]


# --------------------------------------------------------------------------------------------------- the C entry points
def call_stratified(lib, d_rays, R, N, lindisp, d_tr, z_ptr):
    _lib.check(lib.pnr_stratified(_p(d_rays), R, N, int(lindisp), _p(d_tr), z_ptr, _stream()), "pnr_stratified")


def call_points(lib, d_rays, z_ptr, R, N, pts_ptr):
    _lib.check(lib.pnr_points(_p(d_rays), z_ptr, R, N, pts_ptr, _stream()), "pnr_points")


def call_labels(lib, z_ptr, R, N, ht, hb, hc, mh, d_ids, ls, li):
    _lib.check(lib.pnr_sample_labels(z_ptr, R, N, ht, hb, hc, mh, _p(d_ids), ls, li, _stream()), "pnr_sample_labels")


def call_bbox(lib, d_rays, R, d_box, M, mh, ht, hb, hc):
    _lib.check(lib.pnr_bbox_hits(_p(d_rays), R, _p(d_box), M, mh, ht, hb, hc, _stream()), "pnr_bbox_hits")


def call_restrict(lib, d_rays, R, ht, hc, mh, out):
    _lib.check(lib.pnr_restrict_rays(_p(d_rays), R, ht, hc, mh, out, _stream()), "pnr_restrict_rays")


def call_setup(lib, d_rays, R, d_box, M, mh, d_ids, N, lindisp, d_tr, hull, ar, labels=True):
    null = ctypes.c_void_p(0)
    _lib.check(lib.pnr_ray_setup(_p(d_rays), R, _p(d_box), M, mh, _p(d_ids), N, int(lindisp), _p(d_tr), int(hull), ar.ptr("ht"),
                                 ar.ptr("hb"), ar.ptr("hc"), ar.ptr("z"), ar.ptr("ls") if labels else null,
                                 ar.ptr("li") if labels else null, _stream()), "pnr_ray_setup")


def setup_arena(dev, R, N, mh, **more):
    return Arena(dev, ht=R * mh * 2, hb=R * mh, hc=R, z=R * N, ls=R * N, li=R * N, **more)


def oracle_setup(rays, box, ids, mh, N, lindisp, tr, hull):
    """the preamble stage by stage through the C oracle"""
    ht, hb, hc = co.bbox_hits(rays, box, mh)
    use = co.restrict_rays(rays, ht, hc) if hull else rays
    z = co.stratified(use, N, lindisp, tr)
    ls, li = co.sample_labels(z, ht, hb, hc, ids) if len(ids) else (np.full(z.shape, -1, np.int32),) * 2
    return dict(ht=ht, hb=hb, hc=hc, z=z, ls=ls, li=li, rays=use)


def run_setup(dev, rays, box, ids, mh, N, lindisp, tr, hull, labels=True):
    lib = _lib.load()
    R = rays.shape[0]
    ar = setup_arena(dev, R, N, mh)
    keep = [put(dev, rays), put(dev, box) if len(box) else None, put(dev, ids) if len(ids) else None, put(dev, tr)]
    call_setup(lib, keep[0], R, keep[1], box.shape[0], mh, keep[2], N, lindisp, keep[3], hull, ar, labels)
    return ar.read(unwritten=() if labels else ("ls", "li"))


def run_separate(dev, rays, box, ids, mh, N, lindisp, tr, hull):
    """the same through the four separate entry points, chained on the device"""
    lib = _lib.load()
    R = rays.shape[0]
    ar = setup_arena(dev, R, N, mh, rays=R * 8)
    d_rays, d_box, d_ids, d_tr = put(dev, rays), put(dev, box) if len(box) else None, put(dev, ids) if len(ids) else None, put(dev, tr)
    call_bbox(lib, d_rays, R, d_box, box.shape[0], mh, ar.ptr("ht"), ar.ptr("hb"), ar.ptr("hc"))
    call_restrict(lib, d_rays, R, ar.ptr("ht"), ar.ptr("hc"), mh, ar.ptr("rays"))
    _lib.check(lib.pnr_stratified(ar.ptr("rays") if hull else _p(d_rays), R, N, int(lindisp), _p(d_tr), ar.ptr("z"), _stream()), "pnr_stratified")
    if len(ids):
        call_labels(lib, ar.ptr("z"), R, N, ar.ptr("ht"), ar.ptr("hb"), ar.ptr("hc"), mh, d_ids, ar.ptr("ls"), ar.ptr("li"))
    return ar.read(unwritten=() if len(ids) else ("ls", "li"))


def compare_setup(got, ref, tag, labels=True):
    keys = ("ht", "hb", "hc", "z") + (("ls", "li") if labels else ())
    return [m for m in (diff(got[k], ref[k], f"{tag} {k}") for k in keys) if m]


def test_the_harness_notices_a_wrong_word_and_a_missing_one(dev):
    """the comparison itself: one ulp, the sign of a zero, a NaN against a number and a label are reported; an output the kernel
    was not given is reported as never written; a word written into a guard is reported"""
    rays, (box, ids) = POOL[:65], big_boxes(64)
    ref = oracle_setup(rays, box, ids, 3, 5, False, None, 1)
    g, b = run_setup(dev, rays, box, ids, 3, 5, False, None, 1)
    assert not b + compare_setup(g, ref, "fused")
    z = ref["z"].copy()
    z[7, 2] = np.nextafter(z[7, 2], np.float32(np.inf))
    assert "1 of 325 words differ, first at 37" in diff(g["z"], z, "z")
    z = ref["z"].copy()
    z[0, 0] = np.nan
    assert diff(g["z"], z, "z") and not diff(z.view(np.int32), z, "z")
    assert diff(np.array([0], np.int32), np.array([-0.0], np.float32), "zero") and not diff(np.array([0], np.int32), np.array([0.0], np.float32), "zero")
    ls = ref["ls"].copy()
    ls[64, 4] += 1
    assert "first at 324" in diff(g["ls"], ls, "ls") and diff(g["ls"], ls[:64], "ls")
    ar = setup_arena(dev, 65, 5, 3)
    keep = [put(dev, rays), put(dev, box), put(dev, ids)]
    call_setup(_lib.load(), keep[0], 65, keep[1], 64, 3, keep[2], 5, False, None, 1, ar, labels=False)
    _, b = ar.read()
    assert sorted(b) == ["li: 325 words never written", "ls: 325 words never written"]
    ar.buf[ar.off["z"][0] + 325] = 0
    ar.buf[ar.off["ht"][0] - 1] = 0
    assert any("guard touched" in m for m in ar.read(unwritten=("ls", "li"))[1])


# ------------------------------------------------------------------------------- k_stratified, k_points, k_sample_labels
NS = list(range(1, 131)) + [191, 192, 193, 255, 256, 257]


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("jitter", [False, True])
def test_stratified_points_labels_at_every_n(dev, lindisp, jitter):
    """every N = 1 .. 130 and around 192 / 256, R = 1, 63, 64, 65, 257; the labels from overflowing lists of 3"""
    lib = _lib.load()
    box, ids = big_boxes(64)
    d_ids = put(dev, ids)
    d_tr = put(dev, TRAND)
    bad = []
    for R in (1, 63, 64, 65, 257):
        rays = POOL[:R]
        ht, hb, hc = oracle_hits(R, 64, 3)
        assert R < 63 or hc.max() > 3
        d_rays, d_ht, d_hb, d_hc = put(dev, rays), put(dev, ht), put(dev, hb), put(dev, hc)
        for N in NS:
            tr = TRAND[:R * N].reshape(R, N) if jitter else None
            ar = Arena(dev, z=R * N, pts=R * N * 3, ls=R * N, li=R * N)
            call_stratified(lib, d_rays, R, N, lindisp, d_tr if jitter else None, ar.ptr("z"))
            call_points(lib, d_rays, ar.ptr("z"), R, N, ar.ptr("pts"))
            call_labels(lib, ar.ptr("z"), R, N, _p(d_ht), _p(d_hb), _p(d_hc), 3, d_ids, ar.ptr("ls"), ar.ptr("li"))
            got, b = ar.read()
            z = co.stratified(rays, N, lindisp, tr)
            ls, li = co.sample_labels(z, ht, hb, hc, ids)
            tag = f"R={R} N={N}"
            check(b, diff(got["z"], z, tag + " z"), diff(got["pts"], co.points(rays, z), tag + " pts"),
                  diff(got["ls"], ls, tag + " ls"), diff(got["li"], li, tag + " li"))
            bad += [f"{tag}: {x}" for x in b]
    assert not bad, "\n".join(bad[:30])


# ------------------------------------------------------------------------------------------ k_bbox_hits, k_restrict_rays
@pytest.mark.parametrize("mh", [1, 2, 7, 8, 9, 33, 64])
def test_bbox_hits_and_hull_over_ray_and_table_sizes(dev, mh):
    """R = 1, 255, 256, 257, 4099 x M = 0, 1, 2, 15, 64, 300; the tables of 64 and 300 overflow every list up to 9"""
    lib = _lib.load()
    bad = []
    for M in (0, 1, 2, 15, 64, 300):
        box, _ = big_boxes(M)
        d_box = put(dev, box) if M else None
        for R in (1, 255, 256, 257, 4099):
            rays = POOL[:R]
            d_rays = put(dev, rays)
            ar = Arena(dev, ht=R * mh * 2, hb=R * mh, hc=R, rays=R * 8)
            call_bbox(lib, d_rays, R, d_box, M, mh, ar.ptr("ht"), ar.ptr("hb"), ar.ptr("hc"))
            call_restrict(lib, d_rays, R, ar.ptr("ht"), ar.ptr("hc"), mh, ar.ptr("rays"))
            got, b = ar.read()
            ht, hb, hc = oracle_hits(R, M, mh)
            if M >= 64 and R >= 255 and mh <= 9:
                assert hc.max() > mh, (M, R, int(hc.max()))
            tag = f"M={M} R={R}"
            check(b, diff(got["ht"], ht, tag + " hit_t"), diff(got["hb"], hb, tag + " hit_box"), diff(got["hc"], hc, tag + " hit_count"),
                  diff(got["rays"], co.restrict_rays(rays, ht, hc), tag + " restricted rays"))
            bad += b
    assert not bad, "\n".join(bad[:30])


# ------------------------------------------------------------------------------------------------------------ k_ray_setup
@pytest.mark.parametrize("mh", range(1, 9))
def test_ray_setup_stage_by_stage_and_against_the_separate_kernels(dev, mh):
    """R = 1, 2, 63 .. 65, 127 .. 129, 1000 (an odd tail ends the two-rays-in-hand loop on its first ray) x N = 1, 2, 63 .. 65,
    127 .. 129, 192, 257 (the lanes' i += 64 walk) x hull x lindisp x jitter, with the label outputs and without: every output
    equals the C oracle's, the four separate entry points', and z is the same words with and without labels"""
    box, ids = big_boxes(64)
    bad = []
    for R in (1, 2, 63, 64, 65, 127, 128, 129, 1000):
        rays = POOL[:R]
        assert R < 63 or oracle_hits(R, 64, mh)[2].max() > mh
        for N in (1, 2, 63, 64, 65, 127, 128, 129, 192, 257):
            for hull in (0, 1):
                for lindisp in (False, True):
                    for jitter in (False, True):
                        tr = TRAND[:R * N].reshape(R, N) if jitter else None
                        ref = oracle_setup(rays, box, ids, mh, N, lindisp, tr, hull)
                        tag = f"R={R} N={N} hull={hull} lindisp={int(lindisp)} jitter={int(jitter)}"
                        g1, b1 = run_setup(dev, rays, box, ids, mh, N, lindisp, tr, hull, labels=True)
                        g0, b0 = run_setup(dev, rays, box, ids, mh, N, lindisp, tr, hull, labels=False)
                        g4, b4 = run_separate(dev, rays, box, ids, mh, N, lindisp, tr, hull)
                        b = b1 + b0 + b4 + compare_setup(g1, ref, "fused") + compare_setup(g0, ref, "fused, no labels", labels=False)
                        b += compare_setup(g4, ref, "separate")
                        if hull:
                            check(b, diff(g4["rays"], ref["rays"], "separate rays"))
                        if g1["z"].tobytes() != g0["z"].tobytes() or g1["z"].tobytes() != g4["z"].tobytes():
                            b.append("z differs between the fused call with labels, without labels and the separate kernels")
                        bad += [f"{tag}: {x}" for x in b]
    assert not bad, "\n".join(bad[:30])


# -------------------------------------------------------------------------------------------------------------- edge rays
EYE = np.eye(3, dtype=np.float32).reshape(-1)
S2 = np.float32(np.sqrt(0.5))
C30, S30 = np.float32(np.cos(0.5)), np.float32(np.sin(0.5))


def _box(c, rot, e):
    return np.array(list(c) + list(rot) + list(e), np.float32)


EDGE_BOX = np.stack([
    _box((0, 0, 5), EYE, (1, 1, 1)),                                    # 0: the unit box on the optical axis
    _box((0, 0, 5), EYE, (1, 1, 1)),                                    # 1: its duplicate: tied t_in, the lower index first
    _box((0, 0, 5), EYE, (0.25, 0.25, 0.25)),                           # 2: nested in 0: entered later
    _box((0, 0, 0), EYE, (0, 0, 0)),                                    # 3: zero extent, through the origin of most rays
    _box((0, 0, 12), (S2, 0, S2, 0, 1, 0, -S2, 0, S2), (1, 1, 1)),      # 4: turned 45 degrees about y
    _box((3, 0, 9), (C30, 0, S30, 0, 1, 0, -S30, 0, C30), (2, 0.5, 1)),  # 5: turned 0.5 rad
    _box((0, 0, 5), (0, 0, 1, 1, 0, 0, 0, 1, 0), (0.5, 0.5, 0.75)),     # 6: axes permuted (its first axis is world z), inside 0
])
EDGE_IDS = np.array([[10, 20], [11, 21], [12, 22], [13, 23], [14, 24], [15, 25], [16, 26]], np.int32)


def edge_rays():
    inf, nan = np.inf, np.nan
    rows = []

    def add(o, d, near=0.25, far=40.0):
        rows.append(list(o) + list(d) + [near, far])
    add((0.125, 0.0625, -1), (0, 0, 1))                                 # ray 0: through boxes 0, 1, 6, 2 and 4, clear of every face
    for sgn in (1.0, -1.0):
        for off in (0.0, 0.5, 1.0, -1.0, 1.5, 0.25, -0.25):          # inside the slab, on a face, outside, on the nested box's face
            add((off, 0, 5 - 6 * sgn), (0, 0, sgn))                     # along z
            add((5 - 6 * sgn, off, 5), (sgn, 0, 0))                     # along x
            add((0, 5 - 6 * sgn, 5 + off), (0, sgn, 0))                 # along y
            add((off, off, 5 - 6 * sgn), (-0.0, 0.0, sgn))              # a negative zero component
    for d in ((0, 0, 1), (0.3, 0.1, 1), (-1, 0, 0), (0, -2, 0), (1, 1, 1), (0, 0, 0)):
        add((0, 0, 5), d)                                               # origins inside boxes 0, 1, 2, 6
        add((0.1, 0.2, 4.9), d)
        add((0, 0, 0), d)                                               # on the zero-extent box
        add((0, 0, 0), d, near=0.0)
        add((0, 0, 0), d, near=-1.0)
    add((0, 0, 0), (0, 0, 1), 5.0, 5.0)                                 # near == far inside box 0, on its face, outside
    add((0, 0, 0), (0, 0, 1), 4.0, 4.0)
    add((0, 0, 0), (0, 0, 1), 2.0, 2.0)
    add((0, 0, 0), (0, 0, 1), 0.0, 40.0)                                # near = 0 (lindisp: 1 / 0)
    add((0, 0, 0), (0.2, 0, 1), 0.0, 40.0)
    add((0, 0, 0), (0, 0, 1), 0.25, inf)                                # far = inf
    add((0, 0, 0), (0.1, 0.05, 1), 0.0, inf)
    add((nan, 0, 0), (0, 0, 1))                                         # NaN origin
    add((0, 0, nan), (0, 0, 1))
    add((0, 0, 0), (inf, 0, 1))                                         # Inf direction
    add((0, 0, 0), (0, 0, inf))
    add((0, 0, 0), (0, 0, -inf))
    add((0, 0, 0), (0, 0, 1), 8.0, 2.0)                                 # far < near
    add((0.25, 0, 0), (0, 0, 1))                                        # grazing the nested box's face plane: on its slab's face
    return np.array(rows, np.float32)


def test_edge_rays_through_bbox_hits_and_ray_setup(dev):
    """degenerate rays against degenerate boxes through k_bbox_hits (+ k_restrict_rays, k_sample_labels) and k_ray_setup: every
    word equals the C oracle's (NaNs by position), under both `lindisp` and `hull` settings; then what the rule means on them"""
    rays = edge_rays()
    R = rays.shape[0]
    bad = []
    for mh in (1, 2, 7, 8):
        for N in (2, 5, 64):
            for hull in (0, 1):
                for lindisp in (False, True):
                    ref = oracle_setup(rays, EDGE_BOX, EDGE_IDS, mh, N, lindisp, None, hull)
                    tag = f"mh={mh} N={N} hull={hull} lindisp={int(lindisp)}"
                    g1, b1 = run_setup(dev, rays, EDGE_BOX, EDGE_IDS, mh, N, lindisp, None, hull)
                    g4, b4 = run_separate(dev, rays, EDGE_BOX, EDGE_IDS, mh, N, lindisp, None, hull)
                    b = b1 + b4 + compare_setup(g1, ref, "fused") + compare_setup(g4, ref, "separate")
                    if hull:
                        check(b, diff(g4["rays"], ref["rays"], "separate rays"))
                    bad += [f"{tag}: {x}" for x in b]
    for mh in (9, 64):
        g4, b4 = run_separate(dev, rays, EDGE_BOX, EDGE_IDS, mh, 5, False, None, 1)
        ref = oracle_setup(rays, EDGE_BOX, EDGE_IDS, mh, 5, False, None, 1)
        bad += [f"mh={mh}: {x}" for x in b4 + compare_setup(g4, ref, "separate")]
    assert not bad, "\n".join(bad[:40])
    # the meaning, on the kernel's own words (fused call, lists of 8, hull on: z[0] = t_in and z[N - 1] = t_out of the hull)
    g, _ = run_setup(dev, rays, EDGE_BOX, EDGE_IDS, 8, 64, False, None, 1)
    edge_meaning(rays, g["ht"].view(np.float32).reshape(R, 8, 2), g["hb"].reshape(R, 8), g["hc"], g["z"].view(np.float32).reshape(R, 64),
                 g["ls"].reshape(R, 64))


def edge_meaning(rays, ht, hb, hc, z, ls):
    """ray 0 starts at z = -1 and goes +z with near 0.25: boxes 0 and 1 span t in [5, 7], box 6 [5.5, 6.5], the nested box 2
    [5.75, 6.25], the turned box 4 starts near 11.7; the zero-extent box 3 and box 5 are missed"""
    assert list(hb[0, :5]) == [0, 1, 6, 2, 4] and hc[0] == 5                        # tied t_in: the lower index first
    assert list(ht[0, :4, 0]) == [5.0, 5.0, 5.5, 5.75] and list(ht[0, :4, 1]) == [7.0, 7.0, 6.5, 6.25]
    assert z[0, 0] == 5.0 and ls[0, 0] == 10            # a sample exactly on t_in is labelled, by the lower index of the tie
    inner = np.flatnonzero((z[0] >= 5.75) & (z[0] <= 6.25))
    assert inner.size and (ls[0, inner] == 10).all()    # inside the nested box: the label of the nearest t_in, not of the smallest box
    assert z[0, 63] == ht[0, 4, 1] and ls[0, 63] == 14  # a sample exactly on t_out
    assert (ls[0, (z[0] > 7.0) & (z[0] < ht[0, 4, 0])] == -1).all()
    on_face = np.flatnonzero((rays[:, 0] == 1.0) & (rays[:, 1] == 0) & (rays[:, 2] == -1) & (rays[:, 5] == 1.0) & ~np.signbit(rays[:, 3]))[0]
    assert 0 not in hb[on_face] and 1 not in hb[on_face]                            # along a face of box 0: a miss
    inside = np.flatnonzero((rays[:, 0] == 0.5) & (rays[:, 1] == 0) & (rays[:, 2] == -1) & (rays[:, 5] == 1.0))[0]
    assert list(hb[inside, :2]) == [0, 1]                                           # along z inside the slabs of x and y: a hit
    zero = np.flatnonzero((rays[:, :3] == 0).all(1) & (rays[:, 3:6] == 1).all(1) & (rays[:, 6] == 0.0))[0]
    assert hb[zero, 0] == 3 and ht[zero, 0, 0] == 0 and not np.signbit(ht[zero, 0, 0])        # max(+0 near, -0) = +0
    below = np.flatnonzero((rays[:, :3] == 0).all(1) & (rays[:, 3:6] == 1).all(1) & (rays[:, 6] == -1.0))[0]
    assert hb[below, 0] == 3 and ht[below, 0, 0] == 0 and np.signbit(ht[below, 0, 0]) and not np.signbit(ht[below, 0, 1])   # min(-0, +0) = -0
    still = np.flatnonzero((rays[:, :3] == (0, 0, 5)).all(1) & (rays[:, 3:6] == 0).all(1))[0]
    assert sorted(hb[still, :4]) == [0, 1, 2, 6] and (ht[still, :4] == rays[still, 6:8]).all()      # d = 0: the boxes that contain o, [near, far]


def test_nine_overlapping_boxes_drop_the_farthest(dev):
    """nine boxes along the ray, each overlapping the next, in shuffled table order; lists of 8 drop the one entered last, so a
    sample inside that one alone is labelled -1 (and labelled once the list holds 9), through both paths"""
    order = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    box = np.stack([_box((0, 0, 4 * k + 3), EYE, (1, 1, 3)) for k in order])       # box k spans z in [4 k, 4 k + 6]
    ids = np.array([[100 + k, 200 + k] for k in order], np.int32)
    rays = np.array([[0, 0, 0, 0, 0, 1, 0, 72], [0.5, -0.5, 0, 0, 0, 1, 0, 72]], np.float32)         # N = 3: z = 0, 36, 72
    ref = oracle_setup(rays, box, ids, 8, 3, False, None, 0)
    assert list(ref["hc"]) == [9, 9] and list(ref["z"][0]) == [0.0, 36.0, 72.0] and order.index(8) not in ref["hb"][0]
    assert list(ref["ls"][0]) == [100, -1, -1]
    for run in (run_setup, run_separate):
        g, b = run(dev, rays, box, ids, 8, 3, False, None, 0)
        assert not b + compare_setup(g, ref, run.__name__), b
        assert list(g["ls"].reshape(2, 3)[0]) == [100, -1, -1] and list(g["li"].reshape(2, 3)[1]) == [200, -1, -1]
    g, b = run_separate(dev, rays, box, ids, 9, 3, False, None, 0)
    assert not b + compare_setup(g, oracle_setup(rays, box, ids, 9, 3, False, None, 0), "separate, lists of 9")
    assert list(g["ls"].reshape(2, 3)[0]) == [100, 108, -1]


# ------------------------------------------------------------------------------------------------------ grid-stride trips
def trip_rays(R, seed):
    rng = np.random.default_rng(seed)
    rays = np.zeros((R, 8), np.float32)
    rays[:, 0:3] = rng.normal(0, 0.3, (R, 3))
    rays[:, 3:5] = rng.uniform(-0.6, 0.6, (R, 2))
    rays[:, 5] = 1.0
    rays[:, 6] = rng.uniform(0.2, 2.0, R)
    rays[:, 7] = rng.uniform(20.0, 60.0, R)
    return rays


def _slices(R):
    a, b = R // 3 + 1, 2 * (R // 3) + 6
    return (slice(0, a), slice(a, b), slice(b, R))


def test_ray_setup_three_trips_and_a_second_launch(dev):
    """R = 2 * 8 * CU * 64 + 77 rays: every workgroup walks its grid-stride loop three times, re-using its LDS tables after the
    closing barrier.  Equal to the oracle, to the same call on three slices, and to a second launch in the same process."""
    cu = torch.cuda.get_device_properties(dev).multi_processor_count
    R, N, mh = 2 * 8 * cu * 64 + 77, 3, 2
    box, ids = big_boxes(5, seed=2, scale=4.0)
    rays = trip_rays(R, 1)
    tr = np.random.default_rng(2).random((R, N)).astype(np.float32)
    ref = oracle_setup(rays, box, ids, mh, N, False, tr, 1)
    assert ref["hc"].max() > mh and (ref["hc"] == 0).any() and (ref["ls"] >= 0).any()
    g, b = run_setup(dev, rays, box, ids, mh, N, False, tr, 1)
    assert not b + compare_setup(g, ref, "one launch"), (b + compare_setup(g, ref, "one launch"))[:5]
    g2, b2 = run_setup(dev, rays, box, ids, mh, N, False, tr, 1)
    assert not b2 and all(g[k].tobytes() == g2[k].tobytes() for k in g)
    parts = [run_setup(dev, rays[s], box, ids, mh, N, False, tr[s], 1) for s in _slices(R)]
    assert not sum((p[1] for p in parts), [])
    for k in ("ht", "hb", "hc", "z", "ls", "li"):
        assert np.concatenate([p[0][k] for p in parts]).tobytes() == g[k].tobytes(), k
    g0, b0 = run_setup(dev, rays, box, ids, mh, N, True, None, 0, labels=False)
    ref0 = oracle_setup(rays, box, ids, mh, N, True, None, 0)
    assert not b0 + compare_setup(g0, ref0, "lindisp, no labels", labels=False)


def test_the_256_thread_kernels_three_trips(dev):
    """k_stratified, k_points, k_sample_labels at R N > 2 * 8 * CU * 256 samples, k_bbox_hits and k_restrict_rays at as many rays:
    equal to the oracle and to three slice launches"""
    lib = _lib.load()
    cu = torch.cuda.get_device_properties(dev).multi_processor_count
    R, mh = 2 * 8 * cu * 256 + 77, 2
    box, ids = big_boxes(5, seed=2, scale=4.0)
    rays = trip_rays(R, 3)
    d_box, d_ids = put(dev, box), put(dev, ids)

    def hits(rs):
        n = rs.shape[0]
        d_rays = put(dev, rs)
        ar = Arena(dev, ht=n * mh * 2, hb=n * mh, hc=n, rays=n * 8)
        call_bbox(lib, d_rays, n, d_box, 5, mh, ar.ptr("ht"), ar.ptr("hb"), ar.ptr("hc"))
        call_restrict(lib, d_rays, n, ar.ptr("ht"), ar.ptr("hc"), mh, ar.ptr("rays"))
        return ar.read()
    g, b = hits(rays)
    ht, hb, hc = co.bbox_hits(rays, box, mh)
    check(b, diff(g["ht"], ht, "hit_t"), diff(g["hb"], hb, "hit_box"), diff(g["hc"], hc, "hit_count"),
          diff(g["rays"], co.restrict_rays(rays, ht, hc), "restricted rays"))
    assert not b, b
    parts = [hits(rays[s]) for s in _slices(R)]
    assert not sum((p[1] for p in parts), [])
    for k in g:
        assert np.concatenate([p[0][k] for p in parts]).tobytes() == g[k].tobytes(), k

    Rs, N = (R + 2) // 3, 3                     # R N > 2 * 8 * CU * 256 samples

    def samples(s):
        n = s.stop - s.start
        d_rays, d_tr = put(dev, rays[s]), put(dev, tr[s])
        keep = [put(dev, x[s]) for x in (ht, hb, hc)]
        ar = Arena(dev, z=n * N, pts=n * N * 3, ls=n * N, li=n * N)
        call_stratified(lib, d_rays, n, N, True, d_tr, ar.ptr("z"))
        call_points(lib, d_rays, ar.ptr("z"), n, N, ar.ptr("pts"))
        call_labels(lib, ar.ptr("z"), n, N, _p(keep[0]), _p(keep[1]), _p(keep[2]), mh, d_ids, ar.ptr("ls"), ar.ptr("li"))
        return ar.read()
    tr = np.random.default_rng(4).random((Rs, N)).astype(np.float32)
    assert Rs * N > 2 * 8 * cu * 256
    g, b = samples(slice(0, Rs))
    z = co.stratified(rays[:Rs], N, True, tr)
    ls, li = co.sample_labels(z, ht[:Rs], hb[:Rs], hc[:Rs], ids)
    check(b, diff(g["z"], z, "z"), diff(g["pts"], co.points(rays[:Rs], z), "pts"), diff(g["ls"], ls, "ls"), diff(g["li"], li, "li"))
    assert not b, b
    parts = [samples(s) for s in _slices(Rs)]
    assert not sum((p[1] for p in parts), [])
    for k in g:
        assert np.concatenate([p[0][k] for p in parts]).tobytes() == g[k].tobytes(), k


# ------------------------------------------------------------------------------------------------------------------ k_embed
def embed_inputs(n, seed=0):
    """N(0, 30) with a few at +-150 (tests/test_setup_ref.py draws the same for the C oracle)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 30.0, (n, 3)).astype(np.float32)
    k = min(n, 4)
    x[:k] = np.array([[150.0, -150.0, 0.0], [-150.0, 150.0, 149.99], [0.0, -0.0, 1e-30], [3.1415927, 1.5707964, 100.0]], np.float32)[:k]
    return x


def run_embed(dev, x, L):
    n = x.shape[0]
    ar = Arena(dev, out=n * (3 + 6 * L))
    d_x = put(dev, x)
    _lib.check(_lib.load().pnr_embed(_p(d_x), n, L, ar.ptr("out"), _stream()), "pnr_embed")
    g, b = ar.read()
    return g["out"].view(np.float32).reshape(n, 3 + 6 * L), b


def embed_check(x, out, L):
    """identity columns bit for bit; the bands against float64: (problems, worst error on bands < 10, on bands >= 10)"""
    bad = [] if out[:, :3].tobytes() == x.tobytes() else ["identity columns differ from x"]
    if L == 0:
        return bad, 0.0, 0.0
    err = np.abs(out[:, 3:].astype(np.float64) - sr.embed64(x, L)[:, 3:]).reshape(x.shape[0], L, 6).max((0, 2))      # per band
    lo, hi = float(err[:10].max()), float(err[10:].max()) if L > 10 else 0.0
    if lo > m32.TRIG_BOUND:
        bad.append(f"bands < 10: worst error {lo:.3g} > TRIG_BOUND {m32.TRIG_BOUND:.3g}")
    if hi > m32.TRIG_BOUND:       # a correct sinf does not lose accuracy with the argument: the same bound
        bad.append(f"bands 10 .. {L - 1}: worst error {hi:.3g} > TRIG_BOUND {m32.TRIG_BOUND:.3g}")
    return bad, lo, hi


def test_embed_every_band_count_against_float64(dev):
    """L = 0 .. 16 x n = 1, 85, 1001 and one size of three grid-stride trips (also equal to three slice launches)"""
    cu = torch.cuda.get_device_properties(dev).multi_processor_count
    bad = []
    for L in range(17):
        for n in (1, 85, 1001):
            x = embed_inputs(n, seed=L)
            out, b = run_embed(dev, x, L)
            c, lo, hi = embed_check(x, out, L)
            _note("embed_band_lt10", lo)
            _note("embed_band_ge10", hi)
            bad += [f"L={L} n={n}: {m}" for m in b + c]
    for L in (1, 16):
        n = (2 * 8 * cu * 256) // (3 + 6 * L) + 77
        x = embed_inputs(n, seed=99)
        out, b = run_embed(dev, x, L)
        c, lo, hi = embed_check(x, out, L)
        _note("embed_band_lt10", lo)
        _note("embed_band_ge10", hi)
        parts = [run_embed(dev, x[s], L) for s in _slices(n)]
        if np.concatenate([p[0] for p in parts]).tobytes() != out.tobytes():
            c.append("three slice launches give other words")
        bad += [f"L={L} n={n}: {m}" for m in b + c + sum((p[1] for p in parts), [])]
    print("k_embed worst |float32 - float64|: bands < 10 %.3g, bands >= 10 %.3g (TRIG_BOUND %.3g)"
          % (_WORST["embed_band_lt10"], _WORST["embed_band_ge10"], m32.TRIG_BOUND))
    assert not bad, "\n".join(bad[:30])


# ----------------------------------------------------------------------------------------------------- one frame-sized call
@pytest.mark.parametrize("hull", [0, 1])
@pytest.mark.parametrize("jitter", [False, True])
def test_frame_sized_call_properties(dev, hull, jitter):
    """a 376 x 1408 frame against 64 boxes, 64 samples, lists of 8: z non-decreasing along every ray, inside [near, far] (inside
    the hull of the kept intervals under the hull switch; rays without a hit keep [near, far]), and a sample is labelled exactly
    where a kept interval contains it"""
    lib = _lib.load()
    rays = synthetic.camera_rays(width=1408, height=376)
    R, N, mh = rays.shape[0], 64, 8
    assert R == 376 * 1408
    box, ids = big_boxes(64, seed=1, scale=2.0)
    d_rays, d_box, d_ids = rays.to(dev), put(dev, box), put(dev, ids)
    d_tr = torch.rand((R, N), generator=torch.Generator().manual_seed(3)).to(dev) if jitter else None
    ar = setup_arena(dev, R, N, mh)
    call_setup(lib, d_rays, R, d_box, 64, mh, d_ids, N, False, d_tr, hull, ar)
    torch.cuda.synchronize()
    z, ht = ar.view("z").view(R, N), ar.view("ht").view(R, mh, 2)
    hc, ls, li = ar.view("hc", torch.int32), ar.view("ls", torch.int32).view(R, N), ar.view("li", torch.int32).view(R, N)
    kept = hc.clamp(max=mh)
    assert int(hc.max()) > mh and int((hc == 0).sum()) > 0
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    lo, hi = d_rays[:, 6].clone(), d_rays[:, 7].clone()
    if hull:
        use = torch.arange(mh, device=dev)[None, :] < kept[:, None]
        inf = torch.tensor(float("inf"), device=dev)
        hit = kept > 0
        lo = torch.where(hit, torch.where(use, ht[..., 0], inf).amin(1), lo)
        hi = torch.where(hit, torch.where(use, ht[..., 1], -inf).amax(1), hi)
        assert bool((lo >= d_rays[:, 6]).all() and (hi <= d_rays[:, 7]).all())
    assert bool((z >= lo[:, None]).all() and (z <= hi[:, None]).all())
    if not jitter:
        assert bool((z[:, 0] == lo).all() and (z[:, -1] == hi).all())
    inside = torch.zeros((R, N), dtype=torch.bool, device=dev)
    for h in range(mh):
        inside |= (h < kept)[:, None] & (ht[:, h, 0:1] <= z) & (z <= ht[:, h, 1:2])
    assert bool(((ls >= 0) == inside).all() and ((li >= 0) == inside).all())
    assert 0.02 < float(inside.float().mean()) < 0.98
    _, b = ar.read()
    assert not b, b


def test_frame_rays_against_float64(dev):
    """20 000 rays of the frame against 64 boxes (extents x 4), lists of 8, through k_ray_setup with the hull switch: on the
    safe rays (tests/_setup_ref.py: at most 1 % are not) counts and boxes equal float64's, the depths lie inside the derived
    bounds, and z lies inside stratified64's bound on the kernel's own hull -- the docstring's table"""
    rays = ray_pool(20000, seed=4)
    rays[:, 6:8] = (0.5, 100.0)
    box, ids = big_boxes(64, seed=5, scale=4.0)
    mh, N = 8, 64
    chunks = [slice(i, i + 4000) for i in range(0, 20000, 4000)]
    unsafe = np.concatenate([sr.unsafe_rays(rays[c], box, mh) for c in chunks])
    assert unsafe.mean() <= 0.01
    keep = ~unsafe
    h64 = [np.concatenate(x) for x in zip(*(sr.bbox_hits64(rays[c], box) for c in chunks))]
    b_in, b_out, _ = [np.concatenate(x) for x in zip(*(sr.interval_bounds(rays[c], box) for c in chunks))]
    t64, b64, n64 = sr.kept_lists(*h64, mh)
    tr = np.random.default_rng(8).random((20000, N)).astype(np.float32)
    for lindisp in (False, True):
        for jitter in (False, True):
            g, b = run_setup(dev, rays, box, ids, mh, N, lindisp, tr if jitter else None, 1)
            assert not b, b
            ht, hb, hc = g["ht"].view(np.float32).reshape(-1, mh, 2), g["hb"].reshape(-1, mh), g["hc"]
            assert np.array_equal(hc[keep], n64[keep]) and np.array_equal(hb[keep], b64[keep]) and n64[keep].max() > mh
            sel, idx = keep[:, None] & (b64 >= 0), np.maximum(b64, 0).astype(np.int64)
            for end, bnd in enumerate((b_in, b_out)):
                tol = np.take_along_axis(bnd, idx, 1)
                err = np.abs(ht[..., end].astype(np.float64) - t64[..., end])
                assert (err[sel] <= tol[sel]).all(), (end, float((err[sel] - tol[sel]).max()))
                _note("t_err", err[sel].max())
                _note("t_ratio", (err[sel] / np.maximum(tol[sel], 1e-300)).max())
            hull = sr.restrict64(rays, ht, hc).astype(np.float32)       # the kernel's own hull: z's error is the sampler's alone
            z = g["z"].view(np.float32).reshape(-1, N).astype(np.float64)
            ref, tol = sr.stratified64(hull, N, lindisp, tr if jitter else None), sr.stratified_bound(hull, N, lindisp, jitter)
            err = np.abs(z - ref)
            assert (err <= tol).all(), (lindisp, jitter, float((err / tol).max()))
            q = "zd" if lindisp else "z"
            _note(q + "_err", err.max())
            _note(q + "_ratio", (err / tol).max())
            a, bb = sr.labels_vec(g["z"].view(np.float32).reshape(-1, N), ht, hb, hc, ids)
            assert np.array_equal(g["ls"].reshape(-1, N), a) and np.array_equal(g["li"].reshape(-1, N), bb)
    print("against float64:", {k: "%.3g" % v for k, v in sorted(_WORST.items())})
