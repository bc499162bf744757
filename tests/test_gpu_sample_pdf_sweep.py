"""sample_pdf at EVERY coarse sample count, against the C oracle, bit for bit (COVERAGE.md row a7).

pnr_sampling.hip has five sampler kernels -- k_sample_pdf<64, 256>, <256, 512> (one template over sample_pdf_body), their
in-kernel-u twins <..., PnrRngDev> and the inference instance k_sample_pdf_det, all assembled from the pieces of
pnr_sampling_dev.h -- whose code depends on the shape in many places: the ATen-ordered sum (groups of 32 weights,
leftover vectors of 8, a scalar tail; four scalar accumulators for rows shorter than 8), the CDF (an exact parallel scan for
nw = Nc - 2 <= 64 well-conditioned values, a sequential double chain otherwise), fixed-depth bisections that start at the largest
power of two <= Nc / <= Nf, loops that stride by 64 lanes, a bitonic sort padded to a power of two, the dispatch on Nc <= 64,
Nf <= 192, P <= 256, max_hits <= 64, and hit lists kept one entry per lane.  tests/test_gpu_stages.py pins a dozen (Nc, Nf)
pairs; here every Nc = 3 .. 256 runs, on inputs (tests/_sample_pdf_cases.py) whose rows sit on both sides of every
data-dependent branch.  There is no tolerance in this file: every comparison is np.array_equal / torch.equal."""
import functools

import numpy as np
import pytest
import torch

import _sample_pdf_cases as cases
from oracle import c_oracle as co
from panopticnerf_amd import ops

pytestmark = pytest.mark.gpu

R = cases.R_CASE
NC_LIST = (3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 129, 256)         # the label / in-kernel-u cases: around every threshold
F_CANARY, GUARD = -12345.678, 37


def T(x, dev):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).to(dev)        # a copy: shared references are read-only


def N_(t):
    return t.detach().cpu().numpy()


def _bands(lo, hi, width):
    return [(a, min(a + width - 1, hi)) for a in range(lo, hi + 1, width)]


@functools.lru_cache(maxsize=None)
def _case(Nc):
    out = cases.case(Nc)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=256)
def _want(Nc, Nf, given):
    """the oracle's (z_samples, inds, z_fine, u) of the case at (Nc, Nf): computed once, shared, read-only"""
    _, _, z, w = _case(Nc)
    u = cases.uniforms(Nc, Nf) if given else None
    zs, inds = co.sample_pdf(z, w, Nf, u)
    out = (zs, inds, co.merge_sorted(z, zs), u)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _boxes(seed, M=96):
    """Axis-parallel boxes strung along the rays of cases.rays (origin ~ (0, 1.5, 0), direction ~ +z): 72 wide ones that nearly every
    ray crosses -- more than any max_hits <= 64 keeps -- and 24 small ones that few rays cross."""
    rng = np.random.default_rng(seed)
    box = np.zeros((M, 15), np.float32)
    box[:, 0:3] = np.stack([rng.normal(0, 2, M), 1.5 + rng.normal(0, 2, M), rng.uniform(2, 55, M)], 1)
    box[:, 3:12] = np.eye(3, dtype=np.float32).reshape(-1)
    box[:72, 12:15] = np.stack([rng.uniform(15, 25, 72), rng.uniform(15, 25, 72), rng.uniform(0.3, 4, 72)], 1)
    box[72:, 12:15] = rng.uniform(0.3, 2, (M - 72, 3))
    box = box[rng.permutation(M)]
    ids = np.stack([rng.integers(0, 11, M), rng.integers(0, 7, M)], 1).astype(np.int32)
    return box, ids


def _general(monkeypatch, on):
    if on:
        monkeypatch.setenv("PNR_SAMPLE_PDF_GENERAL", "1")
    else:
        monkeypatch.delenv("PNR_SAMPLE_PDF_GENERAL", raising=False)


# ------------------------------------------------------------------------------------------------- 1: the general bodies, every Nc
@pytest.mark.parametrize("lo,hi", _bands(3, 256, 16))
def test_general_bodies_at_every_coarse_count(dev, lo, hi):
    """ops.sample_pdf(want_samples=True) -- sample_pdf_body<64, 256> up to Nc = 64 and P = 256, <256, 512> beyond -- at every
    Nc x Nf in {1, 2, 63, 64, 65, 128, 192, 512 - Nc}, deterministic and given u: indices, z_samples and z_fine."""
    wrong = []
    for Nc in range(lo, hi + 1):
        rays, t_rand, z, w = _case(Nc)
        assert np.array_equal(N_(ops.stratified(T(rays, dev), Nc, False, T(t_rand, dev))), z), Nc
        zd, wd = T(z, dev), T(w, dev)
        for Nf in cases.nf_general(Nc):
            for given in (False, True):
                zs_c, inds_c, zf_c, u = _want(Nc, Nf, given)
                zf, zs, inds = ops.sample_pdf(zd, wd, Nf, T(u, dev))
                ok = (np.array_equal(N_(inds), inds_c), np.array_equal(N_(zs), zs_c), np.array_equal(N_(zf), zf_c))
                if not all(ok):
                    wrong.append((Nc, Nf, "given" if given else "det") + ok)
    assert not wrong, "Nc %s: (Nc, Nf, u, inds ok, z_samples ok, z_fine ok) %s" % (sorted({c[0] for c in wrong}), wrong[:16])


# ------------------------------------------------------------------------------------------------- 2: the inference instance
@pytest.mark.parametrize("lo,hi", _bands(3, 64, 16))
def test_inference_instance_at_every_coarse_count(dev, lo, hi, monkeypatch):
    """want_samples=False with deterministic u is what an inference frame launches: k_sample_pdf_det for Nc <= 64, Nf <= 192,
    Nc + Nf <= 256.  Every Nc x Nf in {1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 256 - Nc} against the oracle and against the general
    body (PNR_SAMPLE_PDF_GENERAL=1 routes the same call to it); and the shapes the instance refuses first (Nf = 193,
    Nc + Nf = 257; 256 - Nc > 192 below Nc = 64), where both settings of the switch run the general body."""
    wrong = []
    for Nc in range(lo, hi + 1):
        _, _, z, w = _case(Nc)
        zd, wd = T(z, dev), T(w, dev)
        nfs = sorted(set(cases.nf_inference(Nc)) | {193, 257 - Nc})
        got = {}
        for general in (False, True):
            _general(monkeypatch, general)
            got[general] = [ops.sample_pdf(zd, wd, Nf, None, want_samples=False) for Nf in nfs]
        _general(monkeypatch, False)
        for k, Nf in enumerate(nfs):
            (a, a_zs, a_inds), (b, _, _) = got[False][k], got[True][k]
            assert a_zs is None and a_inds is None
            ok = (torch.equal(a, b), np.array_equal(N_(a), _want(Nc, Nf, False)[2]))
            if not all(ok):
                wrong.append((Nc, Nf) + ok)
    assert not wrong, "Nc %s: (Nc, Nf, instance == general, instance == oracle) %s" % (sorted({c[0] for c in wrong}), wrong[:16])


# ------------------------------------------------------------------------------------------------- 3: labels in the same launch
@pytest.mark.parametrize("Nc", NC_LIST)
def test_labels_with_hit_lists_up_to_64(dev, Nc, monkeypatch):
    """ops.sample_pdf_labels at max_hits 1 / 8 / 9 / 33 / 64 with hit lists that overflow every one of them: z_fine and both label
    images against the oracle and against ops.sample_labels of the z_fine; u deterministic (for Nc <= 64 the inference instance,
    which keeps one hit per lane and broadcasts it by readlane -- and the general body through the switch) and given."""
    rays, _, z, w = _case(Nc)
    box, ids = _boxes(Nc)
    rays = rays.copy()
    rays[5::16, 0] += 1000.0                                # rays that pass far to the side: no hit
    rd, zd, wd, bd, idd = (T(a, dev) for a in (rays, z, w, box, ids))
    nfs = (2, 65, min(192, 256 - Nc) if Nc <= 64 else 512 - Nc)
    for mh in (1, 8, 9, 33, 64):
        hits = ops.bbox_hits(rd, bd, mh)
        hits_c = co.bbox_hits(rays, box, mh)
        assert all(np.array_equal(N_(a), b) for a, b in zip(hits, hits_c))
        assert (hits_c[2] > mh).any() and (hits_c[2] < mh).any(), mh          # lists that overflow, and lists that do not fill
        for Nf in nfs:
            for given in (False, True):
                zs_c, _, zf_c, u = _want(Nc, Nf, given)
                ls_c, li_c = co.sample_labels(zf_c, *hits_c, ids)
                assert (ls_c >= 0).any() and (ls_c < 0).any()
                for general in ((False, True) if not given and Nc <= 64 else (False,)):
                    _general(monkeypatch, general)
                    zf, ls, li = ops.sample_pdf_labels(zd, wd, Nf, hits, idd, T(u, dev))
                    _general(monkeypatch, False)
                    what = (Nc, Nf, mh, given, general)
                    assert np.array_equal(N_(zf), zf_c), what
                    assert np.array_equal(N_(ls), ls_c) and np.array_equal(N_(li), li_c), what
                    l2 = ops.sample_labels(zf, *hits, idd)
                    assert torch.equal(ls, l2[0]) and torch.equal(li, l2[1]), what


# ------------------------------------------------------------------------------------------------- 4: u drawn in the kernel
@pytest.mark.parametrize("Nc", NC_LIST)
def test_in_kernel_u_equals_explicit_u(dev, Nc):
    """The _rng twins (ops.Draw) against the explicit call fed ops.rng_fill's materialised uniforms: both template instances and
    the short-row sum (test_gpu_rng.py::test_sample_pdf_rng_equals_explicit has Nc = 64 and 128 on other weights)."""
    rays, _, z, w = _case(Nc)
    box, ids = _boxes(Nc + 1)
    rd, zd, wd, bd, idd = (T(a, dev) for a in (rays, z, w, box, ids))
    hits = ops.bbox_hits(rd, bd, 9)
    call = torch.tensor([77 + Nc, 2 ** 33 + 5], dtype=torch.int64, device=dev)
    base = 2 ** 32 - R                                      # the launch's global ray indices end at the last one a stream has
    for Nf in (1, 64, 65, min(192, 512 - Nc), 512 - Nc):
        u = ops.rng_fill(call, 2, base, R, Nf)
        a = ops.sample_pdf(zd, wd, Nf, ops.Draw(call, 2, base))
        b = ops.sample_pdf(zd, wd, Nf, u)
        for x, y, n in zip(a, b, ("z_fine", "z_samples", "inds")):
            assert torch.equal(x, y), (Nc, Nf, n)
        zs_c, inds_c = co.sample_pdf(z, w, Nf, N_(u))       # and the oracle on those uniforms
        assert np.array_equal(N_(a[2]), inds_c) and np.array_equal(N_(a[1]), zs_c) and np.array_equal(N_(a[0]), co.merge_sorted(z, zs_c))
        a = ops.sample_pdf_labels(zd, wd, Nf, hits, idd, ops.Draw(call, 2, base))
        b = ops.sample_pdf_labels(zd, wd, Nf, hits, idd, u)
        for x, y, n in zip(a, b, ("z_fine", "label_sem", "label_inst")):
            assert torch.equal(x, y), (Nc, Nf, n)


# ------------------------------------------------------------------------------------------------- 5: more rays than workgroups
@pytest.mark.parametrize("Nc,Nf", [(64, 128), (128, 64)])
def test_grid_stride_loop_equals_slice_launches(dev, Nc, Nf, monkeypatch):
    """The grid is capped at 32 workgroups per CU and every kernel loops `for (r = blockIdx.x; r < R; r += gridDim.x)`: with
    R = 3 x 32 x CUs + 5 a workgroup meets three or four rays, and what it keeps between them (LDS, the ascending flag, the hit
    registers) must not leak.  Rows with reversed coarse z (the bitonic fallback) are mixed at random among sorted ones, and
    sorted given u among random u, so both orders of the two paths occur in most workgroups.  The big launch must equal launches
    of its first, a middle and its last 300 rays bit for bit, and those the oracle: the inference instance with labels (the
    general body with labels at Nc = 128), the general body with given u, and the in-kernel-u twin."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    Rb, S = 3 * 32 * n_cu + 5, 300
    rng = np.random.default_rng(Nc)
    rays = cases.rays(rng, Rb)
    rays[5::16, 0] += 1000.0                                # no hit
    z = co.stratified(rays, Nc, t_rand=rng.random((Rb, Nc)).astype(np.float32))
    flip = rng.random(Rb) < 0.5
    z[flip] = z[flip, ::-1]
    w = np.tile(cases.weights(rng, 512, Nc), (Rb // 512 + 1, 1))[:Rb]
    u = rng.random((Rb, Nf)).astype(np.float32)
    srt = rng.random(Rb) < 0.5
    u[srt] = np.sort(u[srt], axis=1)
    box, ids = _boxes(Nc + 2)
    rd, zd, wd, ud, bd, idd = (T(a, dev) for a in (rays, z, w, u, box, ids))
    hits = ops.bbox_hits(rd, bd, 33)
    call = torch.tensor([4242, 9], dtype=torch.int64, device=dev)
    base = 1000003
    draw = ops.Draw(call, 2, base)
    big = {"labels": ops.sample_pdf_labels(zd, wd, Nf, hits, idd, None),
           "given": ops.sample_pdf(zd, wd, Nf, ud),
           "rng": ops.sample_pdf(zd, wd, Nf, draw)}
    u_rng = N_(ops.rng_fill(call, 2, base, Rb, Nf))
    hits_c = tuple(N_(h) for h in hits)
    for s in (0, (Rb // 2) // 7 * 7, Rb - S):
        sl = slice(s, s + S)
        zs_, ws_ = zd[sl].contiguous(), wd[sl].contiguous()
        part = {"labels": ops.sample_pdf_labels(zs_, ws_, Nf, tuple(h[sl].contiguous() for h in hits), idd, None),
                "given": ops.sample_pdf(zs_, ws_, Nf, ud[sl].contiguous()),
                "rng": ops.sample_pdf(zs_, ws_, Nf, draw.at(base + s))}
        for k in big:
            for a, b in zip(big[k], part[k]):
                assert torch.equal(a[sl], b), (k, s)
        zs_c, _ = co.sample_pdf(z[sl], w[sl], Nf)
        zf_c = co.merge_sorted(z[sl], zs_c)
        ls_c, li_c = co.sample_labels(zf_c, *(h[sl] for h in hits_c), ids)
        zf, ls, li = part["labels"]
        assert np.array_equal(N_(zf), zf_c) and np.array_equal(N_(ls), ls_c) and np.array_equal(N_(li), li_c), s
        assert (ls_c >= 0).any() and (hits_c[2][sl] > 33).any()
        for k, uu in (("given", u[sl]), ("rng", u_rng[sl])):
            zs_c, inds_c = co.sample_pdf(z[sl], w[sl], Nf, uu)
            zf, zs, inds = part[k]
            assert np.array_equal(N_(inds), inds_c) and np.array_equal(N_(zs), zs_c), (k, s)
            assert np.array_equal(N_(zf), co.merge_sorted(z[sl], zs_c)), (k, s)
    # the instance and the general body agree on the whole launch too
    _general(monkeypatch, True)
    gen = ops.sample_pdf_labels(zd, wd, Nf, hits, idd, None)
    _general(monkeypatch, False)
    for a, b in zip(big["labels"], gen):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 6: edge rays
def _both_bodies(dev, monkeypatch, z, w, Nf):
    """z_fine of the want_samples=False call through the instance it picks and through the general body; asserted equal"""
    out = []
    for general in (False, True):
        _general(monkeypatch, general)
        out.append(ops.sample_pdf(T(z, dev), T(w, dev), Nf, None, want_samples=False)[0])
    _general(monkeypatch, False)
    assert torch.equal(out[0], out[1])
    return N_(out[0])


@pytest.mark.parametrize("Nc,Nf", [(3, 1), (9, 64), (64, 128), (64, 192), (65, 100), (200, 312)])
def test_equal_coarse_depths_and_unsorted_rows(dev, Nc, Nf, monkeypatch):
    _, _, z, w = _case(Nc)
    # near == far: every depth, bin and sample of a row is the same number -- the merge is all ties
    zeq = np.repeat(z[:, :1], Nc, 1)
    zs_c, inds_c = co.sample_pdf(zeq, w, Nf)
    zf, zs, inds = ops.sample_pdf(T(zeq, dev), T(w, dev), Nf)
    assert np.array_equal(N_(inds), inds_c) and np.array_equal(N_(zs), zs_c) and np.array_equal(N_(zf), co.merge_sorted(zeq, zs_c))
    assert np.array_equal(_both_bodies(dev, monkeypatch, zeq, w, Nf), co.merge_sorted(zeq, zs_c))
    # unsorted coarse depths in some rows (reversed, and one swapped pair): the union is sorted all the same
    zu = z.copy()
    zu[::3] = zu[::3, ::-1]
    zu[1::6, [0, Nc - 1]] = zu[1::6, [Nc - 1, 0]]
    zs_c, inds_c = co.sample_pdf(zu, w, Nf)
    zf_c = co.merge_sorted(zu, zs_c)
    zf, zs, inds = ops.sample_pdf(T(zu, dev), T(w, dev), Nf)
    assert np.array_equal(N_(inds), inds_c) and np.array_equal(N_(zs), zs_c) and np.array_equal(N_(zf), zf_c)
    got = _both_bodies(dev, monkeypatch, zu, w, Nf)
    assert np.array_equal(got, zf_c) and (np.diff(got, axis=1) >= 0).all()


@pytest.mark.parametrize("Nc", [10, 18, 34, 66])
def test_samples_that_tie_with_coarse_depths(dev, Nc, monkeypatch):
    """Uniform weights over nw = Nc - 2 = 2^k bins of width 1 and Nf = 2 nw + 1 deterministic u = i / (2 nw): every quantity is exact,
    the odd samples land ON the coarse depths, the even ones on bin centres.  In the merge a coarse depth goes before the sample
    that ties with it; a rank search that counts the tie on both sides sends both to one slot and leaves another unwritten.  A
    launch on shifted depths goes first, so that an unwritten slot cannot hold the right number from the launch before."""
    nw = Nc - 2
    Nf = 2 * nw + 1
    z = (np.arange(Nc, dtype=np.float32)[None] + np.arange(2, 2 + R, dtype=np.float32)[:, None] * 3).astype(np.float32)
    w = np.full((R, Nc), 1024.0, np.float32)                # 1024 + 1e-5 rounds to 1024: the sum and the pdf = 1 / nw are exact
    zs_c, inds_c = co.sample_pdf(z, w, Nf)
    assert np.array_equal(zs_c[:, 1:-1:2], z[:, 1:-1]) and np.array_equal(zs_c[:, 2:-1:2], z[:, 1:-2] + 0.5)       # the ties, exactly
    zf_c = co.merge_sorted(z, zs_c)
    for general in (False, True):
        _general(monkeypatch, general)
        ops.sample_pdf(T(z + 1000, dev), T(w, dev), Nf, None, want_samples=False)
        zf = ops.sample_pdf(T(z, dev), T(w, dev), Nf, None, want_samples=False)[0]
        _general(monkeypatch, False)
        assert np.array_equal(N_(zf), zf_c), general
    ops.sample_pdf(T(z + 1000, dev), T(w, dev), Nf)
    zf, zs, inds = ops.sample_pdf(T(z, dev), T(w, dev), Nf)
    assert np.array_equal(N_(inds), inds_c) and np.array_equal(N_(zs), zs_c) and np.array_equal(N_(zf), zf_c)


@pytest.mark.parametrize("Nc,Nf", [(8, 5), (64, 128), (64, 192), (67, 64), (256, 256)])
def test_u_at_both_ends_of_its_range(dev, Nc, Nf):
    """given u of exactly 0 and of the largest float below 1 (what a uniform generator may return), alone and among others"""
    _, _, z, w = _case(Nc)
    u = cases.uniforms(Nc, Nf).copy()
    top = np.nextafter(np.float32(1), np.float32(0))
    u[0::4, 0] = 0.0
    u[1::4, -1] = top
    u[2::4] = 0.0
    u[3::4] = top
    zs_c, inds_c = co.sample_pdf(z, w, Nf, u)
    zf, zs, inds = ops.sample_pdf(T(z, dev), T(w, dev), Nf, T(u, dev))
    assert np.array_equal(N_(inds), inds_c) and np.array_equal(N_(zs), zs_c) and np.array_equal(N_(zf), co.merge_sorted(z, zs_c))


@pytest.mark.parametrize("Nc,Nf", [(9, 20), (64, 128), (128, 64)])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_weight_stays_in_its_row(dev, Nc, Nf, bad, monkeypatch):
    """One row with a NaN / infinite weight: the call returns and every OTHER row is what it is without it (the row itself is
    not specified)."""
    _, _, z, w = _case(Nc)
    w = w.copy()
    rows = [0, 33, R - 1]
    w[rows, Nc // 2] = bad
    keep = np.ones(R, bool)
    keep[rows] = False
    for given in (False, True):
        zs_c, inds_c, zf_c, u = _want(Nc, Nf, given)
        zf, zs, inds = ops.sample_pdf(T(z, dev), T(w, dev), Nf, T(u, dev))
        torch.cuda.synchronize()
        assert np.array_equal(N_(inds)[keep], inds_c[keep]) and np.array_equal(N_(zs)[keep], zs_c[keep])
        assert np.array_equal(N_(zf)[keep], zf_c[keep])
    for general in (False, True):
        _general(monkeypatch, general)
        zf = ops.sample_pdf(T(z, dev), T(w, dev), Nf, None, want_samples=False)[0]
        _general(monkeypatch, False)
        assert np.array_equal(N_(zf)[keep], _want(Nc, Nf, False)[2][keep])


# ------------------------------------------------------------------------------------------------- 7: nothing else is written
@pytest.mark.parametrize("Nc,Nf", [(3, 1), (9, 7), (64, 128), (63, 193), (128, 64), (256, 256)])
def test_only_z_fine_is_written(dev, Nc, Nf, monkeypatch):
    """want_samples=False into a caller-owned `out` that lies inside a larger buffer: the guard words before and after it
    survive, the inputs are unchanged, and the result is the oracle's -- for the instance the call picks, the general body, given
    u, in-kernel u and the label launch (whose label images get guards of their own kind: fresh tensors, checked whole)."""
    rays, _, z, w = _case(Nc)
    Nt = Nc + Nf
    zd, wd = T(z, dev), T(w, dev)
    box, ids = _boxes(Nc + 3)
    hits = ops.bbox_hits(T(rays, dev), T(box, dev), 8)
    hits_before = tuple(h.clone() for h in hits)
    call = torch.tensor([5, 6], dtype=torch.int64, device=dev)
    u_given = T(cases.uniforms(Nc, Nf), dev)
    u_rng = ops.rng_fill(call, 2, 0, R, Nf)

    def run(fn, want_u):
        buf = torch.full((2 * GUARD + R * Nt,), F_CANARY, device=dev)
        view = buf[GUARD:GUARD + R * Nt].view(R, Nt)
        got = fn(view)
        assert got[0].data_ptr() == view.data_ptr()
        assert (buf[:GUARD] == F_CANARY).all() and (buf[-GUARD:] == F_CANARY).all()
        zs_c, _ = co.sample_pdf(z, w, Nf, None if want_u is None else N_(want_u))
        assert np.array_equal(N_(view), co.merge_sorted(z, zs_c))
        assert torch.equal(zd, T(z, dev)) and torch.equal(wd, T(w, dev))
        return got

    for general in (False, True):
        _general(monkeypatch, general)
        got = run(lambda o: ops.sample_pdf(zd, wd, Nf, None, want_samples=False, out=o), None)
        assert got[1] is None and got[2] is None
        run(lambda o: ops.sample_pdf_labels(zd, wd, Nf, hits, T(ids, dev), None, out=o), None)
        _general(monkeypatch, False)
    u_before = u_given.clone()
    run(lambda o: ops.sample_pdf(zd, wd, Nf, u_given, want_samples=False, out=o), u_given)
    run(lambda o: ops.sample_pdf(zd, wd, Nf, ops.Draw(call, 2, 0), want_samples=False, out=o), u_rng)
    run(lambda o: ops.sample_pdf_labels(zd, wd, Nf, hits, T(ids, dev), u_given, out=o), u_given)
    assert torch.equal(u_given, u_before) and all(torch.equal(a, b) for a, b in zip(hits, hits_before))
    assert call.tolist() == [5, 6]
