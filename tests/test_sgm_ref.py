"""CPU tests of tests/_sgm_ref.py, the reference of the stereo-matching rule (include/pnr.h "stereo matching"): its two
restatements agree, closed forms worked by hand hold, deliberately wrong variants of the rule fail them, and the rule matches
random-dot stereograms well enough to be worth building.  No GPU and no library call here.

Two of the closed forms the rule admits only in a narrower shape than first meets the eye, both by arithmetic:
  * den = 0 cannot occur at an interior d*: ties go to the lowest d, so S(d* - 1) > best strictly and den >= S(d* - 1) - best
    > 0.  The reference still guards it; the nearest reachable case, S(d* + 1) = best, is the offset's upper end, +8.
  * a right image that is the left shifted by d0 matches at d* = d0 with best = 0, but S(d0 - 1) and S(d0 + 1) are sums of
    unrelated Hamming costs, so on random texture the sub-pixel offset is a few sixteenths, not 0 (it was -5 .. 6 on the pair
    below).  The closed form is d* = d0: |d16 - 16 d0| <= 8, every pixel valid."""
import numpy as np
import pytest

import _sgm_ref as R
from panopticnerf_amd import synthetic


def _rand_pair(rng, H, W, shift=None):
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if shift:
        right[:, :W - shift] = left[:, shift:]
    return left, right


# ---------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("shape", [(1, 1, 16), (2, 3, 16), (5, 7, 16), (9, 12, 16), (4, 20, 32)])
def test_restatements_agree(shape, paths):
    H, W, D = shape
    rng = np.random.default_rng(H * 100 + W + paths)
    for shift, p1, p2, uniq, lr in ((None, 1, 1, 0, 0), (2, 10, 120, 5, 1), (3, 192, 192, 15, -1), (1, 3, 20, 99, 2)):
        left, right = _rand_pair(rng, H, W, shift if shift is not None and shift < W else None)
        a = R.sgm(left, right, D, p1, p2, paths, uniq, lr)
        cl, cr, S, d16, dR = R.loop_sgm(left, right, D, p1, p2, paths, uniq, lr)
        assert np.array_equal(a["census_l"].view(np.uint64), np.array(cl, dtype=np.uint64))
        assert np.array_equal(a["census_r"].view(np.uint64), np.array(cr, dtype=np.uint64))
        assert np.array_equal(a["S"], np.array(S, dtype=np.uint16))
        assert np.array_equal(a["disp_right"], np.array(dR, dtype=np.int16))
        assert np.array_equal(a["d16"], np.array(d16, dtype=np.int16))


# ---------------------------------------------------------------- closed forms (each takes the variant of the rule to check)
def cf_census_constant(v):
    assert not R.census(np.full((8, 11), 77, dtype=np.uint8), v).any()
    assert np.array_equal(R.census(np.zeros((1, 1), dtype=np.uint8), v), np.zeros((1, 1), dtype=np.int64))


def cf_census_ramp(v):
    img = np.tile(np.arange(20, dtype=np.uint8) * 3, (9, 1))            # img[y, x] = 3 x
    w = R.census(img, v).view(np.uint64)
    # neighbours left of the centre are smaller: rows of 1111 00000, the centre row without its centre 1111 0000
    word = int("111100000" * 3 + "11110000" + "111100000" * 3, 2)
    assert word < 1 << 62
    assert (w[:, 1:] == np.uint64(word)).all()      # the clamped columns left of the image repeat column 0, still smaller
    assert (w[:, 0] == 0).all()                     # nothing is smaller than column 0
    # a vertical ramp: the three rows above are smaller (27 bits), nothing else
    wv = R.census(np.ascontiguousarray(img.T), v).view(np.uint64)
    assert (wv[1:, :] == np.uint64(((1 << 27) - 1) << 35)).all() and (wv[0] == 0).all()


def cf_identical(v):
    rng = np.random.default_rng(3)
    for img in (rng.integers(0, 256, (7, 40), dtype=np.uint8), np.full((5, 40), 9, dtype=np.uint8)):
        for paths in (4, 8):
            a = R.sgm(img, img, 16, paths=paths, variant=v)
            assert not a["d16"].any() and not a["disp_right"].any()
            assert not a["S"][:, :, 0].any()


def cf_shift(v):
    rng = np.random.default_rng(1)
    H, W, D, d0 = 12, 64, 16, 5
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = np.roll(left, -d0, axis=1)              # right[x] = left[x + d0], wrapping
    a = R.sgm(left, right, D, paths=8, variant=v)
    inner = slice(d0 + 4, W - 4)                    # the census windows of both pixels clear of the border and the seam
    assert (np.abs(a["d16"][:, inner].astype(np.int32) - 16 * d0) <= 8).all()
    assert (R.cost(a["census_l"], a["census_r"], D)[:, inner, d0] == 0).all()
    assert (a["disp_right"][:, 4:W - d0 - 4] == d0).all()


def cf_path(v):
    C = np.array([[[3, 1, 4, 2], [5, 0, 6, 1], [2, 7, 1, 3]]], dtype=np.int32)          # (1, 3, 4)
    want = np.array([[[3, 1, 4, 2], [6, 0, 7, 2], [3, 7, 2, 5]]], dtype=np.int32)       # P1 = 1, P2 = 3, worked by hand:
    # x = 1: m = 1;  d0: 5 + min(3, 1+1, 1+3) - 1 = 6;  d1: 0 + min(1, 3+1, 4+1, 4) - 1 = 0;  d2: 6 + min(4, 1+1, 2+1, 4) - 1 = 7;
    #        d3: 1 + min(2, 4+1, 4) - 1 = 2
    # x = 2: m = 0;  d0: 2 + min(6, 0+1, 3) = 3;  d1: 7 + min(0, ...) = 7;  d2: 1 + min(7, 0+1, 2+1, 3) = 2;  d3: 3 + min(2, 7+1, 3) = 5
    assert np.array_equal(R.path_costs(C, 0, 1, 1, 3, v), want)
    assert np.array_equal(R.path_costs(C[:, ::-1], 0, -1, 1, 3, v), want[:, ::-1])
    col = np.ascontiguousarray(C.transpose(1, 0, 2))                                    # the same costs down a column
    assert np.array_equal(R.path_costs(col, 1, 0, 1, 3, v), want.transpose(1, 0, 2))
    assert np.array_equal(R.path_costs(col, 1, 1, 1, 3, v), col)                        # a diagonal never has a predecessor here


def _volume(rows, W=24, D=16, fill=1000):
    """(len(rows), W, D): row y holds the planted cells {(x, d): value} over `fill`"""
    S = np.full((len(rows), W, D), fill, dtype=np.uint16)
    for y, cells in enumerate(rows):
        for (x, d), val in cells.items():
            S[y, x, d] = val
    return S


def cf_subpixel(v):
    rows = [
        {(10, 5): 100, (10, 4): 150, (10, 6): 150},         # symmetric: 0
        {(10, 5): 100, (10, 4): 200, (10, 6): 120},         # den 120, num 640: floor(1400 / 240) = 5
        {(10, 5): 100, (10, 4): 120, (10, 6): 200},         # num -640: floor(-1160 / 240) = -5 (truncation gives -4)
        {(10, 5): 100, (10, 4): 130, (10, 6): 100},         # a tie above: d* = 5, den 30, num 240: floor(510 / 60) = 8, the upper end
        {(10, 5): 100, (10, 4): 101, (10, 6): 1000},        # den 901, num -7192: floor(-13483 / 1802) = -8, the lower end
        {(10, 0): 100, (10, 1): 101},                       # d* = 0: no offset
        {(20, 15): 100, (20, 14): 101},                     # d* = D - 1: no offset
        {(10, 5): 100, (10, 4): 160, (10, 6): 120},         # den 80, num 320: 720 / 160 = 4.5 -> 4
        {(10, 5): 100, (10, 4): 120, (10, 6): 160},         # -560 / 160 = -3.5 -> -4
        {(10, 5): 100, (10, 8): 100},                       # a tie: the lowest d
    ]
    d16, _ = R.select(_volume(rows), 0, -1, v)
    got = [int(d16[y, 20 if y == 6 else 10]) for y in range(len(rows))]
    assert got == [80, 85, 75, 88, 72, 0, 240, 84, 76, 80], got


def cf_uniqueness(v):
    rows = [
        {(10, 5): 95, (10, 4): 96, (10, 6): 96, (10, 9): 100},      # 100 * 95 = 95 * 100: equality passes; d* +- 1 never count
        {(10, 5): 96, (10, 4): 97, (10, 6): 97, (10, 9): 100},      # 9500 < 9600: not unique
        {(10, 5): 96, (10, 4): 97, (10, 6): 97, (10, 9): 102},      # 9690 >= 9600: unique
    ]
    d16, _ = R.select(_volume(rows, fill=2000), 5, -1, v)
    assert [int(d16[y, 10]) >= 0 for y in range(3)] == [True, False, True]
    assert int(d16[1, 10]) == -2
    d16, _ = R.select(_volume(rows, fill=2000), 0, -1, v)           # uniqueness 0: second < best never holds
    assert all(int(d16[y, 10]) >= 0 for y in range(3))


def cf_left_right(v):
    rows = [
        {(10, 5): 100, (11, 6): 50},        # dR(5) = 6: |6 - 5| = 1
        {(10, 5): 100, (12, 7): 50},        # dR(5) = 7: |7 - 5| = 2
        {(10, 5): 100},                     # dR(5) = 5
        {(10, 5): 100, (12, 7): 100},       # a tie in the right image's minimum: the lowest k, dR(5) = 5
    ]
    S = _volume(rows)
    assert int(R.select(S, 0, 0, v)[1][3, 5]) == 5 and int(R.select(S, 0, 0, v)[0][3, 10]) == 80
    for tol, want in ((1, [True, False, True]), (2, [True, True, True]), (0, [False, False, True]), (-1, [True, True, True])):
        d16, dR = R.select(S, 0, tol, v)
        assert [int(dR[y, 5]) for y in range(3)] == [6, 7, 5]
        assert [int(d16[y, 10]) == 80 for y in range(3)] == want, tol
        assert all(int(d16[y, 10]) in (80, -3) for y in range(3))


def cf_code_order(v):
    rows = [
        {(2, 5): 100, (2, 9): 100},                         # no right pixel AND not unique: -1
        {(10, 5): 100, (10, 9): 100, (12, 7): 50},          # not unique AND left-right: -2
        {(10, 5): 100, (12, 7): 50},                        # left-right alone: -3
        {(2, 5): 100, (4, 7): 50},                          # no right pixel AND (would-be) left-right: -1
    ]
    d16, _ = R.select(_volume(rows), 5, 1, v)
    assert [int(d16[0, 2]), int(d16[1, 10]), int(d16[2, 10]), int(d16[3, 2])] == [-1, -2, -3, -1]


def cf_depth(v):
    d16 = np.array([40, 3, 16, 15, 1600, 1601, 0, -1, -2, -3, 1], dtype=np.int16)
    z = R.depth(d16, 100.0, 1.0, 100.0)
    # 100 / 2.5; 100 / 0.1875 > d_max; 100 / 1 = d_max stays; 100 / 0.9375 > d_max; 100 / 100 = d_min stays; 100 / 100.0625 < d_min
    assert z.dtype == np.float32 and z.tolist() == [40.0, 0.0, 100.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    z = R.depth(d16, 100.0, 1e-3, np.inf)
    assert z[1] == np.float32(1600.0 / 3.0) and z[10] == np.float32(1600.0) and z[5] == np.float32(100.0 / 100.0625)
    assert z[6:10].tolist() == [0.0] * 4
    fb = np.float32(552.554261) * np.float32(0.6)           # the multiply is float32, and so is the division
    assert R.depth(np.array([7 * 16 + 3], dtype=np.int16), fb, 1e-3, np.inf)[0] == fb / np.float32(7.1875)


CLOSED_FORMS = (cf_census_constant, cf_census_ramp, cf_identical, cf_shift, cf_path, cf_subpixel, cf_uniqueness, cf_left_right,
                cf_code_order, cf_depth)


@pytest.mark.parametrize("form", CLOSED_FORMS, ids=lambda f: f.__name__)
def test_closed_form(form):
    form(None)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_corrupted_variant_fails_a_closed_form(variant):
    failed = []
    for form in CLOSED_FORMS:
        try:
            form(variant)
        except AssertionError:
            failed.append(form.__name__)
    assert failed, "the closed forms cannot tell %r from the rule" % variant


def test_variants_cover_the_required_five():
    assert {"census_le", "no_minus_m", "swap_p", "ties_high", "trunc_div"} <= set(R.VARIANTS)


# ---------------------------------------------------------------- quality on stereograms
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(96, 160, 32), (64, 128, 64)])
def test_stereogram_quality(shape, seed, paths):
    H, W, D = shape
    left, right, truth, visible = (t.numpy() for t in synthetic.stereo_pair(H, W, seed=seed))
    d16 = R.sgm(left, right, D, paths=paths)["d16"]
    valid = d16 >= 0
    good = valid & (np.abs(d16 / 16.0 - truth) <= 1.0)
    hit = (good & visible).sum() / visible.sum()
    miss = (valid & ~good).sum() / valid.sum()
    print("stereogram %s seed %d paths %d: %.4f of the visible pixels within one pixel, %.4f of the valid pixels off" % (shape, seed, paths, hit, miss))
    assert hit >= 0.94
    assert miss <= 0.025


def test_stereo_pair_is_a_stereogram():
    left, right, truth, visible = (t.numpy() for t in synthetic.stereo_pair(40, 80, seed=4))
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and visible.dtype == bool and truth.dtype == np.int32
    assert set(np.unique(truth)) == {5, 17}
    ys, xs = np.nonzero(visible)
    assert (right[ys, xs - truth[ys, xs]] == left[ys, xs]).all()
    assert not visible[:, :5].any() and visible.mean() > 0.8
    again = synthetic.stereo_pair(40, 80, seed=4)
    assert np.array_equal(again[1].numpy(), right)
    with pytest.raises(ValueError):
        synthetic.stereo_pair(8, 8, layers=((9, None), (3, (0.2, 0.8, 0.2, 0.8))))
