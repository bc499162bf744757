"""CPU tests that pin tests/_batch_ref.py -- the numpy reference tests/test_gpu_batch.py measures pnr_sample_batch against --
with answers known in closed form, a uniformity test, and three deliberately wrong variants that the same checks must reject."""
import statistics

import numpy as np
import pytest

import _batch_ref as br
import _camera_ref as cr

SEED = 2024            # chosen on the CPU: the reference passes the uniformity test below at this seed (chi^2 printed there)
FISH = (2.2134, 0.016798, 1.6548, 1336.3 * 24 / 1400, 1335.8 * 24 / 1400, 11.5, 7.5)       # the KITTI-360-shaped lens at 24 x 16


def small_pool():
    """3 frames of 24 x 16: a pinhole, a fisheye (lens + a user mask: the corners and a block are not drawable), a pinhole"""
    g = np.random.default_rng(5)
    W, H = 24, 16
    img = lambda: g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = np.ones((H, W), bool)
    mask[10:, :7] = False
    pose = cr.pose(0.3, 0.1, (1.0, 1.5, -2.0))
    return [br.ref_frame("pinhole", (20.0, 20.0, 11.5, 7.5), W, H, pose, 0.5, 50.0, img()),
            br.ref_frame("fisheye", FISH, W, H, cr.pose(1.2), 0.5, 50.0, img(), mask=mask),
            br.ref_frame("pinhole", (20.0, 20.0, 11.5, 7.5), W, H, cr.pose(-0.4), 0.5, 50.0, img())]


# ------------------------------------------------------------------------------------------------ the checks (variant: what to test)
def check_extremes(variant=None):
    """W = 0 draws index 0, W = 2^64 - 1 draws index n - 1, and the index never decreases with W"""
    for n in (1, 2, 7, 1000, 529408, 2 ** 31 + 12345, 10 ** 12):
        cum = np.array([0, n], np.int64)
        assert br.draw_one(0, cum, 0, variant=variant) == (0, 0)
        assert br.draw_one(2 ** 64 - 1, cum, 0, variant=variant) == (0, n - 1), n
        ws = sorted(int(v) for v in np.random.default_rng(n % 97).integers(0, 2 ** 63, 64)) + [2 ** 64 - 2 ** 20]
        ks = [br.draw_one(w, cum, 0, variant=variant)[1] for w in ws]
        assert ks == sorted(ks) and all(0 <= k < n for k in ks)


def _word_for(idx, n):
    """the smallest W with mulhi64(W, n) == idx"""
    return -((-idx * 2 ** 64) // n)


def check_boundaries(variant=None):
    """idx = cum[f] is the first pixel of frame f, idx = cum[f] - 1 the last pixel of the nearest non-empty frame before it"""
    cum = np.array([0, 384, 384, 600, 601, 601, 985], np.int64)        # frames 1 and 4 are empty (n_valid = 0)
    n = int(cum[-1])
    for f in (0, 2, 3, 5):
        W = _word_for(int(cum[f]), n)
        assert br.mulhi64(W, n) == cum[f] and (W == 0 or br.mulhi64(W - 1, n) == cum[f] - 1)
        assert br.draw_one(W, cum, 0, variant=variant) == (f, 0), f
        if W:
            prev = max(i for i in (0, 2, 3, 5) if i < f)
            assert br.draw_one(W - 1, cum, 0, variant=variant) == (prev, int(cum[prev + 1] - cum[prev]) - 1), f


def chi2_bound(dof, p=1e-6):
    """the 1 - p quantile of chi^2 with dof degrees of freedom (Wilson-Hilferty)"""
    z = statistics.NormalDist().inv_cdf(1.0 - p)
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * (2.0 / (9.0 * dof)) ** 0.5) ** 3


def check_uniform(variant=None, n_draws=120000):
    """every drawable pixel of the pool is drawn equally often (chi^2 over (frame, pixel) cells), no other pixel ever"""
    frames = small_pool()
    cells = {}
    for f, fr in enumerate(frames):
        for p in (range(fr["width"] * fr["height"]) if fr["valid_pix"] is None else fr["valid_pix"]):
            cells[(f, int(p))] = 0
    assert len(cells) == br.cum_of(frames)[-1] and frames[1]["valid_pix"] is not None and 100 < len(frames[1]["valid_pix"]) < 384
    fo, po = br.draw(frames, SEED, 0, n_draws, 0, variant=variant)
    for f, p in zip(fo.tolist(), po.tolist()):
        assert (f, p) in cells, "a pixel outside the drawable set was drawn: frame %d pixel %d" % (f, p)
        cells[(f, p)] += 1
    exp = n_draws / len(cells)
    chi2 = sum((c - exp) ** 2 / exp for c in cells.values())
    dof = len(cells) - 1
    print("chi^2 = %.1f at %d degrees of freedom, bound %.1f" % (chi2, dof, chi2_bound(dof)))
    assert chi2 < chi2_bound(dof), (chi2, dof)


# ------------------------------------------------------------------------------------------------ the reference passes them
def test_extremes_and_monotone():
    check_extremes()


def test_frame_boundaries_and_empty_frames():
    check_boundaries()
    # a frame with n_valid = 0 is never chosen, wherever it stands
    cum = np.array([0, 0, 5, 5, 5, 9, 9], np.int64)
    seen = {br.draw_one(w, cum, 0)[0] for w in br.words64(3, 0, br.TAG_PIXEL, 0, 4000)}
    assert seen == {1, 4}
    assert br.draw_one(123, np.array([0], np.int64), 0) == (-1, 0)                     # F = 0
    assert br.draw_one(123, np.array([0, 0, 0], np.int64), 0) == (-1, 0)               # cum[F] = 0


def test_chi2_bound_against_tabulated_quantiles():
    # chi^2 quantiles at p = 0.001 from the tables: 10 dof 29.59, 100 dof 149.45 (Wilson-Hilferty is good to ~0.1 there)
    assert abs(chi2_bound(10, 1e-3) - 29.59) < 0.3 and abs(chi2_bound(100, 1e-3) - 149.45) < 0.3


def test_uniform_over_the_pool():
    check_uniform()


def test_mode_frame_picks_one_frame_independent_of_ray_base():
    frames = small_pool()
    picked = set()
    for off in range(40):
        f0, p0 = br.draw(frames, SEED, off, 64, 1)
        f1, p1 = br.draw(frames, SEED, off, 64, 1, ray_base=64)
        assert len(set(f0.tolist())) == 1 and f0[0] == f1[0] == br.frame_of_call(SEED, off, 3)
        assert not np.array_equal(p0, p1)
        fa, pa = br.draw(frames, SEED, off, 128, 1)
        assert np.array_equal(np.concatenate([p0, p1]), pa) and np.array_equal(np.concatenate([f0, f1]), fa)
        if frames[f0[0]]["valid_pix"] is not None:
            assert np.isin(p0, frames[f0[0]]["valid_pix"]).all()
        picked.add(int(f0[0]))
    assert picked == {0, 1, 2}


@pytest.mark.parametrize("mode", [0, 1])
def test_rank_batches_concatenate_to_the_large_batch(mode):
    frames = small_pool()
    for fr in frames:
        g = np.random.default_rng(fr["width"])
        fr["depth"] = g.random((16, 24), dtype=np.float32) * 30
    frames[0]["sem"] = np.arange(384, dtype=np.int16).reshape(16, 24) % 7 - 1
    R = 50
    whole = br.sample(frames, 9, 4, 4 * R, mode)
    parts = [br.sample(frames, 9, 4, R, mode, ray_base=rank * R) for rank in range(4)]
    for k, v in whole.items():
        assert np.array_equal(np.concatenate([p[k] for p in parts]), v), k
    assert (whole["sem"][whole["frame"] != 0] == -1).all() and (whole["inst"] == -1).all()
    assert not np.array_equal(br.sample(frames, 9, 5, 4 * R, mode)["pix"], whole["pix"])          # the next offset: another batch


def test_targets_are_the_drawn_pixels():
    frames = small_pool()
    out = br.sample(frames, 1, 0, 300, 0)
    for r in range(300):
        fr = frames[out["frame"][r]]
        j, i = divmod(int(out["pix"][r]), fr["width"])
        assert np.array_equal(out["rgb"][r], fr["rgb"][j, i].astype(np.float32) / np.float32(255))
        assert np.array_equal(out["rays"][r, :3], fr["c2w"][:, 3]) and out["rays"][r, 6] == np.float32(0.5)
    assert out["rgb"].max() <= 1.0 and (out["depth"] == 0).all()


# ------------------------------------------------------------------------------------------------ wrong variants are rejected
def test_corrupted_variants_fail():
    with pytest.raises(AssertionError):
        check_extremes("mod_low_word")             # idx = (low word of W) mod n: 2^64 - 1 does not land on n - 1
    with pytest.raises(AssertionError):
        check_boundaries("frame_off_by_one")       # idx = cum[f] resolved to the frame before
    with pytest.raises(AssertionError):
        check_uniform("pix_is_k")                  # valid_pix[k] read as k: masked pixels are drawn, drawable ones never
    check_boundaries("pix_is_k")                   # (each variant breaks what it is aimed at, not everything)
    check_extremes("frame_off_by_one")
