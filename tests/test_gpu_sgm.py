"""GPU parity of the stereo matcher (csrc/pnr_stereo.hip) with tests/_sgm_ref.py: census words, the summed volume S, the
selection and the depth are integer arithmetic up to one correctly rounded float32 division, so every comparison is
torch.equal / array_equal -- no tolerance anywhere.  Every caller-owned output sits between canaries."""
import numpy as np
import pytest
import torch

import _sgm_ref as R
import _splat_ref as sr
from panopticnerf_amd import FrameSet, Pinhole, ops, stereo, synthetic
from panopticnerf_amd.evaluate import Evaluator

pytestmark = pytest.mark.gpu

PENALTIES = ((1, 1), (10, 120), (192, 192))
PAD = 64                # canary elements on each side: 128 bytes of int16, so the volume inside stays 32-byte aligned


def N_(t):
    return t.detach().cpu().numpy()


class Guarded:
    """a caller-owned output inside a larger buffer of a known value"""

    def __init__(self, shape, dtype, dev, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
        self.fill = fill
        self.t = self.buf[PAD:PAD + n].view(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == self.fill).all()) and bool((self.buf[-PAD:] == self.fill).all())


def pair(H, W, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full((H, W), 131, np.uint8), np.full((H, W), 131, np.uint8)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "shift" and W > 3:
        right[:, :W - 3] = left[:, 3:]
    return left, right


def gpu_census(img, dev):
    g = Guarded(img.shape, torch.int64, dev, 0x5A5A5A5A5A5A)
    out = ops.census(torch.from_numpy(img).to(dev), out=g.t)
    assert out.data_ptr() == g.t.data_ptr() and g.intact()
    return out


# ---------------------------------------------------------------- census
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 9), (8, 64), (33, 130), (376, 1408)])
def test_census(dev, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    imgs = [rng.integers(0, 256, shape, dtype=np.uint8)]
    if shape[0] <= 33:
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        imgs += [np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8),
                 rng.integers(0, 3, shape, dtype=np.uint8)]             # few levels: many equal neighbours
    for img in imgs:
        got = N_(gpu_census(img, dev))
        assert np.array_equal(got, R.census(img))
        assert (got >= 0).all() and (got < 1 << 62).all()
    assert not gpu_census(imgs[0] * 0 + 9, dev).any()


# ---------------------------------------------------------------- the volume
def check_volume(dev, H, W, D, paths, pen, kind, seed):
    left, right = pair(H, W, kind, seed)
    cl, cr = R.census(left), R.census(right)
    want = R.aggregate(cl, cr, D, pen[0], pen[1], paths)
    g = Guarded((H, W, D), torch.int16, dev, 0x5A5A)                    # garbage inside too: S need not be zeroed
    S = ops.sgm_aggregate(torch.from_numpy(cl).to(dev), torch.from_numpy(cr).to(dev), D, pen[0], pen[1], paths, out=g.t)
    assert S.data_ptr() == g.t.data_ptr()
    got = N_(S).view(np.uint16)
    assert g.intact(), (H, W, D, paths, pen, kind)
    assert np.array_equal(got, want), (H, W, D, paths, pen, kind, int((got != want).sum()))
    return S, want


@pytest.mark.parametrize("D", [16, 32, 64, 128, 256, 48, 80, 240])
def test_volume_every_shape(dev, D):
    """every W (all below D, at it and above it) x every H; both path counts on each; the penalties and the kind of pair cycle
    so that each meets each.  48, 80 and 240 leave lanes of the 16-lane row without a disparity."""
    i = 0
    for W in (1, 2, 63, 64, 65, 130):
        for H in (1, 2, 7, 33):
            for paths in (4, 8):
                for kind in (("random", "constant") if (i % 2 == 0) else ("shift",)):
                    check_volume(dev, H, W, D, paths, PENALTIES[i % 3], kind, seed=i)
                    i += 1


@pytest.mark.parametrize("pen", PENALTIES)
@pytest.mark.parametrize("paths", [4, 8])
def test_volume_every_penalty(dev, paths, pen):
    for D, (H, W) in ((16, (7, 65)), (64, (33, 63)), (128, (2, 130))):
        for kind in ("random", "constant", "shift"):
            check_volume(dev, H, W, D, paths, pen, kind, seed=D + paths)


def test_volume_strip_full_width(dev):
    """a 24 x 1408 strip at D = 128: full-width rows, 1431 diagonal start pixels"""
    check_volume(dev, 24, 1408, 128, 8, (10, 120), "shift", seed=5)


def test_volume_more_paths_than_one_grid_trip(dev):
    """more start pixels than the path kernel's capped grid (8 one-wave blocks per compute unit) holds in one trip, in both of
    its forms: four paths a wave at D = 16, one path a wave at D = 64 -- the grid-stride loop runs"""
    check_volume(dev, 3, 8300, 16, 8, (10, 120), "random", seed=6)
    check_volume(dev, 2, 2100, 64, 8, (10, 120), "shift", seed=7)


# ---------------------------------------------------------------- selection
def gpu_select(S, dev, uniq, lr_tol, want_right=True):
    H, W, D = S.shape
    d = Guarded((H, W), torch.int16, dev, 0x1234)
    r = Guarded((H, W), torch.int16, dev, 0x4321) if want_right else None
    St = S if isinstance(S, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(S).view(np.int16)).to(dev)
    d16, dR = ops.sgm_select(St, uniq, lr_tol, out=d.t, disp_right=None if r is None else r.t)
    assert d.intact() and (r is None or r.intact())
    return d16, dR


def hand_volume(D, W=40):
    """planted ties, uniqueness and left-right boundaries, minima at d = 0 and D - 1, every sub-pixel case"""
    rows = [
        {(20, 5): 100, (20, 4): 150, (20, 6): 150}, {(20, 5): 100, (20, 4): 200, (20, 6): 120}, {(20, 5): 100, (20, 4): 120, (20, 6): 200},
        {(20, 5): 100, (20, 4): 130, (20, 6): 100}, {(20, 5): 100, (20, 4): 101, (20, 6): 1000}, {(20, 0): 100, (20, 1): 101},
        {(W - 1, D - 1): 100, (W - 1, D - 2): 101}, {(20, 5): 100, (20, 4): 160, (20, 6): 120}, {(20, 5): 100, (20, 4): 120, (20, 6): 160},
        {(20, 5): 100, (20, 8): 100}, {(20, 5): 95, (20, 4): 96, (20, 6): 96, (20, 9): 100}, {(20, 5): 96, (20, 4): 97, (20, 6): 97, (20, 9): 100},
        {(20, 5): 96, (20, 9): 102}, {(20, 5): 100, (21, 6): 50}, {(20, 5): 100, (22, 7): 50}, {(20, 5): 100, (22, 7): 100},
        {(2, 5): 100, (2, 9): 100}, {(20, 5): 100, (20, 9): 100, (22, 7): 50}, {(2, 5): 100, (4, 7): 50},
        {(20, D - 1): 7, (20, 0): 7}, {(20, 15): 3, (20, 16 % D): 3}, {(5, 5): 1}, {(4, 5): 1},
    ]
    S = np.full((len(rows), W, D), 1000, dtype=np.uint16)
    for y, cells in enumerate(rows):
        for (x, d), v in cells.items():
            S[y, x, d] = v
    return S


@pytest.mark.parametrize("D", [16, 48, 128, 256])
def test_select_hand_volumes(dev, D):
    S = hand_volume(D, W=max(40, D + 8))
    for uniq, lr in ((0, -1), (5, 1), (5, 0), (0, 2), (99, 1), (15, -1)):
        want16, wantR = R.select(S, uniq, lr)
        d16, dR = gpu_select(S, dev, uniq, lr)
        assert np.array_equal(N_(d16), want16), (D, uniq, lr)
        assert np.array_equal(N_(dR), wantR)
    assert {-1, -2, -3} <= set(np.unique(R.select(S, 5, 1)[0]).tolist())
    # lr_tol = -1 with a NULL disp_right
    d16, dR = gpu_select(S, dev, 5, -1, want_right=False)
    assert dR is None and np.array_equal(N_(d16), R.select(S, 5, -1)[0])


@pytest.mark.parametrize("D", [16, 32, 80, 256])
def test_select_tied_random_volumes(dev, D):
    """volumes of a few distinct values: ties everywhere, runner-ups at and around the uniqueness boundary"""
    rng = np.random.default_rng(D)
    for H, W in ((1, 1), (3, 17), (9, 70), (2, 300)):
        for levels in (2, 6, 2041):
            S = (rng.integers(0, levels, (H, W, D)) + (95 if levels < 10 else 0)).astype(np.uint16)
            for uniq, lr in ((5, 1), (0, 0), (3, -1)):
                want16, wantR = R.select(S, uniq, lr)
                d16, dR = gpu_select(S, dev, uniq, lr)
                assert np.array_equal(N_(d16), want16), (D, H, W, levels, uniq, lr)
                assert np.array_equal(N_(dR), wantR)


def test_select_on_aggregated_volumes(dev):
    for (H, W, D), paths, kind in (((33, 130, 64), 8, "shift"), ((7, 65, 16), 4, "random"), ((33, 63, 128), 8, "shift"), ((7, 130, 48), 8, "constant")):
        S, want = check_volume(dev, H, W, D, paths, (10, 120), kind, seed=11)
        for uniq, lr in ((5, 1), (0, -1), (20, 0)):
            want16, wantR = R.select(want, uniq, lr)
            d16, dR = gpu_select(S, dev, uniq, lr)
            assert np.array_equal(N_(d16), want16) and np.array_equal(N_(dR), wantR)
        if kind == "shift":
            assert (want16 >= 0).mean() > 0.5


# ---------------------------------------------------------------- depth
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_depth(dev, n):
    rng = np.random.default_rng(n)
    special = np.array([-1, -2, -3, 0, 1, 16, 15, 1600, 1601, 4080, 40, 3], dtype=np.int16)
    d16 = rng.integers(-3, 4081, n).astype(np.int16)
    d16[:min(n, len(special))] = special[:n]
    fb = float(np.float32(552.554261) * np.float32(0.6))
    for fb_, rng_ in ((100.0, (1.0, 100.0)), (100.0, (1e-3, float("inf"))), (fb, (1e-3, float("inf"))), (fb, (0.5, 80.0))):
        g = Guarded((n,), torch.float32, dev, 7.5)
        z = ops.disparity_depth(torch.from_numpy(d16).to(dev), fb_, rng_, out=g.t)
        want = R.depth(d16, fb_, *rng_)
        assert g.intact() and np.array_equal(N_(z).view(np.uint32), want.view(np.uint32)), (n, fb_, rng_)
    if n >= len(special):       # every code and d16 = 0 give 0; both ends of the range are kept, one step outside is not
        z = N_(ops.disparity_depth(torch.from_numpy(special).to(dev), 100.0, (1.0, 100.0)))
        assert z.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 100.0, 0.0, 1.0, 0.0, 0.0, 40.0, 0.0]


# ---------------------------------------------------------------- the whole path
@pytest.fixture(scope="module")
def stereogram():
    left, right, truth, visible = synthetic.stereo_pair(64, 128, seed=1)
    want = R.sgm(left.numpy(), right.numpy(), 32)
    return left, right, truth, visible, want


def test_sgm_equals_the_reference_twice(dev, stereogram):
    left, right, truth, visible, want = stereogram
    L, Rt = left.to(dev), right.to(dev)
    a = stereo.sgm(L, Rt, max_disp=32, keep_volume=True)
    b = stereo.sgm(L, Rt, max_disp=32, keep_volume=True)
    for out in (a, b):
        assert np.array_equal(N_(out["S"]).view(np.uint16), want["S"])
        assert np.array_equal(N_(out["d16"]), want["d16"]) and np.array_equal(N_(out["disp_right"]), want["disp_right"])
        valid = want["d16"] >= 0
        assert np.array_equal(N_(out["valid"]), valid) and np.array_equal(N_(out["code"]), np.where(valid, 0, want["d16"]))
        assert np.array_equal(N_(out["disparity"]), np.where(valid, want["d16"] / 16.0, 0.0).astype(np.float32))
    good = (want["d16"] >= 0) & (np.abs(want["d16"] / 16.0 - truth.numpy()) <= 1.0) & visible.numpy()
    assert good.sum() >= 0.94 * visible.numpy().sum()
    # colour input goes through to_gray; no left-right check: no table
    rgb = torch.stack([L, L, L], -1).contiguous()
    c = stereo.sgm(rgb, Rt, max_disp=32, paths=4, lr_tol=-1)
    w4 = R.sgm(left.numpy(), right.numpy(), 32, paths=4, lr_tol=-1)
    assert c["disp_right"] is None and "S" not in c and np.array_equal(N_(c["d16"]), w4["d16"])


def test_sgm_in_a_captured_graph_follows_the_left_image(dev, stereogram):
    left, right, _, _, want = stereogram
    L, Rt = left.to(dev).clone(), right.to(dev)
    stereo.sgm(L, Rt, max_disp=32)                              # warm call: module loading is not capturable
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = stereo.sgm(L, Rt, max_disp=32, keep_volume=True)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(N_(out["d16"]), want["d16"]) and np.array_equal(N_(out["S"]).view(np.uint16), want["S"])
    edited = left.numpy().copy()
    edited[20:40, 30:90] = np.random.default_rng(9).integers(0, 256, (20, 60), dtype=np.uint8)
    L.copy_(torch.from_numpy(edited))
    g.replay()
    torch.cuda.synchronize()
    want2 = R.sgm(edited, right.numpy(), 32)
    assert not np.array_equal(want2["d16"], want["d16"])
    assert np.array_equal(N_(out["d16"]), want2["d16"]) and np.array_equal(N_(out["S"]).view(np.uint16), want2["S"])
    assert np.array_equal(N_(out["disp_right"]), want2["disp_right"])


def test_depth_from_pair_feeds_frames_and_the_evaluator(dev, stereogram):
    left, right, truth, visible, want = stereogram
    H, W = left.shape
    cam, baseline = Pinhole(120.0, 120.0, (W - 1) / 2.0, (H - 1) / 2.0, W, H), 0.6
    fb = np.float32(120.0) * np.float32(0.6)
    depth = stereo.depth_from_pair(left.to(dev), right.to(dev), cam, baseline, d_range=ops.DEPTH_RANGE, max_disp=32)
    want_depth = R.depth(want["d16"], fb, *ops.DEPTH_RANGE)         # the evaluator's default range: what it keeps, the evaluator counts
    assert np.array_equal(N_(depth).view(np.uint32), want_depth.view(np.uint32))
    assert np.array_equal(N_(stereo.depth(torch.from_numpy(want["d16"]).to(dev), cam, baseline, (2.0, 6.0))), R.depth(want["d16"], fb, 2.0, 6.0))
    # into the frame table and back out
    frames = FrameSet(dev, capacity=2)
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    rgb = torch.stack([left, left, left], -1).to(dev)
    i = frames.add(cam, c2w, 0.5, 100.0, rgb, depth=depth)
    batch = frames.frame_batch(i)
    assert torch.equal(batch["depth"][0], depth.reshape(-1))
    # the evaluator: the true depth as the prediction, the stereo depth as ground truth
    true_depth = (torch.from_numpy(np.float32(fb) / truth.numpy().astype(np.float32))).to(dev)
    ev = Evaluator()
    ev.evaluate_depth({"depth_0": true_depth}, depth)
    _, wc, _ = sr.metrics32_64(N_(true_depth), want_depth, None)
    got = ev.summarize()
    n_valid = int((want_depth > 0).sum())
    assert n_valid > 0.8 * H * W
    assert got["depth_n"] == n_valid == int(wc[0]) and got["depth_missing"] == 0
    assert got["depth_d1"] == sr.summary(np.zeros(5), wc)["depth_d1"] and got["depth_d1"] > 0.9
