"""GPU tests of SURVEY.md 8f rank 4: label post-processing and the evaluator counters, bit-exact with oracle/np_oracle.py."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import np_oracle as no
from panopticnerf_amd import _lib, ops
from panopticnerf_amd.evaluate import Evaluator

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,C,K", [(1, 2, 0), (1000, 45, 32), (70001, 19, 7)])
def test_panoptic_labels_bit_exact(dev, R, C, K):
    g = torch.Generator().manual_seed(R)
    sem = torch.randn(R, C, generator=g)
    sem[::7] = sem[::7].round()                       # ties: lowest index wins
    inst = torch.randn(R, K, generator=g).round() if K else None
    # NaN logits never win and never hide a later column of the same lane (columns c and c + 16 share a lane): ADVICE r3
    sem[1::11, 0] = float("nan")
    if C > 16:
        sem[3::13, 2] = float("nan")
        sem[3::13, 18] = 50.0                         # the row maximum sits 16 columns behind a NaN
    sem[5::17] = float("nan")                         # rows without any number: index 0
    if K:
        inst[2::9, 0] = float("nan")
    thing = (torch.arange(C) % 3 == 0).int()
    sl, il, pan = ops.panoptic_labels(sem.to(dev), None if inst is None else inst.to(dev), thing.to(dev))
    rs, ri, rp = no.panoptic_labels(sem.numpy(), None if inst is None else inst.numpy(), thing.numpy())
    assert np.array_equal(sl.cpu().numpy(), rs) and np.array_equal(il.cpu().numpy(), ri) and np.array_equal(pan.cpu().numpy(), rp)
    sl2, il2, _ = ops.panoptic_labels(sem.to(dev), None if inst is None else inst.to(dev), None)      # every class a thing
    assert torch.equal(sl2, sl) and (K == 0 or (il2 >= 0).all())


def test_confusion_exact_and_accumulates(dev):
    g = torch.Generator().manual_seed(1)
    C, n = 45, 529408
    pred = torch.randint(0, C, (n,), generator=g, dtype=torch.int32)
    gt = torch.randint(-1, C + 1, (n,), generator=g, dtype=torch.int32)      # -1 and C are ignored
    conf = ops.confusion(pred.to(dev), gt.to(dev), C)
    ref = no.confusion(pred.numpy(), gt.numpy(), C)
    assert np.array_equal(conf.cpu().numpy(), ref)
    conf = ops.confusion(pred.to(dev), gt.to(dev), C, conf)                  # second frame accumulates
    assert np.array_equal(conf.cpu().numpy(), 2 * ref)
    assert ops.confusion(pred[:0].to(dev), gt[:0].to(dev), C).sum().item() == 0


def test_evaluator_psnr_miou(dev):
    g = torch.Generator().manual_seed(3)
    R, C, K = 5000, 6, 3
    ev = Evaluator(n_classes=C, is_thing=[0, 1, 0, 1, 0, 0])
    ref_conf = np.zeros((C, C), np.int64)
    psnr = []
    for f in range(3):
        rgb, gt_rgb = torch.rand(1, R, 3, generator=g), torch.rand(1, R, 3, generator=g)
        sem, inst = torch.randn(1, R, C, generator=g), torch.randn(1, R, K, generator=g)
        lab = torch.randint(-1, C, (1, R), generator=g)
        out = {"rgb_1": rgb.to(dev), "semantic_1": sem.to(dev), "instance_1": inst.to(dev)}
        res = ev.evaluate(out, {"rgb": gt_rgb.to(dev), "pseudo_label": lab.to(dev)})
        sl, il, pan = no.panoptic_labels(sem[0].numpy(), inst[0].numpy(), np.array([0, 1, 0, 1, 0, 0]))
        assert np.array_equal(res["panoptic_id"].cpu().numpy(), pan)
        ref_conf += no.confusion(sl, lab[0].numpy(), C)
        psnr.append(-10 * np.log10(((rgb - gt_rgb).double() ** 2).mean().item()))
    s = ev.summarize()
    tp = np.diag(ref_conf).astype(float)
    union = ref_conf.sum(0) + ref_conf.sum(1) - tp
    assert abs(s["psnr"] - np.mean(psnr)) < 1e-4
    assert abs(s["miou"] - np.mean(tp / union)) < 1e-12 and abs(s["pixel_acc"] - tp.sum() / ref_conf.sum()) < 1e-12
    assert ev.summarize() == {}                       # counters reset


def test_panoptic_quality_matches_oracle(dev):
    """PQ terms of the evaluator (pnr_confusion over compact segment ids + tensor ops) vs plain segment loops."""
    g = torch.Generator().manual_seed(9)
    C, K, H, W = 5, 4, 40, 60
    thing = [0, 1, 1, 0, 0]        # class 0 is stuff: id = class*1000 + instance cannot tell a class-0 thing from a stuff class
    ev = Evaluator(NS(num_classes=C, num_instances=K), is_thing=thing)
    ref = np.zeros((C, 4))
    for f in range(3):
        # blocky ground truth and a prediction that agrees on most of it
        gt_sem = torch.randint(0, C, (H // 10, W // 10), generator=g).repeat_interleave(10, 0).repeat_interleave(10, 1)
        gt_ins = torch.randint(0, K, (H // 10, W // 10), generator=g).repeat_interleave(10, 0).repeat_interleave(10, 1)
        th = torch.tensor(thing)[gt_sem] != 0
        if f == 2:
            gt_ins = gt_ins * 37 + 500        # arbitrary, large ground-truth instance indices (KITTI-360 style): ids are re-mapped per frame
        gt_pan = torch.where(th, gt_sem * 1000 + gt_ins, gt_sem)
        gt_pan[:3] = -1                                                  # an ignored band
        noise = torch.rand(H, W, generator=g) < 0.25
        sem_logits = torch.nn.functional.one_hot(torch.where(noise, torch.randint(0, C, (H, W), generator=g), gt_sem), C).float() * 5
        ins_logits = torch.nn.functional.one_hot(torch.where(noise, torch.randint(0, K, (H, W), generator=g), gt_ins % 37 % K if f == 2 else gt_ins), K).float() * 5
        out = {"rgb_1": torch.zeros(1, H * W, 3, device=dev), "semantic_1": sem_logits.reshape(1, -1, C).to(dev),
               "instance_1": ins_logits.reshape(1, -1, K).to(dev)}
        res = ev.evaluate(out, {"panoptic_gt": gt_pan.reshape(1, -1).to(dev)})
        ref += no.panoptic_quality_terms(res["panoptic_id"].cpu().numpy(), gt_pan.reshape(-1).numpy(), C)
    got = ev.pq.cpu().numpy()
    assert np.allclose(got, ref, atol=1e-9), (got, ref)
    s = ev.summarize()
    den = ref[:, 1] + 0.5 * ref[:, 2] + 0.5 * ref[:, 3]
    assert abs(s["pq"] - np.mean(ref[den > 0, 0] / den[den > 0])) < 1e-12



def test_out_of_range_panoptic_ids_go_to_the_overflow_row_and_reset(dev):
    """A ground-truth segment whose class index is >= n_classes is counted in NO real class (it lands in an overflow row that
    is dropped), summarize() reports it -- and resets every accumulator before raising, so the next frame set starts clean
    (the ids used to be clamped into class C-1 and the polluted table survived the exception)."""
    C, K, H, W = 4, 3, 20, 30
    ev = Evaluator(NS(num_classes=C, num_instances=K), is_thing=[0, 1, 1, 0])
    sem = torch.nn.functional.one_hot(torch.randint(0, C, (H * W,), generator=torch.Generator().manual_seed(3)), C).float()[None] * 5
    ins = torch.zeros(1, H * W, K)
    out = {"rgb_1": torch.zeros(1, H * W, 3, device=dev), "semantic_1": sem.to(dev), "instance_1": ins.to(dev)}
    res = ev.evaluate(out, {})
    good = res["panoptic_id"].clone().reshape(1, -1)
    ev.summarize()
    # the same frame twice: once with a clean ground truth, once with a band of class-index 7 (>= C) segments
    ev.evaluate(out, {"panoptic_gt": good})
    clean = ev.pq.clone()
    ev.summarize()
    bad = good.clone()
    bad[:, : 5 * W] = 7 * 1000 + 1
    ev.evaluate(out, {"panoptic_gt": bad})
    # exactly the terms of a table with room for class 7, cut back to the real classes: the segment took no real row
    want = no.panoptic_quality_terms(res["panoptic_id"].cpu().numpy(), bad.reshape(-1).cpu().numpy(), 8)[:C]
    assert np.allclose(ev.pq.cpu().numpy(), want, atol=1e-9), (ev.pq, want)
    with pytest.raises(ValueError, match="class index"):
        ev.summarize()
    assert ev.pq is None and ev._bad_ids is None and ev.summarize() == {}      # reset although it raised
    ev.evaluate(out, {"panoptic_gt": good})
    assert torch.equal(ev.pq, clean)                                           # and the next accumulation is unpolluted


# ------------------------------------------------------------------------------------------------------------------------
# Sweeps: pnr_argmax16's 16 lanes stride over the classes like the loss kernels' do, so every class count, every winning lane
# and stride step, the special values of a float comparison, the tail of the ray loop and every NULL output get a case of their
# own; pnr_confusion runs both of its kernels at every edge of its class and pixel counts, with labels outside [0, n) on both
# sides.  Everything is integer work: bit for bit against oracle/np_oracle.py.
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
K_CYCLE = (0, 1, 15, 16, 17, 33)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _labels_equal(dev, sem, inst, thing):
    got = ops.panoptic_labels(torch.tensor(sem).to(dev), None if inst is None else torch.tensor(inst).to(dev),
                              None if thing is None else torch.tensor(thing).to(dev))
    ref = no.panoptic_labels(sem, inst, thing)
    return [name for name, a, b in zip(("sem_label", "inst_label", "panoptic"), got, ref) if not np.array_equal(a.cpu().numpy(), b)]


def test_panoptic_labels_every_class_count(dev):
    """C = 1 .. 130 x K in {0, 1, 15, 16, 17, 33}: ties on rounded rows, R = 37 (9 lane groups and a tail)"""
    rng = np.random.default_rng(0)
    bad = []
    for C in range(1, 131):
        for K in K_CYCLE:
            sem = rng.normal(size=(37, C)).astype(np.float32)
            sem[::3] = sem[::3].round()
            inst = rng.normal(size=(37, K)).round().astype(np.float32) if K else None
            thing = (np.arange(C) % 3 != 1).astype(np.int32)
            bad += [(C, K, n) for n in _labels_equal(dev, sem, inst, thing)]
    assert not bad, bad[:20]


@pytest.mark.parametrize("tie", [False, True])
def test_panoptic_labels_planted_maximum_in_every_column(dev, tie):
    """R = C rows, row i has its maximum at column i: every lane and every stride step wins once.  tie: the same value again at a
    higher column, which must lose."""
    rng = np.random.default_rng(1 + tie)
    for C in range(1, 131):
        maps = []
        for _ in range(2):
            m = -1.0 - rng.random((C, C)).astype(np.float32)
            m[np.arange(C), np.arange(C)] = 5.0
            if tie:
                for i in range(C - 1):
                    m[i, rng.integers(i + 1, C)] = 5.0
            maps.append(m)
        sl, il, pan = ops.panoptic_labels(torch.tensor(maps[0]).to(dev), torch.tensor(maps[1]).to(dev), None)
        want = np.arange(C, dtype=np.int32)
        assert np.array_equal(sl.cpu().numpy(), want) and np.array_equal(il.cpu().numpy(), want), C
        assert np.array_equal(pan.cpu().numpy(), want * 1001) and not _labels_equal(dev, maps[0], maps[1], None), C


def test_panoptic_labels_special_values(dev):
    """+0.0 and -0.0 compare equal (lowest index); +-inf; a row of all -inf gives index 0, like a row of all NaN"""
    C = 40
    inf = np.float32(np.inf)
    rows, want = [], []
    def row(fill, at=(), expect=0):       # noqa: E306
        r = np.full(C, fill, np.float32)
        for c, v in at:
            r[c] = v
        rows.append(r)
        want.append(expect)
    row(-0.0, [(5, 0.0)], 0)                                  # +0.0 does not beat the -0.0 before it
    row(0.0, [(0, -1.0), (17, -0.0)], 1)
    row(-1.0, [(21, -0.0), (38, 0.0)], 21)
    row(1.0, [(33, inf)], 33)
    row(1.0, [(33, inf), (16, inf)], 16)                      # two +inf: the lower column (lane 0, second step, against lane 1)
    row(-inf, [], 0)                                          # all -inf: index 0
    row(-inf, [(39, -3e38)], 39)                              # anything beats -inf
    row(-inf, [(0, np.nan), (16, np.nan), (32, -inf)], 0)     # NaN reads as -inf: still all equal
    row(np.nan, [(23, -inf)], 0)                              # -inf does not beat a NaN read as -inf
    row(np.nan, [(23, -inf), (24, -1.0)], 24)
    row(inf, [(0, np.nan)], 1)
    row(3e38, [(7, -inf), (0, -3e38)], 1)
    sem = np.stack(rows)
    sl, il, pan = ops.panoptic_labels(torch.tensor(sem).to(dev), torch.tensor(sem[::-1].copy()).to(dev), None)
    assert sl.cpu().tolist() == want and il.cpu().tolist() == want[::-1]
    assert not _labels_equal(dev, sem, sem[::-1].copy(), (np.arange(C) % 2).astype(np.int32))


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 63, 64, 65])
def test_panoptic_labels_ray_count_tail(dev, R):
    """whole waves run the butterflies: rays past R are computed on row R - 1 and not stored"""
    rng = np.random.default_rng(R)
    sem, inst = rng.normal(size=(R, 19)).astype(np.float32), rng.normal(size=(R, 7)).astype(np.float32)
    G = 64
    buf = [torch.full((R + 2 * G,), -77, device=dev, dtype=torch.int32) for _ in range(3)]
    s, i = torch.tensor(sem).to(dev), torch.tensor(inst).to(dev)
    thing = (torch.arange(19) % 2).int().to(dev)
    _lib.check(_lib.load().pnr_panoptic_labels(_p(s), _p(i), _p(thing), R, 19, 7, *(_p(b[G:]) for b in buf), None), "pnr_panoptic_labels")
    torch.cuda.synchronize()
    for b, ref in zip(buf, no.panoptic_labels(sem, inst, thing.cpu().numpy())):
        assert np.array_equal(b[G:G + R].cpu().numpy(), ref) and (b[:G] == -77).all() and (b[G + R:] == -77).all()


def test_panoptic_labels_output_subsets_and_is_thing(dev):
    """every subset of the three outputs NULL, through the C entry point, between guards; is_thing all zero, all one, NULL"""
    rng = np.random.default_rng(5)
    R, C, K, G = 203, 21, 17, 64
    sem, inst = rng.normal(size=(R, C)).astype(np.float32), rng.normal(size=(R, K)).astype(np.float32)
    s, i = torch.tensor(sem).to(dev), torch.tensor(inst).to(dev)
    lib = _lib.load()
    for name, thing in (("zero", np.zeros(C, np.int32)), ("one", np.ones(C, np.int32)), ("null", None), ("mixed", (np.arange(C) % 2).astype(np.int32))):
        ref = no.panoptic_labels(sem, inst, thing)
        assert name != "zero" or ((ref[1] == -1).all() and np.array_equal(ref[2], ref[0]))
        assert name not in ("one", "null") or ((ref[1] >= 0).all() and np.array_equal(ref[2], ref[0] * 1000 + ref[1]))
        th = None if thing is None else torch.tensor(thing).to(dev)
        for mask in range(8):
            buf = [torch.full((R + 2 * G,), -77, device=dev, dtype=torch.int32) for _ in range(3)]
            ptr = [_p(b[G:]) if mask >> j & 1 else _p(None) for j, b in enumerate(buf)]
            _lib.check(lib.pnr_panoptic_labels(_p(s), _p(i), _p(th), R, C, K, *ptr, None), "pnr_panoptic_labels")
            torch.cuda.synchronize()
            for j, b in enumerate(buf):
                assert (b[:G] == -77).all() and (b[G + R:] == -77).all(), (name, mask, j)
                if mask >> j & 1:
                    assert np.array_equal(b[G:G + R].cpu().numpy(), ref[j]), (name, mask, j)
                else:
                    assert (b == -77).all(), (name, mask, j)
        # without an instance map (NULL, or n_inst = 0) every instance label is -1
        out = [torch.empty(R, device=dev, dtype=torch.int32) for _ in range(3)]
        _lib.check(lib.pnr_panoptic_labels(_p(s), _p(None), _p(th), R, C, 0, *(_p(o) for o in out), None), "pnr_panoptic_labels")
        assert (out[1] == -1).all() and torch.equal(out[2], out[0]) and np.array_equal(out[0].cpu().numpy(), ref[0])


def _noisy_labels(rng, n, n_classes):
    """labels in [0, n_classes) with -1, n_classes, INT_MIN, INT_MAX among them (every fourth position or so)"""
    lab = rng.integers(0, n_classes, n).astype(np.int64)
    out = np.array([-1, n_classes, INT_MIN, INT_MAX], np.int64)
    pick = rng.random(n) < 0.25
    lab[pick] = out[rng.integers(0, 4, int(pick.sum()))]
    if n >= 8:
        lab[rng.permutation(n)[:4]] = out                      # each of them at least once
    return lab.astype(np.int32)


@pytest.mark.parametrize("n_classes", [1, 2, 127, 128, 129, 1000])
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_confusion_class_and_pixel_counts(dev, n_classes, n):
    """k_confusion up to 128 classes (128: its 64 KiB LDS histogram), k_confusion_big above; labels outside [0, n) in pred AND gt"""
    rng = np.random.default_rng(n_classes * 7 + n)
    pred, gt = _noisy_labels(rng, n, n_classes), _noisy_labels(rng, n, n_classes)
    if n == 1:
        pred[:], gt[:] = n_classes - 1, n_classes - 1
    conf = ops.confusion(torch.tensor(pred).to(dev), torch.tensor(gt).to(dev), n_classes)
    ref = no.confusion(pred, gt, n_classes)
    assert ref.sum() > 0 and (n == 1 or ref.sum() < n)
    assert np.array_equal(conf.cpu().numpy(), ref)


@pytest.mark.parametrize("n_classes", [128, 129])
def test_confusion_accumulates_over_calls(dev, n_classes):
    rng = np.random.default_rng(n_classes)
    conf, ref = None, np.zeros((n_classes, n_classes), np.int64)
    for n in (4097, 70001):
        pred, gt = _noisy_labels(rng, n, n_classes), _noisy_labels(rng, n, n_classes)
        conf = ops.confusion(torch.tensor(pred).to(dev), torch.tensor(gt).to(dev), n_classes, conf)
        ref += no.confusion(pred, gt, n_classes)
        assert np.array_equal(conf.cpu().numpy(), ref)


def test_confusion_big_grid_stride(dev):
    """n = 3 * 524288 + 5 pixels at 129 classes: three trips of k_confusion_big's grid-stride loop and a tail"""
    rng = np.random.default_rng(3)
    n, n_classes = 3 * 524288 + 5, 129
    pred, gt = _noisy_labels(rng, n, n_classes), _noisy_labels(rng, n, n_classes)
    conf = ops.confusion(torch.tensor(pred).to(dev), torch.tensor(gt).to(dev), n_classes)
    assert np.array_equal(conf.cpu().numpy(), no.confusion(pred, gt, n_classes))


def test_confusion_8192_classes(dev):
    """the largest admitted label space (the segment-pair counts of PQ): its 512 MiB table stays on the device; the cells the
    pixels name hold their counts, and the table's sum says every other cell is zero (cells only ever grow)"""
    rng = np.random.default_rng(8)
    n, n_classes = 5000, 8192
    pred, gt = _noisy_labels(rng, n, n_classes), _noisy_labels(rng, n, n_classes)
    pred[:300], gt[:300] = 8191, 8191                          # the last cell, 300 times
    conf = ops.confusion(torch.tensor(pred).to(dev), torch.tensor(gt).to(dev), n_classes)
    p, g = pred.astype(np.int64), gt.astype(np.int64)
    v = (p >= 0) & (p < n_classes) & (g >= 0) & (g < n_classes)
    cell, cnt = np.unique(g[v] * n_classes + p[v], return_counts=True)
    assert int(conf.sum()) == int(v.sum()) and 300 <= int(conf[8191, 8191]) and int(conf.min()) == 0
    assert np.array_equal(conf.view(-1)[torch.tensor(cell).to(dev)].cpu().numpy(), cnt)
