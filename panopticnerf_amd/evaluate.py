"""Evaluator -- host-side mirror of the reference's evaluator (lib/evaluators/*; not in the mount,
SURVEY.md 0): `evaluate(output, batch)` per frame, `summarize()` at the end.

Per frame, on the GPU: semantic / instance / panoptic label maps from the fine-level composited maps
(pnr_panoptic_labels), the semantic confusion matrix against batch['pseudo_label' | 'semantic_gt'] (pnr_confusion,
accumulated over frames in a device int64 matrix) and the colour MSE (pnr_losses' rgb term).  `summarize()` turns those
counters into PSNR (mean over frames), mIoU / per-class IoU and pixel accuracy.  Nothing is copied to the host before
summarize()."""
import math

import torch

from . import consistency, ops
from .camera import invert_pose


class Evaluator:
    def __init__(self, cfg=None, n_classes=None, is_thing=None):
        g = lambda k, d: getattr(cfg, k, d) if cfg is not None else d
        self.n_classes = n_classes if n_classes is not None else g("num_classes", 0)
        self.is_thing = is_thing
        # panoptic id = class * 1000 + instance on things, class on stuff (KITTI-360's convention, where id 0 is 'unlabeled'):
        # a THING of class 0 would be encoded as its bare instance index and read back as the stuff class of that number
        if is_thing is not None and len(is_thing) and int(is_thing[0]):
            raise ValueError("Evaluator: class 0 cannot be a 'thing' under the class * 1000 + instance id convention (its "
                             "segments would alias stuff classes); re-index the label set so that class 0 is stuff / unlabeled")
        self.level = 1
        self.conf = None
        self.mse = []
        self.n_inst = g("num_instances", 0)
        self.pq = None          # (C, 4) device tensor: sum of matched IoUs, TP, FP, FN per class
        self._bad_ids = None    # device counter: segments whose class index was >= n_classes (reported by summarize())
        self.mc_agree = None    # (C, C) device int64: cross-view confusion [label in the source view, label in the target view]
        self.mc_stats = None    # (5) device int64: source pixels matched / nothing to reproject / left the view / unknown / occluded
        self.mc_tol = consistency.DEFAULT_TOL
        self.depth_sums = None      # (5) device float64: sums of |d|, d^2, |d|/gt, d^2/gt, (log pred - log gt)^2 (pnr_depth_metrics)
        self.depth_counts = None    # (5) device int64: compared pixels, ratio < 1.25 / 1.25^2 / 1.25^3, missing predictions
        self.geom = None            # evaluate_geometry: {"max_dist", "thresholds", "sums": [pred->gt, gt->pred] (2) float64, "counts": likewise (10) int64}

    def evaluate(self, output, batch):
        lv = self.level if f"rgb_{self.level}" in output else 0
        rgb = output[f"rgb_{lv}"].reshape(-1, 3).float().contiguous()
        dev = rgb.device
        res = {}
        if batch.get("rgb") is not None:
            gt = batch["rgb"].reshape(-1, 3).to(dev, torch.float32).contiguous()
            out, _ = ops.losses({"rgb": 1.0}, {"rgb": rgb}, {"rgb": gt}, want_grads=False)
            self.mse.append(out[0])
        if self.n_classes and f"semantic_{lv}" in output:
            sem = output[f"semantic_{lv}"].reshape(-1, self.n_classes).float().contiguous()
            inst = output.get(f"instance_{lv}")
            inst = None if inst is None else inst.reshape(-1, inst.shape[-1]).float().contiguous()
            th = None if self.is_thing is None else torch.as_tensor(self.is_thing, dtype=torch.int32, device=dev)
            res["semantic_label"], res["instance_label"], res["panoptic_id"] = ops.panoptic_labels(sem, inst, th)
            gt = batch.get("semantic_gt", batch.get("pseudo_label"))
            if gt is not None:
                self.conf = ops.confusion(res["semantic_label"], gt.reshape(-1).to(dev, torch.int32).contiguous(),
                                          self.n_classes, self.conf)
            pg = batch.get("panoptic_gt")
            if pg is not None:
                self._accumulate_pq(res["panoptic_id"], pg.reshape(-1).to(dev, torch.int32).contiguous())
        return res

    def _pair_side(self, out, view, what):
        """(camera, c2w, depth image, semantic map, valid) of one side of a pair: every check that needs no device"""
        if not hasattr(out, "keys"):
            raise ValueError("Evaluator.evaluate_pair: %s must be the dict Renderer.render_view returned" % what)
        lv = self.level if f"semantic_{self.level}" in out else 0
        if f"semantic_{lv}" not in out:
            raise ValueError("Evaluator.evaluate_pair: %s holds no semantic map" % what)
        if not isinstance(view, (tuple, list)) or len(view) not in (2, 3):
            raise ValueError("Evaluator.evaluate_pair: %s must be (camera, c2w) or (camera, c2w, maps)" % what)
        own = len(view) == 2            # the depth image comes from `out`, at the level the labels are made from
        cam, c2w, depth = consistency.view_depth((view[0], view[1], out) if own else view, what, f"depth_{lv}" if own else None)
        sem = out[f"semantic_{lv}"]
        if tuple(sem.shape) != (cam.height, cam.width, self.n_classes):
            raise ValueError("Evaluator.evaluate_pair: semantic map of %s is %s, expected (%d, %d, %d)"
                             % (what, tuple(sem.shape), cam.height, cam.width, self.n_classes))
        return cam, c2w, depth, sem, out.get("valid")

    def _pair_labels(self, side, what):
        """(camera, c2w, depth image, semantic label image with -1 where the frame sees nothing)"""
        cam, c2w, depth, sem, valid = side
        if not sem.is_cuda or not depth.is_cuda:
            raise RuntimeError("Evaluator.evaluate_pair: %s is not on the GPU (the HIP path has no CPU fallback)" % what)
        label = ops.panoptic_labels(sem.reshape(-1, self.n_classes).float().contiguous())[0]
        if valid is not None:           # render_view: the argmax of a pixel that sees nothing is class 0, not "nothing"
            label = torch.where(valid.reshape(-1).to(label.device), label, torch.full_like(label, -1))
        return cam, c2w, depth, label.reshape(cam.height, cam.width)

    def evaluate_pair(self, out_a, view_a, out_b, view_b, symmetric=True):
        """Accumulate multi-view consistency over one pair of rendered frames.  out_*: what Renderer.render_view returned
        (semantic and depth maps of the evaluated level, "valid"); view_*: (camera, c2w) of that frame, or (camera, c2w, maps)
        to take the depth image from another dict.  Every pixel of A is carried into B (pnr_reproject, tolerance self.mc_tol);
        where B sees the same surface point the two semantic labels are counted into the cross-view confusion matrix; with
        symmetric=True the same is done from B into A.  Returns the label images and the match images; counters stay on
        the device until summarize()."""
        if not self.n_classes:
            raise ValueError("Evaluator.evaluate_pair: the evaluator has no classes (n_classes = 0)")
        a, b = self._pair_side(out_a, view_a, "view_a"), self._pair_side(out_b, view_b, "view_b")
        a, b = self._pair_labels(a, "view_a"), self._pair_labels(b, "view_b")
        if a[2].device != b[2].device:
            raise ValueError("Evaluator.evaluate_pair: view_a is on %s, view_b on %s" % (a[2].device, b[2].device))
        dev = a[2].device
        if self.mc_agree is None:
            self.mc_agree = torch.zeros((self.n_classes, self.n_classes), device=dev, dtype=torch.int64)
            self.mc_stats = torch.zeros((5,), device=dev, dtype=torch.int64)
        res = {"semantic_label_a": a[3], "semantic_label_b": b[3]}
        for name, (s, t) in (("match_ab", (a, b)), ("match_ba", (b, a)))[: 2 if symmetric else 1]:
            m = ops.reproject(s[0], s[1], s[2], t[0], invert_pose(t[1]), t[2], tol=self.mc_tol, label_src=s[3], label_tgt=t[3],
                              n_classes=self.n_classes, agree=self.mc_agree, stats=self.mc_stats)["match"]
            res[name] = m.reshape(s[0].height, s[0].width)
        return res

    def evaluate_depth(self, output, depth_gt, valid=None, level=None, d_range=ops.DEPTH_RANGE):
        """Accumulate depth-error terms of a rendered depth image against a ground-truth depth image of the same shape and
        convention (e.g. a LiDAR scan through pointcloud.splat: z-depth in a pinhole frame, range otherwise), on the device
        (ops.depth_metrics; the rule is in include/pnr.h "point splatting").  output: what Renderer.render_view returned;
        the depth image is depth_<level>, or with level=None the one consistency.depth_key chooses (the finest present).
        A pixel counts where `valid` (optional bool image) is set and depth_gt is finite and inside d_range -- this build's
        default, unpinned -- so the 0 of a splatted image's holes never counts."""
        if not hasattr(output, "keys"):
            raise ValueError("Evaluator.evaluate_depth: output must be the dict Renderer.render_view returned")
        key = consistency.depth_key(output, None if level is None else "depth_%d" % int(level))
        pred = output[key]
        if not isinstance(pred, torch.Tensor) or not isinstance(depth_gt, torch.Tensor):
            raise ValueError("Evaluator.evaluate_depth: %s and depth_gt must be tensors" % key)
        if tuple(pred.shape) != tuple(depth_gt.shape):
            raise ValueError("Evaluator.evaluate_depth: %s is %s, depth_gt %s" % (key, tuple(pred.shape), tuple(depth_gt.shape)))
        if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != tuple(depth_gt.shape)):
            raise ValueError("Evaluator.evaluate_depth: valid must be a bool image of depth_gt's shape %s" % (tuple(depth_gt.shape),))
        mask = None if valid is None else (valid != 0).contiguous()
        self.depth_sums, self.depth_counts = ops.depth_metrics(pred.float().contiguous(), depth_gt.float().contiguous(), mask, d_range,
                                                               self.depth_sums, self.depth_counts)
        return key

    def evaluate_geometry(self, pred_points, gt_points, max_dist, thresholds=()):
        """Accumulate 3D reconstruction metrics of a predicted cloud (e.g. Mesh.sample of a fused mesh) against a ground-truth
        cloud (e.g. the accumulated scan), both (n, 3) float32 on the GPU: an index over each (pointcloud.NearestIndex), each
        queried with the other at radius max_dist, both directions accumulated on the device (ops.cloud_metrics; the rule is
        in include/pnr.h "nearest neighbours").  Distances are clamped at max_dist, the usual practice: a point with no
        neighbour within max_dist counts as max_dist.  Points with a non-finite coordinate are left out.  thresholds: at
        most 8 distances in (0, max_dist] for precision / recall / F-score.  A later call before summarize() must give the same
        max_dist and thresholds.  Returns the two query results {"pred_to_gt", "gt_to_pred"}."""
        from . import pointcloud
        what = "Evaluator.evaluate_geometry"
        n_p, n_g = ops.nn_cloud(what, "pred_points", pred_points), ops.nn_cloud(what, "gt_points", gt_points)
        d, _ = ops.nn_params(what, max_dist, max(n_p, n_g))
        taus = ops.cloud_thresholds(what, thresholds, d)
        if self.geom is not None and (self.geom["max_dist"] != d or self.geom["thresholds"] != taus):
            raise ValueError("%s: max_dist and thresholds (%r, %r) differ from those of an earlier call since the last summarize() "
                             "(%r, %r)" % (what, d, taus, self.geom["max_dist"], self.geom["thresholds"]))
        if not pred_points.is_cuda or not gt_points.is_cuda:
            raise RuntimeError("%s: the clouds must be on the GPU (the HIP path has no CPU fallback)" % what)
        if pred_points.device != gt_points.device:
            raise ValueError("%s: pred_points is on %s, gt_points on %s" % (what, pred_points.device, gt_points.device))
        res, terms = {}, []
        for name, q, ref in (("pred_to_gt", pred_points, gt_points), ("gt_to_pred", gt_points, pred_points)):
            res[name] = pointcloud.NearestIndex(ref, d).query(q)
            terms.append(ops.cloud_metrics(res[name]["index"], res[name]["dist2"], d, taus, query=q))
        # both directions are in hand before either is accumulated: a call that raises half way leaves the accumulators as they were
        if self.geom is None:
            self.geom = {"max_dist": d, "thresholds": taus, "sums": [s for s, _ in terms], "counts": [c for _, c in terms]}
        else:
            for k, (s, c) in enumerate(terms):
                self.geom["sums"][k] = self.geom["sums"][k] + s
                self.geom["counts"][k] = self.geom["counts"][k] + c
        return res

    def _accumulate_pq(self, pred_id, gt_id):
        """Per-frame PQ terms (Kirillov et al.): segments match when same class and IoU > 0.5 (then the match is unique).
        Panoptic ids: class*1000 + instance for things, class for stuff; < 0 = ignore.  Segment ids are re-mapped PER
        FRAME to 0..n-1 (torch.unique), so arbitrary instance indices (KITTI-360 ground truth uses large ones) can never
        alias into another class's slots.  The pixel-pair counting is pnr_confusion; the small (n_seg x n_seg) IoU /
        matching algebra below is host-side torch bookkeeping on the device (evaluation only, not on the render path)."""
        C = self.n_classes
        dev = pred_id.device

        def segments(ids):
            ok = ids >= 0
            uniq, inv = torch.unique(ids[ok], return_inverse=True)
            comp = torch.full_like(ids, -1)
            comp[ok] = inv.int()
            cls = torch.where(uniq >= 1000, uniq // 1000, uniq).long()
            # out-of-range classes go to a real OVERFLOW row (index C of a C + 1 row table, dropped before it is accumulated), so
            # they never count in a real class's terms; their number is kept on the device and summarize() reports it -- no host
            # round trip per frame
            bad = (cls >= C) | (cls < 0)
            self._bad_ids = bad.sum() if self._bad_ids is None else self._bad_ids + bad.sum()
            return comp.contiguous(), torch.where(bad, torch.full_like(cls, C), cls)

        seg_p, cls_p = segments(pred_id)
        seg_g, cls_g = segments(gt_id)
        n = max(int(cls_p.numel()), int(cls_g.numel()), 1)
        pair = ops.confusion(seg_p, seg_g, n).double()[: max(cls_g.numel(), 1), : max(cls_p.numel(), 1)]   # [gt seg, pred seg]
        if cls_g.numel() == 0 or cls_p.numel() == 0:
            pair = torch.zeros((cls_g.numel(), cls_p.numel()), device=dev, dtype=torch.float64)
        # pixels whose ground truth is ignored do not count against the prediction
        valid = (gt_id >= 0) & (seg_p >= 0)
        area_p = torch.bincount(seg_p[valid].long(), minlength=cls_p.numel()).double()
        area_g = pair.sum(1)
        union = area_g[:, None] + area_p[None, :] - pair
        iou = torch.where(union > 0, pair / union.clamp(min=1), torch.zeros_like(pair))
        match = (iou > 0.5) & (cls_g[:, None] == cls_p[None, :])
        tp_g, tp_p = match.any(1), match.any(0)
        terms = torch.zeros((C + 1, 4), device=dev, dtype=torch.float64)          # row C: the overflow row (dropped)
        terms[:, 0].index_add_(0, cls_g, (iou * match).sum(1))
        terms[:, 1].index_add_(0, cls_g, tp_g.double())
        terms[:, 2].index_add_(0, cls_p, ((area_p > 0) & ~tp_p).double())
        terms[:, 3].index_add_(0, cls_g, ((area_g > 0) & ~tp_g).double())
        terms = terms[:C]
        self.pq = terms if self.pq is None else self.pq + terms

    def summarize(self):
        """The metrics accumulated since the last call; the accumulators are reset in every case (also when it raises)."""
        try:
            return self._summarize()
        finally:
            self.mse, self.conf, self.pq, self._bad_ids, self.mc_agree, self.mc_stats = [], None, None, None, None, None
            self.depth_sums, self.depth_counts = None, None
            self.geom = None

    def _summarize(self):
        out = {}
        if self.mse:
            mse = torch.stack(self.mse).double().cpu()
            out["psnr"] = float((-10.0 * torch.log10(mse.clamp(min=1e-12))).mean())
            out["mse"] = float(mse.mean())
        if self.conf is not None:
            c = self.conf.double().cpu()
            tp = c.diag()
            union = c.sum(0) + c.sum(1) - tp
            seen = union > 0
            iou = torch.where(seen, tp / union.clamp(min=1), torch.full_like(tp, float("nan")))
            out["iou"] = iou.tolist()
            out["miou"] = float(iou[seen].mean()) if seen.any() else math.nan
            out["pixel_acc"] = float(tp.sum() / c.sum().clamp(min=1))
        if self.pq is not None:
            if self._bad_ids is not None and int(self._bad_ids) > 0:
                raise ValueError("Evaluator: %d segment id(s) carried a class index >= n_classes = %d" % (int(self._bad_ids), self.n_classes))
            t = self.pq.cpu()
            denom = t[:, 1] + 0.5 * t[:, 2] + 0.5 * t[:, 3]
            seen = denom > 0
            pq = torch.where(seen, t[:, 0] / denom.clamp(min=1e-12), torch.full_like(denom, float("nan")))
            out["pq_per_class"] = pq.tolist()
            out["pq"] = float(pq[seen].mean()) if seen.any() else math.nan
            out["sq"] = float((t[:, 0][seen] / t[:, 1][seen].clamp(min=1e-12))[t[:, 1][seen] > 0].mean()) if (t[:, 1] > 0).any() else math.nan
            out["rq"] = float((t[:, 1] / denom.clamp(min=1e-12))[seen].mean()) if seen.any() else math.nan
        if self.mc_agree is not None:
            c = self.mc_agree.double().cpu()
            rows = c.sum(1)
            out["mc"] = float(c.diag().sum() / c.sum()) if float(c.sum()) > 0 else math.nan
            out["mc_per_class"] = torch.where(rows > 0, c.diag() / rows.clamp(min=1), torch.full_like(rows, float("nan"))).tolist()
            out["mc_stats"] = [int(v) for v in self.mc_stats.cpu().tolist()]
        if self.depth_counts is not None:
            c, s = [int(v) for v in self.depth_counts.cpu().tolist()], self.depth_sums.cpu().tolist()
            n = c[0]
            mean = lambda v: v / n if n else math.nan
            out["depth_n"], out["depth_missing"] = n, c[4]
            out["depth_mae"], out["depth_rmse"] = mean(s[0]), math.sqrt(mean(s[1])) if n else math.nan
            out["depth_abs_rel"], out["depth_sq_rel"] = mean(s[2]), mean(s[3])
            out["depth_rmse_log"] = math.sqrt(mean(s[4])) if n else math.nan
            out["depth_d1"], out["depth_d2"], out["depth_d3"] = mean(c[1]), mean(c[2]), mean(c[3])
        if self.geom is not None:
            side = []
            for k in range(2):
                c, s = [int(v) for v in self.geom["counts"][k].cpu().tolist()], self.geom["sums"][k].cpu().tolist()
                n = c[0]
                side.append((n, c[1], s[0] / n if n else math.nan, math.sqrt(s[1] / n) if n else math.nan,
                             [c[2 + j] / n if n else math.nan for j in range(len(self.geom["thresholds"]))]))
            (n_p, miss_p, acc, acc_rms, prec), (n_g, miss_g, comp, comp_rms, rec) = side
            out["geom_accuracy"], out["geom_completeness"], out["geom_chamfer"] = acc, comp, 0.5 * (acc + comp)
            out["geom_accuracy_rms"], out["geom_completeness_rms"] = acc_rms, comp_rms
            out["geom_precision"], out["geom_recall"] = prec, rec
            out["geom_fscore"] = [2.0 * p * r / (p + r) if p + r > 0 else math.nan for p, r in zip(prec, rec)]
            out["geom_n_pred"], out["geom_n_gt"], out["geom_missing_pred"], out["geom_missing_gt"] = n_p, n_g, miss_p, miss_g
        return out
