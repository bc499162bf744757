"""Same-box A/B of cfg.coarse_outputs: "all" (every coarse map; the default) against "weights" (the coarse level evaluated by the
sigma-only kernel k_mlp_pp_sigma on the plan-3 image, rgb_0 / semantic_0 / instance_0 not produced), in ONE process, frames of the
two arms interleaved.  Workload: bench.py's headline frame (BASELINE config 5: the full 1408 x 376 frame, 64 + 128 samples, 45 + 32
heads, 64 boxes, logits compositing, chunk 65,536, fine weights not kept).  "all" overlaps its levels where the box allows
(cfg.overlap_levels, the default); "weights" frames run serially; the serial "all" frame is timed too, to separate the two effects.
Then the coarse MLP launch alone on the first chunk of the frame: the plan-2 full launch (k_mlp_tt, what "all" runs) against the plan-3
one (benchlib.time_mlp_forward_tiles: hipEvents, mean over `iters` launches, shader MHz of the last one).

usage: python tools/coarse_outputs_ab.py [--frames 7] [--warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from panopticnerf_amd import benchlib, make_network, make_renderer, ops, synthetic  # noqa: E402
from panopticnerf_amd.renderer import chunk_plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=5, help="rounds of the coarse-launch comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    arms = {}
    base = dict(precision="bf16", chunk_size=65536, keep_weights=False, semantic_activation="none")
    torch.manual_seed(0)
    cfg = synthetic.baseline_cfg(5, **base)
    net = make_network(cfg).eval()
    synthetic.trained_like_(net)
    net = net.to(dev)
    box, ids = (t.to(dev) for t in synthetic.random_boxes(64, cfg.num_classes, max(cfg.num_instances, 1)))
    rays = synthetic.camera_rays().to(dev)
    batch = {"rays": rays.reshape(synthetic.KITTI_H, synthetic.KITTI_W, 8), "bbox": box, "bbox_ids": ids}
    arms["all"] = make_renderer(synthetic.baseline_cfg(5, coarse_outputs="all", **base), net)
    arms["weights"] = make_renderer(synthetic.baseline_cfg(5, coarse_outputs="weights", **base), net)
    arms["all_serial"] = make_renderer(synthetic.baseline_cfg(5, coarse_outputs="all", overlap_levels=False, **base), net)
    say("workload: %d rays (%d x %d), %d + %d samples, %d + %d heads, 64 boxes, logits, chunk %d (%d chunks); device %s" % (
        rays.shape[0], synthetic.KITTI_W, synthetic.KITTI_H, cfg.N_samples, cfg.N_importance, cfg.num_classes, cfg.num_instances,
        base["chunk_size"], len(chunk_plan(rays.shape[0], base["chunk_size"])), torch.cuda.get_device_name(dev)))

    def frame(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = arms[name].render(batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        for _ in range(args.warmup):
            for name in arms:
                frame(name)
        # the values: "weights" returns the bits of "all" for every key it has
        _, oa = frame("all")
        _, ow = frame("weights")
        same = set(ow) == set(oa) - {"rgb_0", "semantic_0", "instance_0"} and all(torch.equal(ow[k], oa[k]) for k in ow)
        say("weights keys = all keys - {rgb_0, semantic_0, instance_0}, every one bit-identical: %s" % same)
        del oa, ow
        times = {name: [] for name in arms}
        order = list(arms)
        for i in range(args.frames):
            for name in (order if i % 2 == 0 else order[::-1]):       # interleaved, the order alternating per round
                times[name].append(frame(name)[0])
    say("")
    say("frames (ms; %d per arm, interleaved):" % args.frames)
    for name in arms:
        t = times[name]
        say("  %-11s median %.2f  min %.2f  max %.2f   [%s]" % (name, statistics.median(t), min(t), max(t), " ".join("%.2f" % v for v in t)))
    ratio = [w / a for w, a in zip(times["weights"], times["all"])]
    faster = all(w < a for w, a in zip(times["weights"], times["all"]))
    say("  weights / all per round: %s   (median %.4f = %+.2f %%); weights faster in every round: %s" % (
        " ".join("%.4f" % r for r in ratio), statistics.median(ratio), 100 * (statistics.median(ratio) - 1), faster))
    rs = [w / a for w, a in zip(times["weights"], times["all_serial"])]
    say("  weights / all_serial per round: median %.4f (%+.2f %%): the coarse launch alone, without the overlap" % (
        statistics.median(rs), 100 * (statistics.median(rs) - 1)))

    # the coarse MLP launch alone, first chunk of the frame
    s, e = chunk_plan(rays.shape[0], base["chunk_size"])[0]
    rc = rays[s:e].contiguous()
    z = ops.stratified(rc, cfg.N_samples)
    full = net.packed(0, dev, fused=True)
    sigma = net.packed(0, dev, fused="sigma")
    lt = {"full": [], "sigma": []}
    for i in range(args.launches):
        for name, (d, img) in (("full", full), ("sigma", sigma)) if i % 2 == 0 else (("sigma", sigma), ("full", full)):
            lt[name].append(benchlib.time_mlp_forward_tiles(d, img, rc, z, iters=10))
    say("")
    say("coarse MLP launch alone (%d rays x %d samples, pnr_mlp_forward_tiles, mean of 10 launches per round, %d rounds):" % (
        rc.shape[0], cfg.N_samples, args.launches))
    for name, plan in (("full", full[0].plan), ("sigma", 3)):
        ms = [v[0] for v in lt[name]]
        say("  %-5s (plan %d) median %.3f ms  [%s]  MHz %s" % (name, plan, statistics.median(ms), " ".join("%.3f" % v for v in ms),
                                                             " ".join("%.0f" % v[1] for v in lt[name])))
    lr = statistics.median(v[0] for v in lt["sigma"]) / statistics.median(v[0] for v in lt["full"])
    say("  sigma / full: %.3f" % lr)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write(json.dumps({"frames_ms": times, "coarse_launch_ms": {k: [v[0] for v in lt[k]] for k in lt},
                                "coarse_launch_mhz": {k: [v[1] for v in lt[k]] for k in lt}}) + "\n")


if __name__ == "__main__":
    main()
