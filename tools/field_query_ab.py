"""Same-box A/B of the field query at the benched network (8 x 256, 45 + 32 heads, bf16, head_tap "trunk") on P points drawn
uniformly from [-50, 50]^3 (default 2^24: a 256^3 grid), in ONE process, the arms alternating round by round, device-event timing:

  A        the workaround a user had before Network.query: degenerate rays (o = point, d = (0, 0, 1), z = 0, one sample per ray),
           ops.mlp_forward on the classic plan-0 image, the two logit blocks transposed, ops.panoptic_labels;
  A_mlp    its ops.mlp_forward launch alone (rays, z and the raw image preallocated);
  B        ops.mlp_query(want = ("sigma", "labels")) into preallocated outputs -- k_mlp_pp_field on the plan-4 image;
  B_sigma  want = ("sigma",): the trunk and alpha_linear alone;
  B_logits want = ("sigma", "labels", "logits").

First the values: B_logits' sigma / logits / labels are compared with A's, bit for bit.  Then the rounds; per round every arm's time
and B / A_mlp.  Acceptance: B faster than A_mlp in EVERY round (B runs a strict subset of A's layers in the same kernel form and
writes 27 x fewer bytes).  TFLOP/s = 2 x MAC per point ("K3 field query": 668,800 full network, 566,656 trunk + sigma +
both heads, 491,264 trunk + sigma) x P over the median time, and its share of the 2.5 PFLOP/s dense bf16 peak.

usage: python tools/field_query_ab.py [--points 16777216] [--rounds 9] [--warmup 2] [--out FILE]
       (--rounds 1 --warmup 1 as the target of `rocprofv3 --kernel-trace --stats`)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from panopticnerf_amd import make_network, ops, synthetic  # noqa: E402

MAC = {"A": 668800, "A_mlp": 668800, "B": 566656, "B_sigma": 491264, "B_logits": 566656}
PEAK_TFLOPS = 2500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    cfg = synthetic.baseline_cfg(5, precision="bf16")
    net = make_network(cfg).eval()
    synthetic.trained_like_(net)
    net = net.to(dev)
    C, K, P = cfg.num_classes, cfg.num_instances, args.points
    d0, img0 = net.packed(1, dev)
    d4, img4 = net.packed(1, dev, fused="field")
    assert d0.plan == 0 and d4.plan == 4
    pts = (torch.rand(P, 3, device=dev) * 100 - 50).contiguous()
    say("workload: %d points in [-50, 50]^3, %d x %d network, %d + %d heads, bf16; device %s" % (
        P, cfg.D, cfg.W, C, K, torch.cuda.get_device_name(dev)))

    rays = torch.zeros(P, 8, device=dev)
    zeros = torch.zeros(P, 1, device=dev)
    raw = ops.alloc_raw(4 + C + K, P, dev)
    out_b = {"sigma": torch.empty(P, device=dev), "sem_label": torch.empty(P, device=dev, dtype=torch.int32),
             "inst_label": torch.empty(P, device=dev, dtype=torch.int32)}
    out_l = dict(out_b, sem_logits=ops.alloc_raw(C, P, dev), inst_logits=ops.alloc_raw(K, P, dev))

    def arm_A():
        r = torch.zeros(P, 8, device=dev)
        r[:, :3] = pts
        r[:, 5] = 1.0
        r[:, 7] = 1.0
        w = ops.mlp_forward(d0, img0, r, torch.zeros(P, 1, device=dev))
        sem, inst, _ = ops.panoptic_labels(w[4:4 + C].t().contiguous(), w[4 + C:].t().contiguous())
        return w, sem, inst

    arms = {
        "A": arm_A,
        "A_mlp": lambda: ops.mlp_forward(d0, img0, rays, zeros, out=raw),
        "B": lambda: ops.mlp_query(d4, img4, pts, ("sigma", "labels"), out=out_b),
        "B_sigma": lambda: ops.mlp_query(d4, img4, pts, ("sigma",), out=out_b),
        "B_logits": lambda: ops.mlp_query(d4, img4, pts, ("sigma", "labels", "logits"), out=out_l),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.no_grad():
        rays[:, :3] = pts
        rays[:, 5] = 1.0
        rays[:, 7] = 1.0
        w, sem, inst = arm_A()
        b = arms["B_logits"]()
        torch.cuda.synchronize()
        same = (torch.equal(b["sigma"], w[3]) and torch.equal(b["sem_logits"], w[4:4 + C]) and torch.equal(b["inst_logits"], w[4 + C:])
                and torch.equal(b["sem_label"], sem) and torch.equal(b["inst_label"], inst))
        say("B's sigma, logits and labels are A's, bit for bit: %s" % same)
        del w, sem, inst
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        order = list(arms)
        for i in range(args.rounds):
            for name in (order if i % 2 == 0 else order[::-1]):
                times[name].append(timed(arms[name]))
    say("")
    say("per round (ms; %d rounds, the arms alternating):" % args.rounds)
    say("  round " + " ".join("%9s" % k for k in arms) + "   B / A_mlp")
    for i in range(args.rounds):
        say("  %5d " % i + " ".join("%9.3f" % times[k][i] for k in arms) + "   %.4f" % (times["B"][i] / times["A_mlp"][i]))
    say("")
    for k in arms:
        t = statistics.median(times[k])
        tf = 2.0 * MAC[k] * P / (t * 1e-3) / 1e12
        say("  %-8s median %9.3f ms  min %9.3f  max %9.3f   %7.1f TFLOP/s algorithmic (%d MAC/point) = %.3f of %.0f" % (
            k, t, min(times[k]), max(times[k]), tf, MAC[k], tf / PEAK_TFLOPS, PEAK_TFLOPS))
    ratio = [b_ / a for b_, a in zip(times["B"], times["A_mlp"])]
    say("")
    say("B / A_mlp: median %.4f (MAC ratio 0.847); B faster than A's MLP launch alone in every round: %s" % (
        statistics.median(ratio), all(r < 1 for r in ratio)))
    say("B / A (the whole workaround): median %.4f;  B_sigma / A_mlp: median %.4f (MAC ratio 0.735);  B_logits / A_mlp: median %.4f" % (
        statistics.median(b_ / a for b_, a in zip(times["B"], times["A"])),
        statistics.median(b_ / a for b_, a in zip(times["B_sigma"], times["A_mlp"])),
        statistics.median(b_ / a for b_, a in zip(times["B_logits"], times["A_mlp"]))))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write(json.dumps({"points": P, "ms": times, "bit_identical": same}) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
