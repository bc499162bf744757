"""One training step with perturb = 1 and raw_noise_std = 1 at the bench's training geometry (bench.py config 5: 8 x 256 NeRFs,
45 / 32 heads, bbox prior, 64 + 128 samples; 4096 rays, NetworkWrapper, Adam(capturable, fused)) -- cfg.rng = "torch" (torch.rand /
torch.randn chunk by chunk) against cfg.rng = "device" (the in-kernel Philox stream), eager and replayed through train.GraphedStep.
The arms are interleaved A/B in one process (one step of each in turn, same batch), each step timed with hip events (torch.cuda.Event)
after a warm-up.  Prints one JSON line per arm (median and spread of the step times, ms) and one summary line.

    python3 tools/rng_step_time.py [--steps 60] [--warmup 5] [--rays 4096] [--mode eager,graph] [--out file.json]

Under rocprofv3 --kernel-trace --stats (a run of its own) the launches that disappear in device mode and the per-kernel time of
the _rng instantiations are in the kernel statistics (one arm per run: --steps 10 --mode eager --rng torch, then --rng device)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(mode, rng, rays_n, dev):
    from types import SimpleNamespace as NS
    from panopticnerf_amd import NetworkWrapper, make_network, make_renderer, synthetic, train as pnr_train
    C, K = 45, 32
    cfg = NS(**vars(synthetic.baseline_cfg(5, precision="bf16")))
    cfg.perturb, cfg.raw_noise_std, cfg.rng, cfg.rng_seed = 1.0, 1.0, rng, 1
    torch.manual_seed(0)
    net = make_network(cfg).to(dev).train()
    synthetic.trained_like_(net)
    wrap = NetworkWrapper(net, cfg)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4, capturable=True, fused=True)
    rays = synthetic.camera_rays()[:: 1408 * 376 // rays_n][:rays_n].contiguous().to(dev)
    box, ids = (t.to(dev) for t in synthetic.random_boxes(64, C, K))
    g = torch.Generator().manual_seed(0)
    R = rays.shape[0]
    tb = {"rays": rays[None], "bbox": box, "bbox_ids": ids, "rgb": torch.rand(1, R, 3, generator=g).to(dev),
          "depth": (torch.rand(1, R, generator=g) * 20).to(dev), "pseudo_label": torch.randint(-1, C, (1, R), generator=g).int().to(dev),
          "instance_label": torch.randint(-1, K, (1, R), generator=g).int().to(dev)}
    assert make_renderer(cfg, net).N_importance == cfg.N_importance
    if mode == "graph":
        step = pnr_train.GraphedStep(wrap, opt, tb)
        return lambda: step(tb)

    def eager():
        opt.zero_grad(set_to_none=False)
        _, loss, _, _ = wrap(tb)
        loss.backward()
        opt.step()
    return eager


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--mode", default="eager,graph")
    ap.add_argument("--rng", default="torch,device", help="arms (one arm: for a kernel trace of that arm alone)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    results = []
    for mode in args.mode.split(","):
        arms = {rng: build(mode, rng, args.rays, dev) for rng in args.rng.split(",")}
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times = {rng: [] for rng in arms}
        for _ in range(args.steps):
            for rng, fn in arms.items():            # interleaved A/B
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[rng].append(a.elapsed_time(b))
        for rng, t in times.items():
            t = sorted(t)
            rec = {"mode": mode, "rng": rng, "rays": args.rays, "steps": len(t), "median_ms": round(statistics.median(t), 4),
                   "p10_ms": round(t[len(t) // 10], 4), "p90_ms": round(t[(9 * len(t)) // 10], 4), "min_ms": round(t[0], 4)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        if len(arms) == 2:
            md, mt = (next(r["median_ms"] for r in results if r["mode"] == mode and r["rng"] == x) for x in ("device", "torch"))
            summary = {"mode": mode, "device_minus_torch_ms": round(md - mt, 4), "device_over_torch": round(md / mt, 4)}
            results.append(summary)
            print(json.dumps(summary), flush=True)
        del arms
        torch.cuda.synchronize()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
