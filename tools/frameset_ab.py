"""Graphed training step fed by a FrameSet (train.GraphedStep(frames=...): the batch is drawn inside the graph) against the
GraphedStep of another checkout fed a pre-built GPU batch (every call copies the batch into the static tensors, then replays) --
bench.py's training geometry (config 5: 8 x 256 NeRFs, 45 / 32 heads, bbox prior, 64 + 128 samples; 4096 rays, NetworkWrapper,
Adam(capturable, fused), cfg.rng = "device" with perturb = 1 and raw_noise_std = 1).  One arm per process, so that the `batch` arm
can import the package of ANOTHER tree (--root: e.g. `git archive <parent> | tar -x -C build/parent` with that commit's
libpnr.so beside it) and runs that commit's code, not this one's:

    python3 tools/frameset_ab.py --arm frames --save-batch build/ab_batch.pt          # this tree; writes one of its batches
    python3 tools/frameset_ab.py --arm batch --root build/parent --batch build/ab_batch.pt
    python3 tools/frameset_ab.py --arm batch --root build/parent --batch build/ab_batch.pt      # twice: the spread of the baseline

Each step is timed with hip events after a warm-up; the whole timed loop is also timed on the host clock around a synchronise
(host work per step shows there).  One JSON line per run.  The sampler kernel's own time: the `frames` arm under
`rocprofv3 --kernel-trace --stats` with a few steps (k_sample_batch in the kernel statistics), a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frame_set(dev, C, K, n_pinhole=8, n_fisheye=4):
    """KITTI-360-shaped posed frames with random images: 1408 x 376 pinhole frames along a path, 1400 x 1400 side-facing fisheyes"""
    import math
    import torch
    from panopticnerf_amd import FrameSet, Pinhole, synthetic
    g = torch.Generator().manual_seed(0)
    fs = FrameSet(dev, capacity=n_pinhole + n_fisheye, seed=1)

    def images(H, W):
        return (torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8), torch.rand(H, W, generator=g) * 20,
                torch.randint(-1, C, (H, W), generator=g), torch.randint(-1, K, (H, W), generator=g))

    pin = Pinhole(synthetic.KITTI_F, synthetic.KITTI_F, synthetic.KITTI_CX, synthetic.KITTI_CY, synthetic.KITTI_W, synthetic.KITTI_H)
    for i in range(n_pinhole):
        yaw = 0.05 * i
        c2w = [[math.cos(yaw), 0.0, math.sin(yaw), 0.3 * i], [0.0, 1.0, 0.0, 1.55], [-math.sin(yaw), 0.0, math.cos(yaw), 1.5 * i]]
        fs.add(pin, c2w, 0.5, 100.0, *images(pin.height, pin.width))
    for i in range(n_fisheye):
        cam, c2w = synthetic.fisheye_camera(yaw=(math.pi / 2) * (1 if i % 2 else -1), origin=(0.0, 1.55, 3.0 * i))
        fs.add(cam, c2w, 0.5, 100.0, *images(cam.height, cam.width))
    fs.set_boxes(*synthetic.random_boxes(64, C, K))
    return fs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("frames", "batch"), required=True)
    ap.add_argument("--root", default=HERE, help="the tree to import panopticnerf_amd from (the `batch` arm: another checkout)")
    ap.add_argument("--batch", default=None, help="`batch` arm: the batch to feed (written by --save-batch)")
    ap.add_argument("--save-batch", default=None, help="`frames` arm: write one sampled batch here")
    ap.add_argument("--mode", default="pooled")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from types import SimpleNamespace as NS
    import panopticnerf_amd
    from panopticnerf_amd import NetworkWrapper, make_network, synthetic, train as pnr_train
    assert os.path.abspath(os.path.dirname(os.path.dirname(panopticnerf_amd.__file__))) == os.path.abspath(args.root), panopticnerf_amd.__file__

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    C, K = 45, 32
    cfg = NS(**vars(synthetic.baseline_cfg(5, precision="bf16")))
    cfg.perturb, cfg.raw_noise_std, cfg.rng, cfg.rng_seed = 1.0, 1.0, "device", 1
    torch.manual_seed(0)
    net = make_network(cfg).to(dev).train()
    synthetic.trained_like_(net)
    wrap = NetworkWrapper(net, cfg)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4, capturable=True, fused=True)
    if args.arm == "frames":
        fs = frame_set(dev, C, K)
        if args.save_batch:
            keep = fs.rng_state.clone()
            torch.save({k: v.cpu() for k, v in fs.sample(args.rays, args.mode).items()}, args.save_batch)
            fs.rng_state.copy_(keep)
        step = pnr_train.GraphedStep(wrap, opt, frames=fs, n_rays=args.rays, mode=args.mode)
        run = step
    else:
        tb = {k: v.to(dev) for k, v in torch.load(args.batch).items()}
        assert tb["rays"].shape[1] == args.rays
        step = pnr_train.GraphedStep(wrap, opt, tb)
        run = lambda: step(tb)
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        run()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps * 1e3
    t = sorted(a.elapsed_time(b) for a, b in ev)
    loss = step.out[1].detach().item()
    print(json.dumps({"arm": args.arm, "label": args.label, "root": os.path.relpath(os.path.abspath(args.root), HERE), "mode": args.mode,
                      "rays": args.rays, "steps": len(t), "median_ms": round(statistics.median(t), 4), "p10_ms": round(t[len(t) // 10], 4),
                      "p90_ms": round(t[(9 * len(t)) // 10], 4), "min_ms": round(t[0], 4), "wall_ms_per_step": round(wall, 4),
                      "last_loss": loss}), flush=True)


if __name__ == "__main__":
    main()
