"""Depth fusion at 256^3 x 32 frames of 1408 x 376 (profiles/README.md "Fusion"): fusion.integrate (k_tsdf_integrate) with and
without the colour and label arrays -- hip events (torch.cuda.Event) around a captured graph of REPS runs, in one process, the
volume and the frames allocated once.  Beside each time two references, measured in the same process:
  * the byte floor: every volume array read once and written once (8 bytes a float or int, 2 + 4 (colour) + 2 (labels) of them a
    point), at the rate of a device-to-device copy_ of 512 MiB;
  * the same 32 frames as 32 single-frame calls, which read and write the volume 32 times.
The scene: pinhole cameras on a short trajectory inside a sphere of radius 10, analytic z-depth, random colour and labels; the box
holds the part of the sphere's surface the cameras look at.  The volume accumulates over the runs (the weights grow; the work per
point and frame does not depend on the values).
   python tools/fusion_time.py [res] [frames] [rounds]     (PNR_LIB_PATH selects an A/B build of the library)"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import FrameSet, Pinhole, _lib, fusion

res = int(sys.argv[1]) if len(sys.argv) > 1 else 256
F = int(sys.argv[2]) if len(sys.argv) > 2 else 32
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
REPS = 20
W, H = 1408, 376
RADIUS, TRUNC = 10.0, 0.25
LO, HI = (-6.0, -2.5, 6.0), (6.0, 2.5, 11.0)
dev = torch.device("cuda:0")
print("library:", _lib.LIB_PATH)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                       # REPS runs replayed from a capture: the Python front end is not timed
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    ms.sort()
    return ms[len(ms) // 2], "median %8.3f ms   min %8.3f   max %8.3f" % (ms[len(ms) // 2], ms[0], ms[-1])


a = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
b = torch.empty_like(a)
t_copy, line = timed(lambda: b.copy_(a))
copy_bw = 2 * a.numel() / (t_copy * 1e-3)                 # bytes read + bytes written per second
print("    %-40s %s   (%.2f TB/s read + written)" % ("copy_ of 512 MiB", line, copy_bw / 1e12))
del a, b

cam = Pinhole(552.554261, 552.554261, 682.049453, 238.769549, W, H)
frames = FrameSet(dev, capacity=F)
g = torch.Generator(device=dev).manual_seed(0)
jj, ii = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
for f in range(F):
    yaw = 0.5 * (f / max(F - 1, 1) - 0.5)
    o = torch.tensor([3.0 * (f / max(F - 1, 1) - 0.5), 0.2, 0.5 * f / max(F - 1, 1)], dtype=torch.float64)
    R = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]], dtype=torch.float64)
    c2w = torch.cat([R, o[:, None]], 1)
    d = torch.stack([(ii - cam.intr[2]) / cam.intr[0], (jj - cam.intr[3]) / cam.intr[1], torch.ones_like(ii)], -1) @ R.T.to(dev)
    oc = o.to(dev)
    qa, qb, qc = (d * d).sum(-1), d @ oc, float(oc @ oc) - RADIUS * RADIUS
    depth = ((-qb + torch.sqrt(qb * qb - qa * qc)) / qa).to(torch.float32)      # z-depth: the parameter of the z_cam = 1 ray
    rgb = torch.randint(0, 256, (H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    sem = torch.randint(-1, 20, (H, W), device=dev, dtype=torch.int16, generator=g)
    inst = torch.randint(-1, 500, (H, W), device=dev, dtype=torch.int16, generator=g)
    frames.add(cam, c2w, 0.1, 100.0, rgb, depth=depth, pseudo_label=sem, instance_label=inst)
frames.w2c_table()
N = res ** 3
print("%d^3 = %d points, %d frames of %d x %d, trunc %.2f, box %s .. %s" % (res, N, F, W, H, TRUNC, LO, HI))

for color, labels in ((False, False), (True, False), (False, True), (True, True)):
    vol = fusion.Volume(LO, HI, res, dev, color=color, labels=labels)
    name = "tsdf" + (" + colour" if color else "") + (" + labels" if labels else "")
    t_one, l_one = timed(lambda: fusion.integrate(vol, frames, TRUNC))
    if not color and not labels:
        fused = int((vol.weight > 0).sum())
        band = int(((vol.weight > 0) & (vol.tsdf.abs() < 1)).sum())
        print("    (after the first runs: %.1f %% of the points fused, %.1f %% inside the band)" % (100.0 * fused / N, 100.0 * band / N))

    def each():
        for f in range(F):
            fusion.integrate(vol, frames, TRUNC, first=f, last=f + 1)

    t_each, l_each = timed(each)
    floor_bytes = 8 * N * (2 + (4 if color else 0) + (2 if labels else 0))
    floor_ms = floor_bytes / copy_bw * 1e3
    print("%s" % name)
    print("    %-40s %s   (%.2f us a frame; byte floor %.2f GB = %.3f ms at the copy rate, %.1f %% of the time)"
          % ("one call, %d frames" % F, l_one, 1e3 * t_one / F, floor_bytes / 1e9, floor_ms, 100.0 * floor_ms / t_one))
    print("    %-40s %s   (%.2f x the one call; its floor is %d x as large: %.3f ms)"
          % ("%d single-frame calls" % F, l_each, t_each / t_one, F, F * floor_ms))
    del vol
