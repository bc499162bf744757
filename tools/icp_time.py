"""Pose tracking against a ray-cast of a 256^3 volume (profiles/README.md "Fusion"): one point-to-plane iteration
(k_icp_accumulate + k_icp_solve), its two launches on their own, and a whole fusion.track of 10 iterations, for a 1408 x 376
pinhole frame against a 1408 x 376 ray-cast -- hip events (torch.cuda.Event) around a captured graph of REPS runs, in one
process, everything allocated once.  The volume is what fusion.integrate makes of pinhole frames of synthetic.room_depth (a
room of 11 x 4.4 x 10.1 units seen from inside, in a volume box of 12 x 5 x 11); the model view is fusion.raycast's own output, and that launch is timed in the same
run, so the two can be placed beside each other.
   python tools/icp_time.py [res] [frames] [rounds] [name=path ...]
name=path: further builds of the library (A/B), loaded into the SAME process and timed in turn with the package's own, round by
round; the difference of their final pose from the package's is printed (a build with another grid adds in another order).
This is the A/B hook of tools/raycast_time.py: a kernel choice is measured by building the other form beside the package's
library and timing both here; the builds are swapped through _lib._lib, which ops reads at every launch."""
import ctypes, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import FrameSet, Pinhole, _lib, fusion, ops, synthetic

nums = [a for a in sys.argv[1:] if "=" not in a]
res = int(nums[0]) if len(nums) > 0 else 256
F = int(nums[1]) if len(nums) > 1 else 8
rounds = int(nums[2]) if len(nums) > 2 else 7
REPS, ITERS = 20, 10
W, H = 1408, 376
LO, HI = (-6.0, -2.5, 0.0), (6.0, 2.5, 11.0)
ROOM = ((-5.5, -2.2, 0.4), (5.5, 2.2, 10.5))
TRUNC, NEAR, FAR, DIST_MAX = 0.25, 0.1, 100.0, 0.25
dev = torch.device("cuda:0")


def library(path):
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


builds = [("package", _lib.load())] + [(a.split("=", 1)[0], library(a.split("=", 1)[1])) for a in sys.argv[1:] if "=" in a]
print("library:", os.path.basename(_lib.LIB_PATH), "".join("\n   + %s=%s" % (a.split("=", 1)[0], os.path.basename(a)) for a in sys.argv[1:] if "=" in a))


def captured(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                       # `reps` runs replayed from a capture: the Python front end is not timed
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def one_round(graph, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def line(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], "median %8.4f ms   min %8.4f   max %8.4f" % (ms[len(ms) // 2], ms[0], ms[-1])


def pose(f, n):
    a = f / max(n - 1, 1) - 0.5
    yaw = 0.4 * a
    return torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw), 3.0 * a], [0.0, 1.0, 0.0, 0.2], [-math.sin(yaw), 0.0, math.cos(yaw), 2.0 + 0.5 * a]], dtype=torch.float32)


cam = Pinhole(552.554261, 552.554261, 682.049453, 238.769549, W, H)
frames = FrameSet(dev, capacity=F)
for f in range(F):
    frames.add(cam, pose(f, F), NEAR, FAR, torch.zeros((H, W, 3), dtype=torch.uint8), depth=synthetic.room_depth(cam, pose(f, F), *ROOM))
vol = fusion.Volume(LO, HI, res, dev)
fusion.integrate(vol, frames, TRUNC)
torch.cuda.synchronize()
print("%d^3 = %d points, box %s .. %s, trunc %.2f, %d frames of %d x %d; %.1f %% of the points observed"
      % (res, res ** 3, LO, HI, TRUNC, F, W, H, 100.0 * float((vol.weight >= 1).float().mean())))

# the model view: the ray-cast from the middle pose; the live frame: the true depth of a pose 3 cm and 1.2 degrees away, tracked from the model's pose
c2w_m = pose(F // 2, F)
maps = {"depth": torch.empty((H, W), device=dev), "code": torch.empty((H, W), dtype=torch.uint8, device=dev),
        "normal": torch.empty((H, W, 3), device=dev), "src": torch.empty((H, W), dtype=torch.int32, device=dev)}


def raycast():
    ops.tsdf_raycast("pinhole", cam.params, c2w_m, W, H, NEAR, FAR, vol.lo32, vol.step, vol.tsdf, vol.weight, maps["depth"], maps["code"],
                     normal=maps["normal"], src=maps["src"])


g_ray = captured(raycast)
t_ray, l_ray = line([one_round(g_ray) for _ in range(rounds)])
print("    %-52s %s" % ("fusion.raycast, pinhole %d x %d" % (W, H), l_ray))
yaw = 0.02
truth = c2w_m.clone()
truth[:, :3] = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]]) @ c2w_m[:, :3]
truth[:, 3] += torch.tensor([0.02, -0.01, 0.02])
depth = synthetic.room_depth(cam, truth, *ROOM).to(dev)
view = (cam, c2w_m, maps)
guess = c2w_m.to(dev)

runs = []
for label, lib in builds:
    _lib._lib = lib                                       # ops asks _lib.load() for the library at launch (= capture) time
    ws = ops.icp_workspace(W * H, dev)
    p12 = guess.reshape(12).clone()
    hist = torch.zeros((1, 5), dtype=torch.float64, device=dev)
    acc = lambda ws=ws, p12=p12: ops.icp_accumulate("pinhole", cam.params, W, H, depth, p12, "pinhole", cam.params, c2w_m, W, H, maps["depth"], maps["normal"], DIST_MAX, ws)
    sol = lambda ws=ws, p12=p12, hist=hist: ops.icp_solve(ws, W * H, p12, hist[0], min_matches=64, max_rot=0.25, max_trans=0.5, update=False)
    out = {}

    def whole(out=out):
        out["c2w"], out["info"] = fusion.track(view, cam, depth, guess, iters=ITERS, dist_max=DIST_MAX, maps=False)

    runs.append((label, {"accumulate": (captured(acc), REPS), "solve": (captured(sol), REPS),
                         "iteration": (captured(lambda acc=acc, sol=sol: (acc(), sol())), REPS), "track": (captured(whole, 5), 5)}, out,
                 {k: [] for k in ("accumulate", "solve", "iteration", "track")}))
_lib._lib = builds[0][1]
for _ in range(rounds):                                   # the builds in turn, round by round
    for label, graphs, out, ms in runs:
        for k, (g, reps) in graphs.items():
            ms[k].append(one_round(g, reps))
h = runs[0][2]["info"]["history"].cpu()
err = lambda c2w: (float(torch.linalg.norm(c2w.cpu()[:, 3] - truth[:, 3])), float(torch.acos((((c2w.cpu()[:, :3] @ truth[:, :3].T).trace() - 1) / 2).clamp(-1, 1))))
print("live frame %d x %d: %d matches of %d pixels at the guess, %d at the end; pose error (units, radians) %s -> %s; statuses %s"
      % (W, H, h[0, 0], W * H, h[-1, 0], "(%.4f, %.4f)" % err(guess), "(%.5f, %.5f)" % err(runs[0][2]["c2w"]), h[:, 4].int().tolist()))
for label, graphs, out, ms in runs:
    note = "" if label == "package" else "   max |pose - the package's| = %.3g" % float((out["c2w"] - runs[0][2]["c2w"]).abs().max())
    for k, what in (("accumulate", "k_icp_accumulate"), ("solve", "k_icp_solve"), ("iteration", "one iteration (accumulate + solve)"),
                    ("track", "fusion.track, %d iterations (%d launches of its own)" % (ITERS, 2 * ITERS + 2))):
        t, text = line(ms[k])
        print("    %-52s %s   (%.2f x the ray-cast)%s" % (what + ", " + label, text, t / t_ray, note if k == "track" else ""))
