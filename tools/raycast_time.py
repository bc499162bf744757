"""Volume ray casting of a 256^3 volume (profiles/README.md "Fusion"): fusion.raycast's launch (k_tsdf_raycast) into a 1408 x 376
pinhole and a 1400 x 1400 fisheye -- hip events (torch.cuda.Event) around a captured graph of REPS launches, in one process,
the volume and the outputs allocated once.  The volume is what fusion.integrate makes of 32 pinhole frames inside a sphere of
radius 10 (tools/fusion_time.py's scene), and that call is timed in the same run, so the two can be placed beside each other.
Every launch writes depth, normal, src and code; the default march step (half the smallest lattice step) and max_steps.
   python tools/raycast_time.py [res] [frames] [rounds] [name=path ...]
name=path: further builds of the library (A/B), loaded into the SAME process and timed in turn with the package's own, round by
round; their outputs must equal the package's bit for bit."""
import ctypes, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import Fisheye, FrameSet, Pinhole, _lib, fusion, ops

nums = [a for a in sys.argv[1:] if "=" not in a]
res = int(nums[0]) if len(nums) > 0 else 256
F = int(nums[1]) if len(nums) > 1 else 32
rounds = int(nums[2]) if len(nums) > 2 else 7
REPS = 20
W, H = 1408, 376
RADIUS, TRUNC = 10.0, 0.25
LO, HI = (-6.0, -2.5, 6.0), (6.0, 2.5, 11.0)
NEAR, FAR = 0.1, 100.0
dev = torch.device("cuda:0")


def library(path):
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


builds = [("package", _lib.load())] + [(a.split("=", 1)[0], library(a.split("=", 1)[1])) for a in sys.argv[1:] if "=" in a]
print("library:", os.path.basename(_lib.LIB_PATH), "".join("\n   + %s=%s" % (a.split("=", 1)[0], os.path.basename(a)) for a in sys.argv[1:] if "=" in a))


def captured(fn):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                       # REPS runs replayed from a capture: the Python front end is not timed
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def one_round(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def line(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], "median %8.3f ms   min %8.3f   max %8.3f" % (ms[len(ms) // 2], ms[0], ms[-1])


# the scene of tools/fusion_time.py: pinhole cameras on a short trajectory inside a sphere, analytic z-depth
cam = Pinhole(552.554261, 552.554261, 682.049453, 238.769549, W, H)
frames = FrameSet(dev, capacity=F)
jj, ii = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
poses = []
for f in range(F):
    yaw = 0.5 * (f / max(F - 1, 1) - 0.5)
    o = torch.tensor([3.0 * (f / max(F - 1, 1) - 0.5), 0.2, 0.5 * f / max(F - 1, 1)], dtype=torch.float64)
    R = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]], dtype=torch.float64)
    c2w = torch.cat([R, o[:, None]], 1)
    poses.append(c2w.float())
    d = torch.stack([(ii - cam.intr[2]) / cam.intr[0], (jj - cam.intr[3]) / cam.intr[1], torch.ones_like(ii)], -1) @ R.T.to(dev)
    oc = o.to(dev)
    qa, qb, qc = (d * d).sum(-1), d @ oc, float(oc @ oc) - RADIUS * RADIUS
    depth = ((-qb + torch.sqrt(qb * qb - qa * qc)) / qa).to(torch.float32)
    frames.add(cam, c2w, 0.1, 100.0, torch.zeros((H, W, 3), dtype=torch.uint8, device=dev), depth=depth)
frames.w2c_table()
vol = fusion.Volume(LO, HI, res, dev)
g_int = captured(lambda: fusion.integrate(vol, frames, TRUNC))
t_int, l_int = line([one_round(g_int) for _ in range(rounds)])
vol.reset()
fusion.integrate(vol, frames, TRUNC)                      # the volume the rays see: every frame once
torch.cuda.synchronize()
print("%d^3 = %d points, box %s .. %s, trunc %.2f; %.1f %% of the points observed" % (res, res ** 3, LO, HI, TRUNC, 100.0 * float((vol.weight >= 1).float().mean())))
print("    %-44s %s" % ("fusion.integrate, %d frames of %d x %d" % (F, W, H), l_int))

fish = Fisheye(2.2134, 0.016798, 1.6548, 1336.3, 1335.8, 716.94, 705.76, 1400, 1400)
dt = ops.raycast_default_dt(vol.step)
max_steps = ops.raycast_default_max_steps(vol.res, vol.step, dt)
print("march step %.5f (half the smallest lattice step), max_steps %d" % (dt, max_steps))
for name, camera, model, c2w in (("pinhole %d x %d" % (W, H), cam, "pinhole", poses[F // 2]), ("fisheye 1400 x 1400", fish, "fisheye", poses[F // 2])):
    h, w = camera.height, camera.width
    runs = []
    for label, lib in builds:
        out = {"depth": torch.empty((h, w), device=dev), "code": torch.empty((h, w), dtype=torch.uint8, device=dev),
               "normal": torch.empty((h, w, 3), device=dev), "src": torch.empty((h, w), dtype=torch.int32, device=dev)}

        def launch(out=out):
            ops.tsdf_raycast(model, camera.params, c2w, w, h, NEAR, FAR, vol.lo32, vol.step, vol.tsdf, vol.weight, out["depth"], out["code"],
                             normal=out["normal"], src=out["src"], dt=dt, max_steps=max_steps)

        _lib._lib = lib                                  # ops asks _lib.load() for the library at launch (= capture) time
        runs.append((label, captured(launch), out, []))
    _lib._lib = builds[0][1]
    for _ in range(rounds):                               # the builds in turn, round by round
        for label, graph, out, ms in runs:
            ms.append(one_round(graph))
    codes = torch.bincount(runs[0][2]["code"].reshape(-1).long(), minlength=4).tolist()
    print("%s: %d rays; HIT %d, NO_RAY %d, MISSED %d, NO_SURFACE %d" % ((name, h * w) + tuple(codes)))
    for label, graph, out, ms in runs:
        t, text = line(ms)
        equal = all(torch.equal(out[k].view(torch.uint8), runs[0][2][k].view(torch.uint8)) for k in out)
        print("    %-44s %s   (%.1f M rays/s; %.2f x the %d-frame integrate)%s"
              % ("raycast, " + label, text, 1e-3 * h * w / t, t / t_int, F, "" if label == "package" else "   outputs equal the package's: %s" % equal))
