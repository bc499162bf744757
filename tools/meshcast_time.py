"""Mesh ray casting of a mesh.extract sphere (profiles/README.md "Mesh ray casting"): mesh.RayIndex's build and the cast launch
(k_mesh_cast) into a 1408 x 376 pinhole frame and a 2048 x 1024 panorama, from outside the sphere and from inside it -- hip events
(torch.cuda.Event) around a captured graph of REPS launches, in one process, the index and the outputs allocated once; the
build, which synchronises twice, by a host clock around a call that ends in a synchronise.  Every cast writes all seven outputs.
For scale, not as a pass mark: fusion.raycast's launch (k_tsdf_raycast) of a TSDF volume of the same sphere on the same
lattice into the same cameras, and the plain loop over all faces (an index of one cell) on a strip of the pinhole frame.
   python tools/meshcast_time.py [res] [rounds]                       (PNR_LIB_PATH selects an A/B build of the library)"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from panopticnerf_amd import Equirect, Pinhole, _lib, fusion, mesh, ops, synthetic as sy

res = int(sys.argv[1]) if len(sys.argv) > 1 else 256
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
REPS = 20
LO, HI, RADIUS = (-1.2, -1.2, -1.2), (1.2, 1.2, 1.2), 0.7
NEAR, FAR = 0.05, 100.0
dev = torch.device("cuda:0")
prop = torch.cuda.get_device_properties(0)
print("library:", os.path.relpath(_lib.LIB_PATH, ROOT))
print("device: %s, %d CUs, clock_rate %.0f MHz, memory_clock_rate %.0f MHz" % (prop.name, prop.multi_processor_count,
      getattr(prop, "clock_rate", 0) / 1e3, getattr(prop, "memory_clock_rate", 0) / 1e3))


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                       # replayed from a capture: the Python front end is not timed
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1) / reps)
    us.sort()
    return us[len(us) // 2], "median %9.1f us   min %9.1f   max %9.1f" % (us[len(us) // 2], us[0], us[-1])


def clocks_while(fn, reps=REPS, replays=6):
    """the box's clocks while `fn` runs: replays of a captured graph are queued, `rocm-smi --showclocks` (a read) is asked while
    they run, and its sclk / mclk / fclk lines come back"""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    for _ in range(replays):
        graph.replay()
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError) as e:
        out = "rocm-smi: %s" % e
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    return [l.strip() for l in out.splitlines() if any(k in l for k in ("sclk", "mclk", "fclk", "rocm-smi:"))], busy


field = sy.sdf_grid("sphere", LO, HI, res, radius=RADIUS, device=dev)
m = mesh.extract(field, LO, HI, 0.0)
V, F = m.vertices.shape[0], m.faces.shape[0]
walls = []
for _ in range(rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx = mesh.RayIndex(m)
    torch.cuda.synchronize()
    walls.append(1e3 * (time.perf_counter() - t0))
walls.sort()
n = idx.records.shape[0]
print("sphere of radius %.1f in a %d^3 lattice: %d vertices, %d faces; grid %d x %d x %d, %d entries (%.2f a face, %.2f a cell), records %.1f MB"
      % ((RADIUS, res, V, F) + idx.res + (n, n / max(F, 1), n / (idx.res[0] * idx.res[1] * idx.res[2]), 48e-6 * n)))
print("    %-46s median %9.2f ms   min %9.2f   max %9.2f   (host clock: five launch groups, two read-backs, the allocations)"
      % ("RayIndex build", walls[len(walls) // 2], walls[0], walls[-1]))
ws = ops.mesh_grid_workspace(idx.res, dev)
total, start = torch.empty(1, dtype=torch.int64, device=dev), torch.empty_like(idx.start)
records, bounds = torch.empty_like(idx.records), torch.empty(8, device=dev)


def build_launches():
    ops.mesh_grid_bounds(m.vertices, m.faces, bounds=bounds)
    ops.mesh_grid_count(m.vertices, m.faces, idx.res, idx.lo, idx.cell, start=start, total=total, workspace=ws)
    ops.mesh_grid_fill(m.vertices, m.faces, idx.res, idx.lo, idx.cell, start, records, ws)


_, line = timed(build_launches)
print("    %-46s %s" % ("its launches alone (bounds, count, scan, fill)", line))

# the same sphere as a TSDF volume on the same lattice: positive behind the surface, every point observed
vol = fusion.Volume(LO, HI, res, dev)
vol.tsdf.copy_((field / 0.1).clamp(-1.0, 1.0))
vol.weight.fill_(1.0)
dt = ops.raycast_default_dt(vol.step)
max_steps = ops.raycast_default_max_steps(vol.res, vol.step, dt)

outside = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, -2.0]])
inside = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, -0.2]])
views = (("pinhole 1408 x 376", Pinhole(552.554261, 552.554261, 682.049453, 238.769549, 1408, 376)), ("equirect 2048 x 1024", Equirect(2048, 1024)))
last = None
for vname, cam in views:
    h, w = cam.height, cam.width
    out = {k: torch.empty((h, w) + tail, dtype=dt_, device=dev) for k, dt_, tail in ops.MESHCAST_OUTPUTS}
    tout = {"depth": torch.empty((h, w), device=dev), "code": torch.empty((h, w), dtype=torch.uint8, device=dev),
            "normal": torch.empty((h, w, 3), device=dev), "src": torch.empty((h, w), dtype=torch.int32, device=dev)}
    for pname, c2w in (("from outside", outside), ("from inside", inside)):
        def cast(c2w=c2w, index=idx):
            ops.mesh_raycast(cam.model, cam.params, c2w, w, h, NEAR, FAR, m.vertices, m.faces, index.res, index.lo, index.cell, index.start,
                             index.records, out)

        def march(c2w=c2w):
            ops.tsdf_raycast(cam.model, cam.params, c2w, w, h, NEAR, FAR, vol.lo32, vol.step, vol.tsdf, vol.weight, tout["depth"], tout["code"],
                             normal=tout["normal"], src=tout["src"], dt=dt, max_steps=max_steps)

        us, line = timed(cast)
        codes = torch.bincount(out["code"].reshape(-1).long(), minlength=3).tolist()
        print("%s, %s: %d rays; HIT %d, NO_RAY %d, MISSED %d" % ((vname, pname, h * w) + tuple(codes[:3])))
        print("    %-46s %s   (%.1f M rays/s)" % ("mesh.raycast's launch", line, h * w / us))
        us_t, line = timed(march)
        tc = torch.bincount(tout["code"].reshape(-1).long(), minlength=4).tolist()
        print("    %-46s %s   (for scale; HIT %d, NO_SURFACE %d)" % ("fusion.raycast's launch, the same lattice", line, tc[0], tc[3]))
        last = cast
lines, busy = clocks_while(last)
print("    clocks read %s:" % ("while the casts ran" if busy else "AFTER the queued casts had finished"))
for l in lines:
    print("        " + l)

# for scale: the plain loop over all faces, through an index of one cell, on an 8-row strip of the pinhole frame
one = mesh.RayIndex(m, (1, 1, 1))
strip = Pinhole(552.554261, 552.554261, 682.049453, 3.5, 1408, 8)
sout = {k: torch.empty((8, 1408) + tail, dtype=dt_, device=dev) for k, dt_, tail in ops.MESHCAST_OUTPUTS}
gout = {k: torch.empty((8, 1408) + tail, dtype=dt_, device=dev) for k, dt_, tail in ops.MESHCAST_OUTPUTS}
us1, line = timed(lambda: ops.mesh_raycast(strip.model, strip.params, outside, 1408, 8, NEAR, FAR, m.vertices, m.faces, one.res, one.lo, one.cell,
                                           one.start, one.records, sout), reps=2)
usg, _ = timed(lambda: ops.mesh_raycast(strip.model, strip.params, outside, 1408, 8, NEAR, FAR, m.vertices, m.faces, idx.res, idx.lo, idx.cell,
                                        idx.start, idx.records, gout))
equal = all(torch.equal(sout[k].view(torch.uint8), gout[k].view(torch.uint8)) for k in sout)
print("a strip of 1408 x 8 pixels through one cell of all %d faces: %s   (the grid: %.1f us; outputs equal: %s)" % (F, line, usg, equal))
