"""pnr_cc_label and pnr_cc_mesh on scene-sized inputs, hip events (torch.cuda.Event) around a captured graph of REPS launches, in
one process (profiles/README.md "Connected components"): an SGM d16 image of synthetic.stereo_pair in the values mode, a panoptic
image and a 256^3 lattice (sdf_grid spheres plus Bernoulli floaters) in the keys mode, and the mesh mesh.extract makes of that
lattice.  Reports per case the time per call (median, min, max of the rounds), elements per second, the bytes per second of the
compulsory traffic (the data read once, labels and size written once) and that rate as a share of the measured HBM copy rate
(6.29 TB/s, MI355X_MICROARCH: a description, not a pass mark), the device's clocks while it runs, and -- for scale only --
scipy.ndimage.label on the host for the same input.  The flat-versus-tiled A/B is two runs of this tool:
   tools/build_ab.sh cc_flat:"-DPNR_CC_FLAT"
   python tools/cc_time.py [res] [rounds];  PNR_LIB_PATH=build/ab/libpnr_cc_flat.so python tools/cc_time.py [res] [rounds]"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from panopticnerf_amd import _lib, mesh, ops, stereo, synthetic as sy

res = int(sys.argv[1]) if len(sys.argv) > 1 else 256
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W, H, REPS, HBM = 1408, 376, 10, 6.29e12
dev = torch.device("cuda:0")
prop = torch.cuda.get_device_properties(0)
print("library:", os.path.relpath(_lib.LIB_PATH, ROOT))
print("device: %s, %d CUs; tiles %s / %s" % (prop.name, prop.multi_processor_count, ops.CC_TILE_2D, ops.CC_TILE_3D))


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
    return graph, us[len(us) // 2], "median %9.1f us   min %9.1f   max %9.1f" % (us[len(us) // 2], us[0], us[-1])


def clocks_while(graph, replays=6):
    """the box's clocks while the captured calls run: `rocm-smi --showclocks` (a read) is asked while queued replays run"""
    for _ in range(replays):
        graph.replay()
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError) as e:
        out = "rocm-smi: %s" % e
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    return [l.strip() for l in out.splitlines() if any(k in l for k in ("sclk", "mclk", "fclk", "rocm-smi:"))], busy


def host_label(mask, full):
    import scipy.ndimage as ndi
    t0 = time.perf_counter()
    _, n = ndi.label(mask, ndi.generate_binary_structure(mask.ndim, mask.ndim if full else 1))
    return n, 1e3 * (time.perf_counter() - t0)


def lattice_case(name, data, full, tol=None, host_mask=None):
    n = data.numel()
    labels, size = torch.empty(data.shape, dtype=torch.int32, device=dev), torch.empty(data.shape, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(ops.cc_workspace_bytes(n) // 8, dtype=torch.int64, device=dev)
    run = lambda: ops.cc_label(data, full, tol, labels=labels, size=size, count=count, workspace=ws)
    graph, us, line = timed(run)
    nc, largest = int(count.item()), int(size.max())
    moved = 12.0 * n                                          # the data read once, labels and size written once
    print("%-44s %s" % (name, line))
    print("    %d elements, %d foreground, %d components (largest %d);  %.2f Gelements/s;  %.1f GB/s compulsory = %.1f %% of %.2f TB/s"
          % (n, int((labels >= 0).sum()), nc, largest, n / us / 1e3, moved / us / 1e3, 100.0 * moved / (us * 1e-6) / HBM, HBM / 1e12))
    if host_mask is not None:
        hn, ms = host_label(host_mask, full)
        print("    for scale: scipy.ndimage.label of the foreground mask on the host, %d components, %.1f ms" % (hn, ms))
    return graph


# ---- 1. an SGM d16 image in the values mode, as stereo.despeckle labels it
left, right, _, _ = sy.stereo_pair(H, W, seed=0, device=dev)
d16 = stereo.sgm(left, right, max_disp=64)["d16"]
values = (d16.to(torch.int32) + 1).to(torch.float32).contiguous()
g = lattice_case("cc_label, values, %d x %d SGM d16, 4-linked" % (W, H), values, False, 16.0, (d16 >= 0).cpu().numpy())
lines, busy = clocks_while(g)
print("    clocks read %s: %s" % ("while it ran" if busy else "AFTER the queued calls had finished", ";  ".join(lines)))

# ---- 2. a panoptic image in the keys mode: blocks of ids with holes and salt
gen = np.random.default_rng(0)
ys, xs = np.mgrid[0:H, 0:W]
ids = ((ys // 47) * 100 + xs // 64).astype(np.int32)
ids[gen.random((H, W)) < 0.02] = -1
salt = gen.random((H, W)) < 0.01
ids[salt] = gen.integers(0, 50, size=int(salt.sum()))
lattice_case("cc_label, keys, %d x %d panoptic, 4-linked" % (W, H), torch.from_numpy(ids).to(dev), False)
lattice_case("cc_label, keys, %d x %d panoptic, 8-linked" % (W, H), torch.from_numpy(ids).to(dev), True)

# ---- 3. a lattice in the keys mode: spheres plus Bernoulli floaters
lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
field = torch.maximum(sy.sdf_grid("sphere", lo, hi, res, center=(-0.4, 0.0, 0.0), radius=0.45),
                      sy.sdf_grid("sphere", lo, hi, res, center=(0.55, 0.2, 0.1), radius=0.3))
inside = (field > 0) | (torch.from_numpy(np.random.default_rng(1).random((res,) * 3)) < 0.01)
keys = torch.where(inside, 0, -1).to(torch.int32).to(dev)
g = lattice_case("cc_label, keys, %d^3 spheres + floaters, 6-linked" % res, keys, False, host_mask=inside.numpy())
lines, busy = clocks_while(g, replays=3)
print("    clocks read %s: %s" % ("while it ran" if busy else "AFTER the queued calls had finished", ";  ".join(lines)))
lattice_case("cc_label, keys, %d^3 spheres + floaters, 26-linked" % res, keys, True)

# ---- 4. the mesh of that lattice
m = mesh.extract(inside.to(torch.float32).to(dev), lo, hi, 0.5)
V, F = m.vertices.shape[0], m.faces.shape[0]
vl, fl, fs = (torch.empty(k, dtype=torch.int32, device=dev) for k in (V, F, F))
count = torch.empty(1, dtype=torch.int64, device=dev)
ws = torch.empty(ops.cc_workspace_bytes(V) // 8, dtype=torch.int64, device=dev)
_, us, line = timed(lambda: ops.cc_mesh(m.faces, V, vl, fl, fs, count, ws))
moved = 12.0 * F + 4.0 * V + 8.0 * F
print("%-44s %s" % ("cc_mesh, the mesh of that lattice", line))
print("    %d vertices, %d faces, %d components (largest %d faces);  %.2f Gfaces/s;  %.1f GB/s compulsory = %.1f %% of %.2f TB/s"
      % (V, F, int(count.item()), int(fs.max()), F / us / 1e3, moved / us / 1e3, 100.0 * moved / (us * 1e-6) / HBM, HBM / 1e12))
