"""Mesh extraction at 256^3 (profiles/README.md "Mesh"): ops.mesh_count (k_mesh_classify, k_mesh_scan_sums, k_mesh_scan_add) and
ops.mesh_emit (k_mesh_emit) on a sphere and on Gaussian noise -- hip events (torch.cuda.Event) around a captured graph of REPS
runs, in one process, buffers allocated once.  Beside each time: V and T, the bytes the form must move -- 4N of field read,
the workspace written and read once each, 12V + 12T + 8V written -- and what share of the copy bandwidth that is, the copy
being measured here, in the same process, on a buffer of the same order of size (a device-to-device copy_ of 512 MiB).
   python tools/mesh_time.py [res] [rounds]                (PNR_LIB_PATH selects an A/B build of the library)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import _lib, mesh, ops, synthetic as sy

res = int(sys.argv[1]) if len(sys.argv) > 1 else 256
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
REPS = 10
dev = torch.device("cuda:0")
print("library:", _lib.LIB_PATH)
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                       # REPS runs replayed from a capture: the Python front end is not timed
    with torch.cuda.graph(graph):
        for _ in range(REPS):
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
        us.append(1000.0 * e0.elapsed_time(e1) / REPS)
    us.sort()
    return us[len(us) // 2], "median %8.1f us   min %8.1f   max %8.1f" % (us[len(us) // 2], us[0], us[-1])


a = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
b = torch.empty_like(a)
t_copy, line = timed(lambda: b.copy_(a))
copy_bw = 2 * a.numel() / (t_copy * 1e-6)                 # bytes read + bytes written per second
print("    %-34s %s   (%.2f TB/s read + written)" % ("copy_ of 512 MiB", line, copy_bw / 1e12))
del a, b

N = res ** 3
lo32, step = mesh.lattice(LO, HI, (res,) * 3)
ws_bytes = ops.mesh_workspace_bytes(res, res, res)
fields = {"sphere r = 0.7": sy.sdf_grid("sphere", LO, HI, res, radius=0.7, device=dev),
          "Gaussian noise": torch.randn((res, res, res), device=dev, generator=torch.Generator(device=dev).manual_seed(0))}
for name, field in fields.items():
    totals, ws = ops.mesh_count(field, 0.0)
    V, T = totals.tolist()
    vertices = torch.empty((V, 3), device=dev)
    faces = torch.empty((T, 3), device=dev, dtype=torch.int32)
    src = torch.empty((V,), device=dev, dtype=torch.int64)
    print("%s, %d^3 = %d points: V = %d, T = %d; workspace %.1f MB, outputs %.1f MB" % (name, res, N, V, T, ws_bytes / 1e6, (20 * V + 12 * T) / 1e6))
    t_count, l_count = timed(lambda: ops.mesh_count(field, 0.0, workspace=ws, totals=totals))
    t_emit, l_emit = timed(lambda: ops.mesh_emit(field, 0.0, lo32, step, ws, vertices, faces, src))

    def both():
        ops.mesh_count(field, 0.0, workspace=ws, totals=totals)
        ops.mesh_emit(field, 0.0, lo32, step, ws, vertices, faces, src)

    t_both, l_both = timed(both)
    # the floor: the field once, the workspace written once and read once, the outputs written once
    floor_bytes = 4 * N + 2 * ws_bytes + 12 * V + 12 * T + 8 * V
    floor_us = floor_bytes / copy_bw * 1e6
    print("    %-34s %s" % ("mesh_count", l_count))
    print("    %-34s %s" % ("mesh_emit", l_emit))
    print("    %-34s %s   (floor %.2f GB: %.1f us at the copy rate; the copy rate's share achieved: %.0f %%)"
          % ("count + emit", l_both, floor_bytes / 1e9, floor_us, 100.0 * floor_us / t_both))
    del vertices, faces, src, ws
