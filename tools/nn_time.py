"""pnr_nn_build and pnr_nn_query on a room-sized cloud, hip events (torch.cuda.Event) around a captured graph of 20 launches, in
one process (profiles/README.md "Nearest neighbours"): the surface points of synthetic.room_depth seen through an equirect
camera, lifted; n of them are the reference cloud, n others, moved by a few centimetres, the queries, at D = 0.05 m.  Reports the
build and the query time, the cloud metrics of the answers (both kernels), the records tested per query (counted with torch from the table the build made), the bytes the query
moves per second, the device's clocks, and -- for scale, not a pass mark -- a chunked torch.cdist brute force on a subset.
   python tools/nn_time.py [n] [rounds] [brute force subset]          (PNR_LIB_PATH selects an A/B build of the library)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from panopticnerf_amd import Equirect, _lib, ops, pointcloud, synthetic as sy

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n_brute = int(sys.argv[3]) if len(sys.argv) > 3 else 100000
D, REPS = 0.05, 20
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
    return us[len(us) // 2], "median %8.1f us   min %8.1f   max %8.1f" % (us[len(us) // 2], us[0], us[-1])


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
    lines = [l.strip() for l in out.splitlines() if any(k in l for k in ("sclk", "mclk", "fclk", "rocm-smi:"))]
    return lines, busy


# a 6 x 3 x 8 m room seen from inside: 2 n + pixels of an equirect image, lifted
side = 1
while 2 * side * side < 2 * n + 1000:
    side += 1
cam = Equirect(2 * side, side)
c2w = torch.tensor([[1.0, 0.0, 0.0, 0.3], [0.0, 1.0, 0.0, 1.55], [0.0, 0.0, 1.0, -0.4]])
depth = sy.room_depth(cam, c2w, (-3.0, 0.0, -4.0), (3.0, 3.0, 4.0)).to(dev)
points, _ = pointcloud.lift((cam, c2w, {"depth": depth}), "depth")
perm = torch.randperm(points.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(0))
ref = points[perm[:n]].contiguous()
query = (points[perm[n:2 * n]] + 0.02 * torch.randn((n, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(1))).contiguous()
assert ref.shape[0] == n and query.shape[0] == n
_, T = ops.nn_params("nn_time", D, n)
start = torch.empty(T + 1, dtype=torch.int32, device=dev)
records = torch.empty((n, 4), device=dev)
index, dist2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
stats = torch.zeros(3, dtype=torch.int64, device=dev)
ops.nn_build(ref, D, start=start, records=records)
ops.nn_query(ref, start, records, query, D, index=index, dist2=dist2, stats=stats)
found, none, invalid = stats.tolist()

# records tested per query: the rule's cells and buckets in torch float32 (a statistic: the kernel's own arithmetic is tested elsewhere)
dp = torch.tensor(D, dtype=torch.float32) * 1.0009765625
inv = (1.0 / (2.0 * dp)).to(dev)
c0 = torch.floor((query - dp.to(dev) - ref[0]) * inv).clamp(-2 ** 20, 2 ** 20).to(torch.int64)
c1 = torch.floor((query + dp.to(dev) - ref[0]) * inv).clamp(-2 ** 20, 2 ** 20).to(torch.int64)
tested, buckets = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
span = int((c1 - c0).max())
mult = torch.tensor([73856093, 19349663, 83492791], dtype=torch.int64, device=dev)
for dz in range(span + 1):
    for dy in range(span + 1):
        for dx in range(span + 1):
            c = c0 + torch.tensor([dx, dy, dz], device=dev)
            inside = (c <= c1).all(dim=1)
            w = (c & 0xFFFFFFFF) * mult & 0xFFFFFFFF
            b = (w[:, 0] ^ w[:, 1] ^ w[:, 2]) & (T - 1)
            tested += torch.where(inside, (start[b + 1] - start[b]).to(torch.int64), torch.zeros_like(tested))
            buckets += inside.to(torch.int64)
per_query, per_bucket = float(tested.sum()) / n, float(buckets.sum()) / n
print("%d reference points, %d queries, D = %g m, table of %d buckets (largest %d records)" % (n, n, D, T, int((start[1:] - start[:-1]).max())))
print("    found / none in radius / invalid: %d / %d / %d;   buckets visited per query %.2f, records tested per query %.1f" % (found, none, invalid, per_bucket, per_query))
us_b, line = timed(lambda: ops.nn_build(ref, D, start=start, records=records))
print("    %-40s %s" % ("build (zero, count, scan, fill)", line))
us_q, line = timed(lambda: ops.nn_query(ref, start, records, query, D, index=index, dist2=dist2))
moved = n * (12 + 8 + 8 * per_bucket + 16 * per_query)          # query, outputs, a start pair per bucket, 16 bytes per record
print("    %-40s %s   (%.1f GB/s asked of the memory system, %.1f Mqueries/s)" % ("query", line, moved / us_q / 1e3, n / us_q))
cm_sums, cm_counts = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(10, dtype=torch.int64, device=dev)
_, line = timed(lambda: ops.cloud_metrics(index, dist2, D, (0.01, 0.02, 0.05), query=query, sums=cm_sums, counts=cm_counts))
print("    %-40s %s" % ("cloud_metrics (both kernels)", line))
lines, busy = clocks_while(lambda: ops.nn_query(ref, start, records, query, D, index=index, dist2=dist2))
print("    clocks read %s:" % ("while the query ran" if busy else "AFTER the queued queries had finished"))
for l in lines:
    print("        " + l)

# for scale: brute force through torch.cdist on a subset, chunked so that the distance matrix stays small
k = min(n_brute, n)
rs, qs = ref[:k], query[:k]


def brute():
    out = []
    for i in range(0, k, 8192):
        d, j = torch.cdist(qs[i:i + 8192], rs).min(dim=1)
        out.append(torch.where(d <= D, j, torch.full_like(j, -1)))
    return torch.cat(out)


brute()
torch.cuda.synchronize()
ms = []
for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    bi = brute()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
sub = pointcloud.NearestIndex(rs, D).query(qs)["index"]
us_s, line = timed(lambda: pointcloud.NearestIndex(rs, D).query(qs), reps=5)
print("    %-40s median %8.1f us   (%d x %d; the index, build + query: %.1f us; answers that differ: %d -- cdist is not the rule's arithmetic)"
      % ("torch.cdist brute force, chunked", 1000.0 * sorted(ms)[1], k, k, us_s, int((bi != sub.long()).sum())))
