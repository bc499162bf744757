"""Does a captured hipMemsetAsync replay?  (DESIGN 8 "Nearest neighbours and geometry metrics", Build; profiles/README.md "Nearest
neighbours".)  A: the runtime's own call on a torch tensor in a chain memset -> add_ -> copy, captured with torch.cuda.graph and
replayed three times over a dirtied buffer, at four sizes.  B: ops.mesh_count, whose entry point clears its totals with a 16-byte
hipMemsetAsync, captured and replayed over dirtied totals.  Wrong VALUES are the finding; nothing is written outside its buffer.
   python tools/memset_capture_probe.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import _lib, ops, synthetic
dev = torch.device("cuda:0")
_lib.load()
torch.zeros(1, device=dev)
paths = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l})
print("hip runtime mapped:", [os.path.basename(p) for p in paths])
hip = ctypes.CDLL(paths[0])
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
for N in (2, 2048, 2048 + 3, 1 << 21):
    buf = torch.full((N,), 7, dtype=torch.int32, device=dev)
    out = torch.empty_like(buf)
    def chain():
        rc = hip.hipMemsetAsync(buf.data_ptr(), 0, N * 4, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        buf.add_(1)
        out.copy_(buf)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    res = []
    for trial in range(3):
        buf.fill_(7)
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        res.append(sorted(out.unique().tolist()))
    print("A: N = %d: values of out after each replay (1 = the memset ran before the kernel): %s" % (N, res), flush=True)
field = synthetic.sdf_grid("sphere", (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 16, radius=0.7, device=dev)
totals, ws = ops.mesh_count(field, 0.0)
torch.cuda.synchronize()
want = totals.tolist()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    ops.mesh_count(field, 0.0, workspace=ws, totals=totals)
res = []
for trial in range(3):
    totals.fill_(12345)
    g.replay()
    torch.cuda.synchronize()
    res.append(totals.tolist())
print("B: mesh_count eager totals %s, after each replay over dirtied totals: %s" % (want, res))
