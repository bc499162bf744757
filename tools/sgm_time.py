"""The stereo matcher's stages on one 1408 x 376 pair at D = 128, paths 4 and 8 (profiles/README.md "Stereo"): k_census (both
images), the aggregation (one k_sgm_path launch per direction), the selection (k_sgm_right + k_sgm_select), k_disparity_depth,
and the whole of stereo.sgm + depth -- hip events (torch.cuda.Event) around a captured graph of 10 runs, in one process.  The
pair is a random-dot stereogram (synthetic.stereo_pair): the kernels' work does not depend on the image content.
Beside each aggregation time: the bytes that form must move (S stored once and read + written by every later direction) and
what they cost at the HBM rate given on the command line.
   python tools/sgm_time.py [rounds] [hbm_TB_per_s]         (PNR_LIB_PATH selects an A/B build of the library)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import Pinhole, _lib, ops, stereo, synthetic as sy

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
hbm = float(sys.argv[2]) if len(sys.argv) > 2 else 8.0
REPS = 10
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


H, W, D = sy.KITTI_H, sy.KITTI_W, 128
left, right, _, _ = sy.stereo_pair(H, W, layers=((5, None), (40, (0.3, 0.9, 0.2, 0.5)), (90, (0.5, 1.0, 0.6, 0.9))), seed=0, device=dev)
cam = Pinhole(sy.KITTI_F, sy.KITTI_F, sy.KITTI_CX, sy.KITTI_CY, W, H)
cl, cr = torch.empty((H, W), dtype=torch.int64, device=dev), torch.empty((H, W), dtype=torch.int64, device=dev)
S = torch.empty((H, W, D), dtype=torch.int16, device=dev)
d16, dR = torch.empty((H, W), dtype=torch.int16, device=dev), torch.empty((H, W), dtype=torch.int16, device=dev)
z = torch.empty((H, W), device=dev)
vol = H * W * D * 2
print("%d x %d pair, D = %d: S is %.1f MB; HBM rate assumed %.1f TB/s" % (W, H, D, vol / 1e6, hbm))


def census_both():
    ops.census(left, out=cl)
    ops.census(right, out=cr)


print("    %-44s %s" % ("census, both images", timed(census_both)[1]))
for paths in (4, 8):
    t, line = timed(lambda: ops.sgm_aggregate(cl, cr, D, 10, 120, paths, out=S))
    moved = vol * (2 * paths - 1) + paths * 2 * H * W * 8       # S: one store, then a read and a write per direction; the census words once per direction
    floor = moved / (hbm * 1e12) * 1e6
    print("    %-44s %s   (%.2f GB to move: %.1f us at the HBM rate, %.1fx that)" % ("aggregate, paths %d" % paths, line, moved / 1e9, floor, t / floor))
    t, line = timed(lambda: ops.sgm_select(S, 5, 1, out=d16, disp_right=dR))
    print("    %-44s %s   (S read twice: %.1f us at the HBM rate)" % ("select (right table + left), after paths %d" % paths, line, 2 * vol / (hbm * 1e12) * 1e6))
    print("    %-44s %s" % ("select, no left-right check", timed(lambda: ops.sgm_select(S, 5, -1, out=d16))[1]))
    print("    %-44s %s" % ("disparity_depth", timed(lambda: ops.disparity_depth(d16, 331.5, out=z))[1]))
    print("    %-44s %s" % ("stereo.depth_from_pair, paths %d (all of it)" % paths, timed(lambda: stereo.depth_from_pair(left, right, cam, 0.6, max_disp=D, paths=paths))[1]))
    print("    valid pixels: %.3f" % float((d16 >= 0).float().mean()))
