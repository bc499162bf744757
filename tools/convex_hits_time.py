"""k_convex_hits on the 64-box scene as 384 planes against k_bbox_hits on the same boxes: the full 529,408-ray frame, max_hits 8,
hipEvents through benchlib.time_hits, both in one process, alternating (profiles/README.md "convex primitives").
   python tools/convex_hits_time.py [rounds]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import ConvexSet, benchlib, ops, synthetic

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda:0")
rays = synthetic.camera_rays().contiguous().to(dev)
box, ids = synthetic.random_boxes(64, 45, 32)
cs = ConvexSet.from_boxes(box, ids).to(dev)
b = cs.batch()
table = (b["prim_planes"], b["prim_offsets"])
box = box.to(dev)
hb, hc = ops.bbox_hits(rays, box, 8), ops.convex_hits(rays, *table, 8)
same = torch.equal(hb[1], hc[1]) and torch.equal(hb[2], hc[2])
print("%d rays, 64 boxes = %d planes; kept lists identical: %s, max |t| difference %.3g" %
      (rays.shape[0], b["prim_planes"].shape[0], same, float((hb[0] - hc[0]).abs().max())))
for fn in (lambda: benchlib.time_hits(rays, box, 8, 5), lambda: benchlib.time_hits(rays, table, 8, 5)):
    fn()                                                        # warm-up
res = {"bbox": [], "convex": []}
for _ in range(rounds):
    res["bbox"].append(benchlib.time_hits(rays, box, 8, 50))
    res["convex"].append(benchlib.time_hits(rays, table, 8, 50))
for k, v in res.items():
    v = sorted(v)
    print("k_%s_hits  median %7.1f us   min %7.1f   max %7.1f   (%d rounds x 50 launches)" % (k, 1e3 * v[len(v) // 2], 1e3 * v[0], 1e3 * v[-1], rounds))
