"""k_reproject on the two benchmark frame shapes, hip events (torch.cuda.Event) around a captured graph of 100 launches, in one process
(profiles/README.md "Reprojection"): a 1408 x 376 pinhole pair and a 1400 x 1400 fisheye pair, 0.5 m and 3 degrees apart, depth
images of a sphere around the cameras; match only, with the depth test, and with the 45-class agree / stats accumulators.
   python tools/reproject_time.py [rounds]"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import Fisheye, Pinhole, camera, ops, synthetic as sy

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda:0")


def pose(yaw, pitch, origin):
    cy, sy_, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    ry = torch.tensor([[cy, 0.0, sy_], [0.0, 1.0, 0.0], [-sy_, 0.0, cy]], dtype=torch.float64)
    rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]], dtype=torch.float64)
    return torch.cat([ry @ rx, torch.tensor(origin, dtype=torch.float64).reshape(3, 1)], 1).float()


def sphere_depth(cam, c2w, radius=20.0):
    """depth image of a sphere around the world origin in the camera's own convention (the ray parameter of cam.rays)"""
    r = cam.rays(c2w, 0.0, 1.0, device=dev)
    o, d = r[:, :3].double(), r[:, 3:6].double()
    a, b, c = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - radius * radius
    t = (-b + torch.sqrt(b * b - a * c)) / a.clamp(min=1e-30)
    return torch.where(a > 0, t, torch.zeros_like(t)).float().reshape(cam.height, cam.width).contiguous()


ca, cb = pose(0.0, 0.0, (0.0, 1.55, 0.0)), pose(0.05, -0.03, (0.3, 1.5, 0.4))
w2c = camera.invert_pose(cb)
cams = {"pinhole 1408 x 376": Pinhole(sy.KITTI_F, sy.KITTI_F, sy.KITTI_CX, sy.KITTI_CY, sy.KITTI_W, sy.KITTI_H),
        "fisheye 1400 x 1400": Fisheye(sy.FISHEYE_XI, sy.FISHEYE_K1, sy.FISHEYE_K2, sy.FISHEYE_GAMMA1, sy.FISHEYE_GAMMA2, sy.FISHEYE_U0,
                                       sy.FISHEYE_V0, sy.FISHEYE_W, sy.FISHEYE_H)}
for name, cam in cams.items():
    da, db = sphere_depth(cam, ca), sphere_depth(cam, cb)
    g = torch.Generator().manual_seed(0)
    la = torch.randint(0, 45, (cam.height, cam.width), generator=g, dtype=torch.int32).to(dev)
    agree, stats = torch.zeros((45, 45), dtype=torch.int64, device=dev), torch.zeros(5, dtype=torch.int64, device=dev)
    out = {"match": torch.empty(cam.width * cam.height, dtype=torch.int32, device=dev)}
    arms = {"match, no depth test": lambda: ops.reproject(cam, ca, da, cam, w2c, out=out),
            "match + depth test": lambda: ops.reproject(cam, ca, da, cam, w2c, db, out=out),
            "match + depth test + agree (45) + stats": lambda: ops.reproject(cam, ca, da, cam, w2c, db, label_src=la, label_tgt=la, n_classes=45,
                                                                               agree=agree, stats=stats, out=out)}
    s = ops.reproject(cam, ca, da, cam, w2c, db, want=("stats",))["stats"].tolist()
    print("%s: matched / -1 / -2 / -3 / -4 = %s" % (name, s))
    for arm, fn in arms.items():
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()                       # 100 launches replayed from a capture: the Python front end is not timed
        with torch.cuda.graph(graph):
            for _ in range(100):
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
            ms.append(e0.elapsed_time(e1) / 100)
        ms.sort()
        print("    %-42s median %7.1f us   min %7.1f   max %7.1f   (%d rounds x 100 launches)" % (arm, 1e3 * ms[len(ms) // 2], 1e3 * ms[0], 1e3 * ms[-1], rounds))
