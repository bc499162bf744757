"""k_splat_points, k_splat_resolve and k_depth_metrics on the two benchmark frame shapes, hip events (torch.cuda.Event) around a
captured graph of 100 launches, in one process (profiles/README.md "Splatting"): one 100,800-point scan into a 1408 x 376 pinhole
frame and into a 1400 x 1400 fisheye frame at radius 0 and 1 -- spread over the view, and contended (the same number of points
inside a 1.5 degree cone) --, the resolve, and the depth metrics of one frame.  Every splat is preceded by the reset of its
buffer inside the capture (a buffer that already holds the minimum would flatter a pre-read); the reset alone is timed too.
   python tools/splat_time.py [rounds]          (PNR_LIB_PATH selects an A/B build of the library)"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import Fisheye, Pinhole, _lib, camera, ops, synthetic as sy

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda:0")
print("library:", _lib.LIB_PATH)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                       # 100 launches replayed from a capture: the Python front end is not timed
    with torch.cuda.graph(graph):
        for _ in range(100):
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
        us.append(10.0 * e0.elapsed_time(e1))
    us.sort()
    return "median %7.1f us   min %7.1f   max %7.1f" % (us[len(us) // 2], us[0], us[-1])


origin = (0.0, 1.55, 0.0)
spread, _ = sy.lidar_scan(origin, ((0.0, 1.55, 10.0), 30.0), ground_y=3.0, n_azimuth=1800, n_elevation=56)
cone, _ = sy.lidar_scan(origin, ((0.0, 1.55, 10.0), 30.0), n_azimuth=1800, n_elevation=56, azimuth=(-0.75, 0.75), elevation=(-0.75, 0.75))
c2w = torch.tensor([[1.0, 0.0, 0.0, origin[0]], [0.0, 1.0, 0.0, origin[1]], [0.0, 0.0, 1.0, origin[2]]])
w2c = camera.invert_pose(c2w)
cams = {"pinhole 1408 x 376": Pinhole(sy.KITTI_F, sy.KITTI_F, sy.KITTI_CX, sy.KITTI_CY, sy.KITTI_W, sy.KITTI_H),
        "fisheye 1400 x 1400": Fisheye(sy.FISHEYE_XI, sy.FISHEYE_K1, sy.FISHEYE_K2, sy.FISHEYE_GAMMA1, sy.FISHEYE_GAMMA2, sy.FISHEYE_U0,
                                       sy.FISHEYE_V0, sy.FISHEYE_W, sy.FISHEYE_H)}
for name, cam in cams.items():
    z = torch.full((cam.height, cam.width), -1, dtype=torch.int64, device=dev)
    print("%s, %d points" % (name, spread.shape[0]))
    print("    %-44s %s" % ("buffer reset alone", timed(lambda: z.fill_(-1))))
    for kind, pts in (("spread", spread.to(dev)), ("contended", cone.to(dev))):
        for radius in (0, 1):
            st = torch.zeros(3, dtype=torch.int64, device=dev)
            ops.splat_points(cam, w2c, pts, zbuf=z.fill_(-1), radius=radius, stats=st)
            cells = int((z != -1).sum())

            def fn():
                z.fill_(-1)
                ops.splat_points(cam, w2c, pts, zbuf=z, radius=radius)

            print("    %-44s %s   (landed / left / clipped %s, %d cells)" % ("reset + splat, %s, radius %d" % (kind, radius), timed(fn), st.tolist(), cells))
    out = {"depth": torch.empty((cam.height, cam.width), device=dev), "index": torch.empty((cam.height, cam.width), dtype=torch.int32, device=dev)}
    print("    %-44s %s" % ("resolve (depth + index)", timed(lambda: ops.splat_resolve(z, out=out))))
    gt = (10.0 + 5.0 * torch.rand((cam.height, cam.width), device=dev)).contiguous()
    pred = (gt * (0.8 + 0.4 * torch.rand_like(gt))).contiguous()
    sums, counts = torch.zeros(5, dtype=torch.float64, device=dev), torch.zeros(5, dtype=torch.int64, device=dev)
    print("    %-44s %s" % ("depth_metrics, one frame (both kernels)", timed(lambda: ops.depth_metrics(pred, gt, sums=sums, counts=counts))))
