"""k_gen_rays_equirect and k_reproject with a panoramic view on one side, on the benchmark shapes (profiles/README.md "Panoramic
camera"): the 1408 x 704 full-sphere panorama and the 1400 x 1400 fisheye at one place, 0.5 m and 3 degrees apart, depth images of
a sphere around the cameras.  Hip events (torch.cuda.Event) around a captured graph of 100 launches, in one process; the timing
loop is tools/reproject_time.py's.
   python tools/pano_time.py [rounds]"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticnerf_amd import Fisheye, camera, ops, synthetic as sy

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


def timed(name, fn):
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
    print("    %-52s median %7.1f us   min %7.1f   max %7.1f   (%d rounds x 100 launches)" % (name, 1e3 * ms[len(ms) // 2], 1e3 * ms[0], 1e3 * ms[-1], rounds))


pano, _ = sy.equirect_camera()
fish = Fisheye(sy.FISHEYE_XI, sy.FISHEYE_K1, sy.FISHEYE_K2, sy.FISHEYE_GAMMA1, sy.FISHEYE_GAMMA2, sy.FISHEYE_U0, sy.FISHEYE_V0, sy.FISHEYE_W, sy.FISHEYE_H)
ca, cb = pose(0.0, 0.0, (0.0, 1.55, 0.0)), pose(0.05, -0.03, (0.3, 1.5, 0.4))
dp, df = sphere_depth(pano, ca), sphere_depth(fish, cb)
print("%d x %d panorama, %d x %d fisheye" % (pano.width, pano.height, fish.width, fish.height))
timed("k_gen_rays<equirect>, whole frame (991,232 rays)", lambda: pano.rays(ca, 0.5, 100.0, device=dev))
timed("k_gen_rays<fisheye>, whole frame (1,960,000 rays)", lambda: fish.rays(cb, 0.5, 100.0, device=dev))
out_p = {"match": torch.empty(pano.width * pano.height, dtype=torch.int32, device=dev)}
out_f = {"match": torch.empty(fish.width * fish.height, dtype=torch.int32, device=dev)}
wb, wa = camera.invert_pose(cb), camera.invert_pose(ca)
for name, args, out in (("panorama -> fisheye", (pano, ca, dp, fish, wb, df), out_p), ("fisheye -> panorama", (fish, cb, df, pano, wa, dp), out_f),
                        ("panorama -> panorama", (pano, ca, dp, pano, wb, sphere_depth(pano, cb)), out_p)):
    print("%s: matched / -1 / -2 / -3 / -4 = %s" % (name, ops.reproject(*args, want=("stats",))["stats"].tolist()))
    timed(name + ", match + depth test", lambda: ops.reproject(*args, out=out))
