"""FrameSet -- a training set of posed images that lives in GPU memory, and the ray batches drawn from it (include/pnr.h
"training frames"; DESIGN.md "Training frames").  The producer between the cameras (camera.Pinhole / Fisheye / Equirect) and the
training step: `sample()` is ONE kernel (pnr_sample_batch) that picks (frame, pixel) pairs from the set's own Philox stream,
builds their rays and gathers rgb / depth / label targets into the batch dict NetworkWrapper takes.  The frame table is device
memory read when the kernel runs, so a captured training step (train.GraphedStep with `frames=`) draws a fresh batch on every
replay with no host work and no host-to-device copy, and a frame added later is seen by later replays.

Images are stored compactly (rgb uint8, depth float32, labels int16).  Draws are with replacement.  Off-GPU everything here
fails loudly, like the rest of the product path.
"""
import ctypes

import torch

from . import _lib, ops
from .camera import _Camera, _rows3, invert_pose

MODES = ("pooled", "frame")
_REC = ctypes.sizeof(_lib.Frame)


def _image(t, what, H, W, tail=()):
    t = torch.as_tensor(t)
    if tuple(t.shape) != (H, W) + tail:
        raise ValueError("FrameSet.add: %s must be %s (the camera's height, width), not %s" % (what, (H, W) + tail, tuple(t.shape)))
    return t


class FrameSet:
    """
        frames = FrameSet("cuda:0", capacity=256, seed=0)
        frames.add(camera, c2w, near, far, rgb, depth=..., pseudo_label=..., instance_label=...)      # once per posed image
        frames.set_boxes(bbox, bbox_ids)                                                             # the scene's box prior
        batch = frames.sample(4096)                   # rays (1,R,8), rgb, depth, pseudo_label, instance_label, frame, pix (+ boxes)
        ret, loss, stats, _ = wrapper(batch)

    `rng_state` is the set's own (seed, offset) on the device -- not the renderer's, so rendering does not change which batches
    come; every sample() takes one offset.  Restore it (copy_) to draw the same batches again."""

    def __init__(self, device, capacity=1024, seed=0):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("FrameSet: expected a GPU device (the HIP path has no CPU fallback)")
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("FrameSet: capacity must be >= 1")
        self.device, self.seed = dev, int(seed)
        self.table = self.cum = self.n_frames = self.rng_state = None       # device memory: allocated by the first add() / sample()
        self.frames = []            # host side of every record: camera, pose, bounds and the device images (kept alive here)
        self._total = 0
        self._w2c, self._w2c_rows = None, 0      # w2c_table(): the world-to-camera rows of the frames, on the device
        self.bbox = self.bbox_ids = None
        self.prims = None           # set_primitives: {"prim_planes", "prim_offsets", "prim_ids"} on the device

    def _alloc(self):
        if self.table is not None:
            return
        dev = self.device
        if dev.index is None:
            dev = self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = torch.zeros(self.capacity * _REC, dtype=torch.uint8, device=dev)        # pnr_frame records
        self.cum = torch.zeros(self.capacity + 1, dtype=torch.int64, device=dev)
        self.n_frames = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rng_state = torch.tensor([self.seed, 0], dtype=torch.int64, device=dev)

    def __len__(self):
        return len(self.frames)

    @property
    def n_pixels(self):
        """drawable pixels of the whole set (cum[F])"""
        return self._total

    # ------------------------------------------------------------------------------------------------ building the set
    def add(self, camera, c2w, near, far, rgb, depth=None, pseudo_label=None, instance_label=None):
        """Append one posed image.  camera: camera.Pinhole / Fisheye / Equirect; c2w: 3x4 (or 4x4) camera-to-world, host values; rgb
        (H, W, 3) uint8, or float in [0, 1] (rounded to the nearest byte); depth (H, W) float, <= 0 where there is none;
        pseudo_label / instance_label (H, W) integers in the int16 range, -1 = unlabelled.  A fisheye frame draws from
        camera.valid_pix() (lens and user mask), a pinhole or equirect frame from every pixel.  Returns the frame's index.  The record, cum
        and n_frames are updated by stream-ordered copies: launches enqueued later (graph replays included) see the frame."""
        if not isinstance(camera, _Camera):
            raise TypeError("FrameSet.add: camera must be a camera.Pinhole or camera.Fisheye (or camera.Equirect)")
        if len(self.frames) >= self.capacity:
            raise RuntimeError("FrameSet.add: the set is full (capacity = %d frames)" % self.capacity)
        H, W = camera.height, camera.width
        if H * W >= 2 ** 31:
            raise ValueError("FrameSet.add: pixel indices are int32")
        pose = _rows3(torch.as_tensor(c2w, dtype=torch.float32), "FrameSet.add: c2w must be a 3x4 (or 4x4) matrix")
        rgb = _image(rgb, "rgb", H, W, (3,))
        if rgb.dtype != torch.uint8:
            if not rgb.dtype.is_floating_point:
                raise TypeError("FrameSet.add: rgb must be uint8 or float in [0, 1], not %s" % rgb.dtype)
            if rgb.numel() and not bool(((rgb >= 0) & (rgb <= 1)).all()):          # (false for NaN)
                raise ValueError("FrameSet.add: float rgb must lie in [0, 1]")
            rgb = (rgb.to(torch.float32) * 255.0).round().to(torch.uint8)
        imgs = {"rgb": rgb}
        if depth is not None:
            depth = _image(depth, "depth", H, W)
            if not depth.dtype.is_floating_point:
                raise TypeError("FrameSet.add: depth must be a float image, not %s" % depth.dtype)
            imgs["depth"] = depth
        for key, lab in (("sem", pseudo_label), ("inst", instance_label)):
            if lab is None:
                continue
            name = "pseudo_label" if key == "sem" else "instance_label"
            lab = _image(lab, name, H, W)
            if lab.dtype.is_floating_point or lab.dtype == torch.bool:
                raise TypeError("FrameSet.add: %s must be an integer image, not %s" % (name, lab.dtype))
            if lab.numel() and (int(lab.min()) < -2 ** 15 or int(lab.max()) > 2 ** 15 - 1):
                raise ValueError("FrameSet.add: %s is stored as int16: values must lie in [-32768, 32767]" % name)
            imgs[key] = lab
        # every argument is checked: from here on the GPU
        self._alloc()
        dev = self.device
        store = {"rgb": torch.uint8, "depth": torch.float32, "sem": torch.int16, "inst": torch.int16}
        imgs = {k: v.to(dev, store[k]).contiguous() for k, v in imgs.items()}
        pix = None if camera.all_valid else camera.valid_pix(dev)
        if pix is not None and pix.numel() == H * W:
            pix = None
        n_valid = H * W if pix is None else int(pix.numel())
        cam = list(camera.params) + [0.0] * (7 - len(camera.params))
        ptr = lambda t: 0 if t is None else t.data_ptr()
        rec = _lib.Frame(camera.word, W, H, (ctypes.c_float * 7)(*cam),
                         (ctypes.c_float * 12)(*pose.tolist()), float(near), float(far), n_valid, ptr(pix), ptr(imgs["rgb"]),
                         ptr(imgs.get("depth")), ptr(imgs.get("sem")), ptr(imgs.get("inst")))
        i = len(self.frames)
        total = self._total + n_valid
        with torch.cuda.device(dev):
            # record, then cum, then the count: every launch ordered between two of the copies still sees a consistent table
            self.table[i * _REC:(i + 1) * _REC].copy_(torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8))
            self.cum[i + 1:i + 2].copy_(torch.tensor([total], dtype=torch.int64))
            self.n_frames.fill_(i + 1)
        self.frames.append({"camera": camera, "c2w": pose.reshape(3, 4), "near": float(near), "far": float(far), "pix": pix,
                            "n_valid": n_valid, **imgs})
        self._total = total
        return i

    def w2c_table(self):
        """(capacity, 12) float32 on the device: row f = camera.invert_pose of frame f's c2w, the pose table that goes with
        `table` into ops.tsdf_integrate.  Kept on the device; a call after the set grew uploads the new rows only (a
        stream-ordered copy, as add()'s)."""
        self._alloc()
        if self._w2c is None:
            self._w2c = torch.zeros((self.capacity, 12), dtype=torch.float32, device=self.device)
        n = len(self.frames)
        if n > self._w2c_rows:
            rows = torch.stack([invert_pose(fr["c2w"]).reshape(12) for fr in self.frames[self._w2c_rows:n]])
            with torch.cuda.device(self.device):
                self._w2c[self._w2c_rows:n].copy_(rows)
            self._w2c_rows = n
        return self._w2c

    def set_pose(self, i, c2w):
        """Replace the pose of frame i: c2w a 3x4 (or 4x4) camera-to-world, host values (a tracked pose comes back from the device
        with .cpu(): the one read a tracking loop needs per frame).  The frame's record on the device, the host copy and --
        once w2c_table() has been made -- its row there are updated by stream-ordered copies, as add()'s: launches enqueued
        later (graph replays included) see the new pose, launches enqueued before see the old one."""
        try:
            i = int(i)
        except (TypeError, ValueError):
            raise TypeError("FrameSet.set_pose: i must be a frame index") from None
        if not 0 <= i < len(self.frames):
            raise IndexError("FrameSet.set_pose: frame %d of a set of %d" % (i, len(self.frames)))
        pose = torch.as_tensor(c2w)
        if pose.is_cuda:
            raise TypeError("FrameSet.set_pose: c2w must be host values (a device pose: c2w.cpu())")
        pose = _rows3(pose.to(torch.float32), "FrameSet.set_pose: c2w must be a 3x4 (or 4x4) matrix").clone()
        if not bool(torch.isfinite(pose).all()):
            raise ValueError("FrameSet.set_pose: c2w must be finite")
        off = i * _REC + _lib.Frame.c2w.offset
        with torch.cuda.device(self.device):
            self.table[off:off + 48].copy_(pose.view(torch.uint8))
            if self._w2c is not None and i < self._w2c_rows:
                self._w2c[i].copy_(invert_pose(pose).reshape(12))
        self.frames[i]["c2w"] = pose.reshape(3, 4)

    def set_boxes(self, bbox, bbox_ids):
        """The scene's 3D box prior, returned in every batch: bbox (M, 15), bbox_ids (M, 2) (ops.bbox_hits' layout).  A second
        call with the same number of boxes writes into the tensors of the first, so batches handed out before -- the static batch
        of a captured step -- see the new values; another number of boxes makes new tensors, which only later sample() calls return
        (a captured graph fixes shapes: a train.GraphedStep keeps the boxes it was built with)."""
        if self.prims is not None:
            raise ValueError("FrameSet.set_boxes: the set has primitives (set_primitives) -- one prior per set: ConvexSet.from_boxes "
                             "turns boxes into primitives")
        bbox, bbox_ids = torch.as_tensor(bbox), torch.as_tensor(bbox_ids)
        if bbox.dim() != 2 or bbox.shape[1] != 15:
            raise ValueError("FrameSet.set_boxes: bbox must be (M, 15), not %s" % (tuple(bbox.shape),))
        if tuple(bbox_ids.shape) != (bbox.shape[0], 2):
            raise ValueError("FrameSet.set_boxes: bbox_ids must be (%d, 2), not %s" % (bbox.shape[0], tuple(bbox_ids.shape)))
        if bbox_ids.dtype.is_floating_point or bbox_ids.dtype == torch.bool:
            raise TypeError("FrameSet.set_boxes: bbox_ids must be integers, not %s" % bbox_ids.dtype)
        bbox, bbox_ids = bbox.to(self.device, torch.float32).contiguous(), bbox_ids.to(self.device, torch.int32).contiguous()
        if self.bbox is not None and self.bbox.shape == bbox.shape:
            self.bbox.copy_(bbox)                  # in place: batches handed out before (a captured step's static batch) see the new boxes
            self.bbox_ids.copy_(bbox_ids)
        else:
            self.bbox, self.bbox_ids = bbox, bbox_ids

    def set_primitives(self, convex_set):
        """The scene's prior as convex primitives (primitives.ConvexSet), returned in every batch as prim_planes (P,4),
        prim_offsets (M+1), prim_ids (M,2) -- what Renderer.render takes instead of bbox / bbox_ids.  Like set_boxes: a second
        call with the same numbers of planes and primitives writes into the tensors of the first (a captured step's static
        batch sees the new table), other shapes make new tensors.  Not together with set_boxes (ConvexSet.from_boxes)."""
        if self.bbox is not None:
            raise ValueError("FrameSet.set_primitives: the set has boxes (set_boxes) -- one prior per set: ConvexSet.from_boxes "
                             "turns them into primitives")
        if not all(hasattr(convex_set, k) for k in ("planes", "offsets", "ids")):
            raise TypeError("FrameSet.set_primitives: expected a primitives.ConvexSet")
        new = {"prim_planes": torch.from_numpy(convex_set.planes.copy()), "prim_offsets": torch.from_numpy(convex_set.offsets.copy()),
               "prim_ids": torch.from_numpy(convex_set.ids.copy())}
        new = {k: v.to(self.device).contiguous() for k, v in new.items()}
        if self.prims is not None and all(self.prims[k].shape == v.shape for k, v in new.items()):
            for k, v in new.items():
                self.prims[k].copy_(v)              # in place: batches handed out before see the new table
        else:
            self.prims = new

    # ------------------------------------------------------------------------------------------------ batches
    _KEYS = (("rays", "rays"), ("rgb", "rgb"), ("depth", "depth"), ("pseudo_label", "sem"), ("instance_label", "inst"),
             ("frame", "frame"), ("pix", "pix"))

    def sample(self, n_rays, mode="pooled", rank=0, world=1, out=None):
        """A training batch of n_rays rays: {rays (1,R,8), rgb (1,R,3), depth (1,R), pseudo_label, instance_label (1,R) int32,
        frame, pix (R) int32} plus bbox / bbox_ids when set_boxes was called (prim_planes / prim_offsets / prim_ids after set_primitives) -- what NetworkWrapper takes.  mode "pooled": every
        drawable pixel of the set is equally likely; "frame": one frame per call (the same on every rank), then pixels of it.
        Rank `rank` of `world` draws global rays rank * n_rays ...: the ranks' batches concatenated are, bit for bit, the
        world * n_rays batch of one rank (every rank holds the same set and state).  out: a batch this method returned before,
        written in place (a captured graph's static batch).  One kernel after rng_begin; nothing is copied or synchronised."""
        if mode not in MODES:
            raise ValueError("FrameSet.sample: mode must be 'pooled' or 'frame', not %r" % (mode,))
        n_rays, rank, world = int(n_rays), int(rank), int(world)
        if n_rays < 0:
            raise ValueError("FrameSet.sample: n_rays must be >= 0")
        if world < 1 or not 0 <= rank < world:
            raise ValueError("FrameSet.sample: need world >= 1 and 0 <= rank < world (got rank %d, world %d)" % (rank, world))
        if world * n_rays > 2 ** 32:
            raise ValueError("FrameSet.sample: world * n_rays exceeds the 2^32 rays of one draw")
        if out is not None and any(k not in out for k, _ in self._KEYS):
            raise ValueError("FrameSet.sample: out must be a batch that sample() returned")
        self._alloc()
        with torch.cuda.device(self.device):
            call = ops.rng_begin(self.rng_state)
            flat = None if out is None else {n: (out[k] if k in ("frame", "pix") else out[k][0]) for k, n in self._KEYS}
            res = ops.sample_batch(self.table, self.cum, self.n_frames, ops.Draw(call, _lib.TAG_PIXEL, rank * n_rays), n_rays, mode,
                                   out=flat)
        if out is not None:
            return out
        batch = {k: (res[n] if k in ("frame", "pix") else res[n][None]) for k, n in self._KEYS}
        if self.bbox is not None:
            batch.update(bbox=self.bbox, bbox_ids=self.bbox_ids)
        if self.prims is not None:
            batch.update(self.prims)
        return batch

    def frame_batch(self, i):
        """Frame i as an evaluation batch: the rays of its drawable pixels (camera.rays) and their targets, in the layout of
        sample() -- rays (1,P,8), rgb (1,P,3) float, depth (1,P) (0 without a depth image), labels (1,P) int32 (-1 without),
        frame, pix (P) int32, boxes.  Plain torch indexing: evaluation is not the hot path."""
        fr = self.frames[i]
        cam, dev = fr["camera"], self.device
        pix = fr["pix"]
        P = fr["n_valid"]
        idx = slice(None) if pix is None else pix.long()
        rays = cam.rays(fr["c2w"], fr["near"], fr["far"], pix=pix, device=dev)
        # rgb: the byte over 255 in float64, then rounded -- for all 256 bytes the correctly rounded float32 quotient sample() writes
        batch = {"rays": rays[None], "rgb": (fr["rgb"].reshape(-1, 3)[idx].to(torch.float64) / 255.0).to(torch.float32)[None],
                 "depth": (fr["depth"].reshape(-1)[idx] if "depth" in fr else torch.zeros(P, device=dev))[None]}
        for k, n in (("pseudo_label", "sem"), ("instance_label", "inst")):
            batch[k] = (fr[n].reshape(-1)[idx].to(torch.int32) if n in fr else torch.full((P,), -1, dtype=torch.int32, device=dev))[None]
        batch["frame"] = torch.full((P,), int(i), dtype=torch.int32, device=dev)
        batch["pix"] = pix if pix is not None else torch.arange(P, dtype=torch.int32, device=dev)
        if self.bbox is not None:
            batch.update(bbox=self.bbox, bbox_ids=self.bbox_ids)
        if self.prims is not None:
            batch.update(self.prims)
        return batch
