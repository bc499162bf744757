"""The DEVICE weight packer (pnr_mlp_pack_device, pnr_mlp_repack_device: k_pack_fragments) and the image cache around it
(Network._pack), byte for byte against the host packer.  Every render of a GPU-resident network reads images that come from this
kernel and this cache; the kernel sweeps upload host-packed images and never touch either.  SURVEY.md 8a row a5.

Every comparison is exact.  The reference is the host packer (pnr_mlp_pack, pnr_mlp_pack_bwd), which test_pack_values.py holds to
the layout header's rounding rule and which the float64 sweeps of the MLP kernels run on.

  * every geometry of _pack_cases.geometries() x every plan the library accepts x bf16 / fp32 x forward / transposed: the whole
    image [0, total_bytes), header and chunk table included, and the three size functions;
  * image and workspace are interior views of one sentinel-filled allocation (_arena.ByteArena): nothing outside them, and
    nothing of the workspace behind the descriptors, is written; the alignment gap between the chunk table and the data area is
    left as the caller handed it in (the host packer zeroes it; ops.pack_mlp_device hands in zeros); a repack writes the data
    area alone;
  * the three regimes of the kernel's grid-stride loop (2048 workgroups): <= 2048, 2049 .. 4096 and > 4096 fragments;
  * NaNs, infinities, signed zeros, subnormals, FLT_MAX and ties planted in the parameters (test_pack_values.py's list);
  * repack after in-place edits, inside a captured graph, on a side stream, and its refusal of parameters that were packed
    from a temporary copy;
  * Network.packed / packed_bwd on the GPU for every key, in eval and training mode, across .data writes, mode switches,
    replaced storage, a .double() network and a real optimiser step."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _pack_cases as pc
from _arena import BYTE_SENTINEL, ByteArena
from panopticnerf_amd import _lib, make_network, make_renderer, ops, synthetic

pytestmark = pytest.mark.gpu

FRAG_DESC_BYTES = 80            # sizeof(PnrFragDesc): two pointers and fifteen 32-bit words, padded to 8


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _to(params, dev):
    return {k: v.to(dev) for k, v in params.items()}


class Pack:
    """pnr_mlp_pack_device / pnr_mlp_repack_device through the C entry points, image and workspace exactly as long as the size
    functions say, inside a ByteArena.  fill: what the image holds before the call (None: the sentinel)."""

    def __init__(self, dev, desc, params_dev, backward, fill=0):
        self.lib, self.desc, self.backward, self.params = _lib.load(), desc, int(backward), params_dev
        size = self.lib.pnr_mlp_bwd_packed_bytes if backward else self.lib.pnr_mlp_packed_bytes
        self.nbytes = int(size(ctypes.byref(desc)))
        self.wbytes = int(self.lib.pnr_mlp_pack_workspace_bytes(ctypes.byref(desc), self.backward))
        assert self.nbytes > 0 and self.wbytes > 0
        self.arena = ByteArena(dev, [("img", self.nbytes), ("ws", self.wbytes)])
        self.img, self.ws = self.arena.view("img"), self.arena.view("ws")
        if fill is not None:
            self.img.fill_(fill)
        self.run(self.lib.pnr_mlp_pack_device, "pnr_mlp_pack_device")

    def run(self, fn, name):
        P, keep = ops._param_struct(self.desc, self.params, self.img.device)
        assert {t.data_ptr() for t in keep if isinstance(t, torch.Tensor)} <= {t.data_ptr() for t in self.params.values()}     # no copies
        _lib.check(fn(ctypes.byref(self.desc), ctypes.byref(P), self.backward, _p(self.ws), _p(self.img),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
        torch.cuda.synchronize()

    def repack(self):
        self.run(self.lib.pnr_mlp_repack_device, "pnr_mlp_repack_device")

    def check_sizes(self, hdr):
        """the three size functions against the header of the image: what the test allocated is what the packer needs"""
        assert hdr["total_bytes"] == self.nbytes and hdr["data_off"] % 1024 == 0 and hdr["gap"][0] <= hdr["gap"][1]
        assert self.wbytes == (self.nbytes // 1024 + 1) * FRAG_DESC_BYTES and hdr["n_frags"] * FRAG_DESC_BYTES <= self.wbytes

    def check_guards(self, hdr):
        assert self.arena.guards_intact(), "written outside the image or the workspace"
        assert bool((self.ws[hdr["n_frags"] * FRAG_DESC_BYTES:] == BYTE_SENTINEL).all()), "workspace written behind the descriptors"


# ------------------------------------------------------------------------------------------ every plan of every geometry
GEOMS = pc.geometries()


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: pc.GEOM_ID % g)
def test_device_image_equals_host_image(dev, geom):
    params = pc.random_params(geom, seed=GEOMS.index(geom))
    params_dev = _to(params, dev)
    done = []
    for label, desc, backward in pc.images(geom):
        host = pc.host_image(desc, params, backward)
        hdr = pc.header(host)
        assert host.numel() == hdr["total_bytes"]
        run = Pack(dev, desc, params_dev, backward)                  # the gap as ops.pack_mlp_device hands it in: zeros
        run.check_sizes(hdr)
        run.check_guards(hdr)
        got = run.img.cpu()
        assert torch.equal(got[:hdr["data_off"]], host[:hdr["data_off"]]), "%s: header / chunk table" % label
        bad = (got != host).nonzero()
        assert bad.numel() == 0, "%s: %d bytes differ, the first in fragment %d" % (label, bad.numel(), (int(bad[0]) - hdr["data_off"]) // 1024)
        done.append(label)
    print("%d images compared: %s" % (len(done), " ".join(done)))


def test_every_plan_precision_and_direction_occurs_at_both_widths():
    """the list above, counted on the host: plans 0, 3 and 4, fp32 and the transposed image at W = 128; plans 0 .. 4, fp32 and the
    transposed image at W = 256 (plans 1 and 2 exist for 256-wide networks only)"""
    seen, n = {128: set(), 256: set()}, 0
    for g in GEOMS:
        for label, desc, backward in pc.images(g):
            seen[g[1]].add(label)
            n += 1
    print("%d (geometry, plan, precision, direction) images over %d geometries" % (n, len(GEOMS)))
    common = {"bf16/plan0/fwd", "bf16/plan3/fwd", "bf16/plan4/fwd", "fp32/plan0/fwd", "bf16/plan0/bwd"}
    assert seen[128] == common and seen[256] == common | {"bf16/plan1/fwd", "bf16/plan2/fwd"}
    assert 100 <= len(GEOMS) < 1000


# ------------------------------------------------------------------------------------------------- grid-stride regimes
TRIPS = [   # geometry, precision, fragments: lo < n <= hi
    ((2, 128, -1, 0, 0, "trunk", 2, 10, 4), "bf16", 0, 2048),
    ((16, 256, 14, 45, 32, "trunk", 2, 10, 4), "bf16", 2048, 4096),
    ((16, 256, 14, 256, 256, "trunk", 2, 10, 4), "fp32", 4096, 1 << 20),
]


@pytest.mark.parametrize("geom,prec,lo,hi", TRIPS, ids=["one_trip", "two_trips", "three_trips"])
def test_grid_stride_trips(dev, geom, prec, lo, hi):
    """k_pack_fragments runs min(n, 2048) workgroups, each striding over the fragments: one image whose fragments need one trip
    of that loop, one that needs two, one that needs three or more.  The count is read from the DEVICE image's header."""
    params = pc.random_params(geom, seed=7)
    desc = pc.make_desc(geom, prec)
    run = Pack(dev, desc, _to(params, dev), False)
    got = run.img.cpu()
    hdr = pc.header(got)
    n = (hdr["total_bytes"] - hdr["data_off"]) // 1024
    print("%s %s: %d fragments, %d trip(s)" % (pc.GEOM_ID % geom, prec, n, -(-n // 2048)))
    assert lo < n <= hi
    run.check_sizes(hdr)
    run.check_guards(hdr)
    assert torch.equal(got, pc.host_image(desc, params))


# ------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("geom,prec,backward", [(pc.PLANT_GEOM, "bf16", 0), (pc.PLANT_GEOM, "fp32", 0), (pc.PLANT_GEOM_BWD, "bf16", 1),
                                                (pc.PLANT_GEOM_BWD, "bf16", 0)], ids=["bf16_fwd", "fp32_fwd", "bf16_bwd", "bf16_fwd_40"])
def test_planted_values(dev, geom, prec, backward):
    """NaNs of every kind, +-Inf, +-0, subnormals, FLT_MAX and ties: the device image is the host's, byte for byte; it is also
    what the restatement of the rounding rule gives (fp32 images and bias fragments: the bits verbatim); and no subnormal was
    flushed on the way through the kernel"""
    params, places = pc.planted_params(geom, seed=3)
    desc = pc.make_desc(geom, prec)
    host = pc.host_image(desc, params, backward)
    hdr = pc.header(host)
    run = Pack(dev, desc, _to(params, dev), backward)
    got = run.img.cpu()
    assert torch.equal(got, host)
    run.check_guards(hdr)
    smap = pc.source_map(geom, desc, backward)
    data = got[hdr["data_off"]:].numpy()
    assert np.array_equal(data, pc.expected_data(geom, desc, params, backward, smap=smap))
    wide = prec == "fp32" and not backward
    words = data.view(np.uint32 if wide else np.uint16)
    kept = 0
    for name, index, bits in places:
        if bits not in pc.SUBNORMALS:
            continue
        rounded = not wide and not name.endswith(".bias")
        want = int(pc.f32_to_bf16(np.array([bits], np.uint32))[0]) << 16 if rounded else bits
        for at in pc.word_of(smap, geom, name, index):
            if wide:
                word = int(words[at])
            elif rounded:
                word = int(words[at]) << 16
            else:
                word = int(words[at]) << 16 | int(words[at - 1])
            assert word == want, (name, index, hex(want), hex(word))
            kept += bool(word & 0x7FFFFFFF) and not (word & 0x7F800000)
    print("%d subnormal words in the device image" % kept)
    assert kept >= (6 if backward else 12)


# ----------------------------------------------------------------------------------------------------- guards and repack
REPACK_GEOMS = [(8, 256, 4, 45, 32, "trunk", 2, 10, 4), (3, 128, 1, 31, 33, "feature", 2, 3, 1)]
EDITED = ["pts_linears.1.weight", "pts_linears.0.bias", "pts_linears.2.bias", "alpha_linear.weight", "alpha_linear.bias", "feature_linear.weight",
          "views_linears.0.bias", "rgb_linear.weight", "semantic_linears.0.weight", "semantic_linears.1.weight", "semantic_linears.1.bias",
          "instance_linears.1.weight", "instance_linears.0.bias"]


def _edit(params_dev, step):
    """in-place updates of weights and biases of the trunk and of every head; returns the new values on the host"""
    for i, k in enumerate(EDITED):
        params_dev[k].mul_(1.0 + 0.25 * step).add_(0.125 * (i + 1) * step)
    return {k: v.cpu() for k, v in params_dev.items()}


@pytest.mark.parametrize("geom", REPACK_GEOMS, ids=lambda g: pc.GEOM_ID % g)
def test_gap_guards_and_repack(dev, geom):
    """Images packed into a buffer that holds the sentinel: the gap between the chunk table and the data area keeps it (the device
    packer leaves the gap to the caller), everything else is the host image.  Then the parameters change in place and
    pnr_mlp_repack_device runs into the same buffers: the data area is the host image of the new values; header, chunk table,
    gap and workspace keep their bytes.  Forward plans 0 .. 4, fp32 and the transposed image."""
    labels = []
    for label, desc, backward in pc.images(geom):
        params = pc.random_params(geom, seed=11)
        params_dev = _to(params, dev)
        host = pc.host_image(desc, params, backward)
        hdr = pc.header(host)
        a, b = hdr["gap"]
        assert b > a and not host[a:b].any()                          # there is a gap, and the host packer zeroes it
        run = Pack(dev, desc, params_dev, backward, fill=None)
        run.check_guards(hdr)
        got = run.img.cpu()
        assert bool((got[a:b] == BYTE_SENTINEL).all()), "%s: the gap was written" % label
        assert torch.equal(got[:a], host[:a]) and torch.equal(got[b:], host[b:]), label
        head, ws = run.img[:b].clone(), run.ws.clone()
        for step in (1, 2):
            new = _edit(params_dev, step)
            run.repack()
            run.check_guards(hdr)
            assert torch.equal(run.img[:b], head), "%s: a repack wrote in front of the data area" % label
            assert torch.equal(run.ws, ws), "%s: a repack wrote the workspace" % label
            want = pc.host_image(desc, new, backward)
            assert not torch.equal(want, host)
            assert torch.equal(run.img[b:].cpu(), want[b:]), "%s: repack %d" % (label, step)
        labels.append(label)
    print("repacked:", " ".join(labels))
    assert {"bf16/plan0/fwd", "bf16/plan3/fwd", "bf16/plan4/fwd", "bf16/plan0/bwd"} <= set(labels)
    assert geom[1] == 128 or {"bf16/plan1/fwd", "bf16/plan2/fwd"} <= set(labels)


SMALL = (3, 128, 1, 6, 4, "trunk", 2, 10, 4)


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
def test_repack_in_a_captured_graph_follows_the_parameters(dev, backward):
    """ops.pack_mlp_device(repack=True) captured with torch.cuda.graph: each replay packs the values the parameters hold then.
    The first, full pack copies descriptors from the host and synchronises, so it stays outside the capture."""
    params_dev = _to(pc.random_params(SMALL, seed=2), dev)
    desc = pc.make_desc(SMALL)
    img, ws = ops.pack_mlp_device(desc, params_dev, backward)
    assert torch.equal(img.cpu(), pc.host_image(desc, {k: v.cpu() for k, v in params_dev.items()}, backward))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        img2, ws2 = ops.pack_mlp_device(desc, params_dev, backward, img, ws, repack=True)
    assert img2.data_ptr() == img.data_ptr() and ws2.data_ptr() == ws.data_ptr()
    for step in (1, 2):
        new = _edit(params_dev, step)
        stale = img.cpu()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(img.cpu(), pc.host_image(desc, new, backward)) and not torch.equal(img.cpu(), stale)


def test_pack_and_read_on_a_side_stream(dev):
    params = pc.random_params(SMALL, seed=4)
    params_dev = _to(params, dev)
    desc = pc.make_desc(SMALL)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        img, ws = ops.pack_mlp_device(desc, params_dev, False)
        first = img.clone()
        new = _edit(params_dev, 1)
        ops.pack_mlp_device(desc, params_dev, False, img, ws, repack=True)
        second = img.clone()
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert torch.equal(first.cpu(), pc.host_image(desc, params)) and torch.equal(second.cpu(), pc.host_image(desc, new))


def test_repack_refuses_parameters_it_would_read_from_a_dead_copy(dev):
    """A parameter that is not float32 and contiguous is packed from a temporary copy, and the descriptors of that pack point at
    the copy: repack=True is a ValueError that names the parameter, raised before anything runs.  (The buffers handed in here
    come from a pack of live float32 tensors, so no version of the code reads freed memory in this test.)  A full pack of the
    same parameters is the host image of their float32 values."""
    live = _to(pc.random_params(SMALL, seed=6), dev)
    desc = pc.make_desc(SMALL)
    img, ws = ops.pack_mlp_device(desc, live, False)
    before = img.clone()
    doubles = {k: v.double() for k, v in live.items()}
    with pytest.raises(ValueError, match=r"'pts_linears\.0\.weight' \(torch\.float64\).*float32, contiguous"):
        ops.pack_mlp_device(desc, doubles, False, img, ws, repack=True)
    views = dict(live)
    views["feature_linear.weight"] = live["feature_linear.weight"].t()              # square: the same shape, other strides
    assert not views["feature_linear.weight"].is_contiguous()
    with pytest.raises(ValueError, match=r"'feature_linear\.weight' \(torch\.float32, not contiguous\).*float32, contiguous"):
        ops.pack_mlp_device(desc, views, False, img, ws, repack=True)
    torch.cuda.synchronize()
    assert torch.equal(img, before)
    for p in (doubles, views):
        full, _ = ops.pack_mlp_device(desc, p, False)
        assert torch.equal(full.cpu(), pc.host_image(desc, {k: v.float().cpu().contiguous() for k, v in p.items()}))


# ------------------------------------------------------------------------------------------------ Network._pack on the GPU
KEYS = [("classic", {}), ("fp32", dict(precision="fp32")), ("fused", dict(fused=True)), ("fused1", dict(fused=1)),
        ("softmax", dict(fused="softmax")), ("sigma", dict(fused="sigma")), ("field", dict(fused="field")), ("bwd", None)]
NETS = {   # the default 8 x 256 network (every plan exists) with two NeRFs, and a small shared one
    "two_nerfs": NS(N_samples=32, N_importance=32, num_classes=19, num_instances=8, precision="bf16"),
    "shared": NS(N_samples=32, N_importance=32, num_classes=6, num_instances=4, precision="bf16", D=3, W=128, skips=[1], share_coarse_fine=True),
}


@pytest.fixture(params=list(NETS))
def net(request, dev):
    torch.manual_seed(13)
    n = make_network(NETS[request.param]).to(dev)
    assert (n.nerf_1 is None) == (request.param == "shared")
    return n


@pytest.fixture
def calls(monkeypatch):
    """(repack, data_ptr of the image) of every ops.pack_mlp_device call that Network._pack makes"""
    seen, real = [], ops.pack_mlp_device

    def spy(desc, params, backward=False, out=None, workspace=None, repack=False):
        res = real(desc, params, backward, out, workspace, repack=repack)
        seen.append((bool(repack), res[0].data_ptr()))
        return res

    monkeypatch.setattr(ops, "pack_mlp_device", spy)
    return seen


def _first_per_image(calls):
    """image -> the repack flag of the FIRST of `calls` that packed it (two levels of a shared network, or two keys that reach
    the same plan, are one image: its second call in a round finds the pointers of the first)"""
    first = {}
    for repack, ptr in calls:
        first.setdefault(ptr, repack)
    return first


def _images(net, dev):
    """{(level, key): (desc, image, backward)} of every key at both levels"""
    out = {}
    for lv in (0, 1):
        for name, kw in KEYS:
            desc, img = net.packed_bwd(lv, dev) if kw is None else net.packed(lv, dev, **kw)
            out[lv, name] = (desc, img, kw is None)
    return out


def _host_images(net, images):
    sd = {lv: {k: v.detach().float().cpu() for k, v in net.nerf(lv).named_parameters()} for lv in (0, 1)}
    return {k: pc.host_image(desc, sd[k[0]], backward) for k, (desc, img, backward) in images.items()}


def _check(net, images, host=None):
    host = _host_images(net, images) if host is None else host
    for k, (desc, img, backward) in images.items():
        assert img.is_cuda and torch.equal(img.cpu(), host[k]), k
    return host


def _touched(nerf):
    return [nerf.pts_linears[1].weight, nerf.pts_linears[0].bias, nerf.alpha_linear.weight, nerf.alpha_linear.bias, nerf.feature_linear.bias,
            nerf.views_linears[0].weight, nerf.rgb_linear.bias, nerf.semantic_linears[0].weight, nerf.semantic_linears[1].bias,
            nerf.instance_linears[1].weight]


def _nerfs(net):
    return [net.nerf_0] + ([net.nerf_1] if net.nerf_1 is not None else [])


def _edit_net(net, step, data=False):
    """an in-place edit of weights and biases of trunk and heads: versioned (add_ under no_grad) or through .data"""
    with torch.no_grad():
        for nerf in _nerfs(net):
            for i, p in enumerate(_touched(nerf)):
                (p.data if data else p).add_(0.0625 * (i + 1) * step)


def _ptrs(images):
    return {k: v[1].data_ptr() for k, v in images.items()}


def test_network_plans_are_the_ones_meant(net, dev):
    """the keys reach the plans they name: sigma -> 3, field -> 4, and at the 8 x 256 network fused -> 2, fused=1 -> 1"""
    im = _images(net.eval(), dev)
    plans = {k[1]: int(v[0].plan) for k, v in im.items() if k[0] == 0}
    assert plans["classic"] == plans["fp32"] == plans["bwd"] == 0 and plans["sigma"] == 3 and plans["field"] == 4
    if net.nerf_1 is not None:
        assert plans["fused"] == 2 and plans["fused1"] == 1 and plans["softmax"] in (1, 2)
    _check(net, im)


def test_network_eval_cache_follows_versions(net, dev, calls):
    net.eval()
    first = _images(net, dev)
    _check(net, first)
    n_packs = len(calls)
    again = _images(net, dev)
    assert all(again[k][1] is first[k][1] for k in first) and len(calls) == n_packs            # served from the cache
    for step in (1, 2):
        _edit_net(net, step)
        im = _images(net, dev)
        assert _ptrs(im) == _ptrs(first)                                                      # captured pointers stay valid
        _check(net, im)
    assert n_packs == len(set(_ptrs(first).values())) and not any(r for r, _ in calls[:n_packs])      # one full pack per image
    assert len(calls) == 3 * n_packs and all(r for r, _ in calls[n_packs:])                     # in-place edits: the kernel alone


def test_network_eval_sees_data_writes_after_invalidate(net, dev):
    net.eval()
    first = _images(net, dev)
    old = _check(net, first)
    _edit_net(net, 1, data=True)
    stale = _images(net, dev)
    new = _host_images(net, stale)
    assert all(not torch.equal(new[k], old[k]) for k in old)
    _check(net, stale, old)                                  # tensor versions do not see a .data write: the documented contract
    net.invalidate_packed()
    im = _images(net, dev)
    _check(net, im, new)
    assert _ptrs(im) == _ptrs(first)


def test_network_train_repacks_on_every_call(net, dev, calls):
    net.train()
    first = _images(net, dev)
    _check(net, first)
    n_keys = len(calls)
    assert n_keys == 2 * len(KEYS)                           # every call packs, also a key that another call of the round packed
    assert set(_first_per_image(calls)) == set(_ptrs(first).values()) and not any(_first_per_image(calls).values())
    for step in (1, 2):
        _edit_net(net, step, data=(step == 1))               # a .data write, then a versioned one
        im = _images(net, dev)
        _check(net, im)
        assert _ptrs(im) == _ptrs(first)
    _images(net, dev)                                        # and with nothing changed
    assert len(calls) == 4 * n_keys and all(r for r, _ in calls[n_keys:])


def test_network_mode_switch_drops_the_images(net, dev):
    net.eval()
    first = _images(net, dev)
    old = _check(net, first)
    _edit_net(net, 1, data=True)
    _check(net, _images(net, dev), old)                      # eval: still the cached images
    net.train()
    _check(net, _images(net, dev))                           # the switch dropped them
    _edit_net(net, 2, data=True)
    net.eval()
    im = _images(net, dev)
    now = _check(net, im)                                    # and so did the switch back
    assert all(not torch.equal(now[k], old[k]) for k in old)


@pytest.mark.parametrize("how", ["data", "assign"])
def test_network_replaced_storage_takes_a_full_pack(net, dev, calls, how):
    """p.data = other / load_state_dict(assign=True) move parameters to other storage: the descriptors on the device point at the
    old one, so the next image must be a full pack.  The old tensors stay alive here, so a repack would read their (old) values
    and fail the comparison rather than touch freed memory."""
    net.train()
    first = _images(net, dev)
    _check(net, first)
    _images(net, dev)
    n = len(calls)
    assert all(r for r, _ in calls[n // 2:])                  # steady state: repacks
    old = [p.data for p in net.parameters()]                  # kept alive
    if how == "data":
        for nerf in _nerfs(net):
            for i, p in enumerate(_touched(nerf)):
                p.data = p.data * 1.5 + 0.03125 * (i + 1)
    else:
        net.load_state_dict({k: v.detach() * 1.5 + 0.03125 for k, v in net.state_dict().items()}, assign=True)
    assert {p.data_ptr() for p in net.parameters()} != {t.data_ptr() for t in old}
    im = _images(net, dev)
    took = _first_per_image(calls[n:])
    assert set(took) == set(_ptrs(first).values()) and not any(took.values())      # every image: a full pack, into its old buffer
    _check(net, im)
    assert _ptrs(im) == _ptrs(first)
    n = len(calls)
    _edit_net(net, 1)
    _check(net, _images(net, dev))
    assert len(calls) > n and all(r for r, _ in calls[n:])   # and back to the kernel alone
    assert all(torch.isfinite(t).all() for t in old)


def test_double_network_is_packed_in_full_every_time(net, dev, calls):
    """a network cast with .double(): the packer reads float32 copies that die with the call, so there is nothing a repack
    could read -- every image of every render is a full pack, and right"""
    net.double().train()
    assert all(p.dtype == torch.float64 for p in net.parameters())
    _check(net, _images(net, dev))
    for step in (1, 2):
        _edit_net(net, step)
        _check(net, _images(net, dev))
    assert len(calls) == 3 * 2 * len(KEYS) and not any(r for r, _ in calls)
    net.eval()
    _check(net, _images(net, dev))
    _edit_net(net, 3)
    _check(net, _images(net, dev))
    assert not any(r for r, _ in calls)


def test_images_after_one_adam_step(dev):
    """one real optimiser step (render with autograd, backward through the HIP kernels, Adam) on a small network: the images the
    next render packs -- whatever keys the renderer asks for -- and packed / packed_bwd are the host images of the stepped
    parameters"""
    cfg = NS(N_samples=32, N_importance=32, num_classes=6, num_instances=4, precision="bf16", D=3, W=128, skips=[1])
    torch.manual_seed(21)
    net = make_network(cfg).to(dev).train()
    rend = make_renderer(cfg, net)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    rays = synthetic.camera_rays()[::8009][:64].contiguous().to(dev)
    tgt = torch.rand((1, 64, 3), device=dev)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    for _ in range(2):                                                          # the second render packs the stepped parameters
        opt.zero_grad(set_to_none=True)
        out = rend.render({"rays": rays[None]})
        loss = ((out["rgb_0"] - tgt) ** 2).mean() + ((out["rgb_1"] - tgt) ** 2).mean() + (out["semantic_1"] ** 2).mean() + (out["instance_1"] ** 2).mean()
        loss.backward()
        held = dict(net._packed)
        sd = {lv: {k: v.detach().float().cpu() for k, v in net.nerf(lv).named_parameters()} for lv in (0, 1)}
        opt.step()
    moved = [k for k, v in net.named_parameters() if not torch.equal(v, before[k])]
    assert len(moved) > len(before) // 2, moved
    assert {k[0] for k in held} == {"fwd", "bwd"} and {k[1] for k in held} == {0, 1}
    for key, (ver, desc, img, ws, ptrs) in held.items():                        # what the second render read: the once-stepped values
        assert torch.equal(img.cpu(), pc.host_image(desc, sd[key[1]], key[0] == "bwd")), key
    sd = {lv: {k: v.detach().float().cpu() for k, v in net.nerf(lv).named_parameters()} for lv in (0, 1)}
    for lv in (0, 1):
        for backward in (False, True):
            desc, img = net.packed_bwd(lv, dev) if backward else net.packed(lv, dev)
            assert torch.equal(img.cpu(), pc.host_image(desc, sd[lv], backward)), (lv, backward)
