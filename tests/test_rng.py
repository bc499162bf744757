"""CPU tests of the in-kernel RNG (include/pnr.h "in-kernel RNG"): the test-side Philox reference reproduces Random123's
known-answer vectors, every _rng entry point refuses a bad descriptor with PNR_EINVAL + a message before touching the device, and
the Renderer's cfg.rng switch is validated and leaves the default path alone.  No GPU."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _philox
from panopticnerf_amd import _lib


@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_reference_philox_known_answers(ctr, key, want):
    got = _philox.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert " ".join("%08x" % v for v in got) == want


def test_reference_stream_layout():
    """word j & 3 of the block with counter (j >> 2 | tag << 24, ray, lo(offset), hi(offset)) under key (lo(seed), hi(seed))"""
    seed, off, tag, base = 0x0123456789ABCDEF, (5 << 32) + 7, 4, 2**32 - 3
    w = _philox.stream_words(seed, off, tag, base, 3, 9)
    for r in range(3):
        for j in range(9):
            ctr = np.array([(j >> 2) | (tag << 24), (base + r) & 0xFFFFFFFF, 7, 5], dtype=np.uint64)
            blk = _philox.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
            assert w[r, j] == blk[j & 3]
    u = _philox.uniforms(w)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()


def _rng(call=16, tag=1, ray_base=0, scale=1.0):
    return _lib.RngDesc(call, ray_base, tag, scale)


BAD = [
    (None, b"null rng"),
    (_rng(call=0), b"null rng"),
    (_rng(tag=0), b"tag 0"),
    (_rng(tag=256), b"tag 256"),
    (_rng(scale=-1.0), b"scale"),
    (_rng(scale=float("nan")), b"scale"),
    (_rng(ray_base=-1), b"ray_base"),
    (_rng(ray_base=2**32 - 3), b"2^32"),           # + 4 rays > 2^32
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_rng_entry_points_reject_bad_descriptors_before_any_launch(i):
    lib = _lib.load()
    d, msg = BAD[i]
    ref = None if d is None else ctypes.byref(d)
    one = ctypes.c_void_p(16)         # non-null, never dereferenced: validation fails first
    null = ctypes.c_void_p(0)
    calls = {
        "pnr_rng_fill": lambda: lib.pnr_rng_fill(ref, 4, 8, 0, one, null),
        "pnr_stratified_rng": lambda: lib.pnr_stratified_rng(one, 4, 8, 0, ref, one, null),
        "pnr_ray_setup_rng": lambda: lib.pnr_ray_setup_rng(one, 4, one, 2, 8, null, 8, 0, ref, 0, one, one, one, one, null, null, null),
        "pnr_sample_pdf_rng": lambda: lib.pnr_sample_pdf_rng(one, one, ref, 4, 64, 128, null, null, one, null),
        "pnr_sample_pdf_labels_rng": lambda: lib.pnr_sample_pdf_labels_rng(one, one, ref, 4, 64, 128, one, one, one, one, 8, one, one, one, null),
        "pnr_composite_rng": lambda: lib.pnr_composite_rng(one, 1, 256, one, one, ref, null, null, 4, 64, 0, 0, 0, 0,
                                                          one, one, one, null, null, null, null, null, null),
        "pnr_composite_backward_rng": lambda: lib.pnr_composite_backward_rng(one, 256, one, one, ref, 4, 64, 0, 0, 0, *([null] * 12), one, null),
    }
    for name, fn in calls.items():
        assert fn() == -1, name
        err = lib.pnr_last_error()
        assert name.encode() in err and msg in err, (name, err)


def test_rng_begin_and_other_checks_without_a_device():
    lib = _lib.load()
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    assert lib.pnr_rng_begin(null, one, null) == -1 and b"pnr_rng_begin" in lib.pnr_last_error()
    assert lib.pnr_rng_begin(one, one, null) == -1 and b"aliased" in lib.pnr_last_error()
    assert lib.pnr_rng_begin(ctypes.c_void_p(12), ctypes.c_void_p(32), null) == -1 and b"aligned" in lib.pnr_last_error()
    ok = _rng()
    assert lib.pnr_rng_fill(ctypes.byref(ok), 4, 0, 0, one, null) == -1 and b"n_samples" in lib.pnr_last_error()
    # the composite twin takes channel-major images only
    assert lib.pnr_composite_rng(one, 64, 1, one, one, ctypes.byref(ok), null, null, 4, 64, 0, 0, 0, 0,
                                 one, one, one, null, null, null, null, null, null) == -1
    assert b"channel-major" in lib.pnr_last_error()
    # the whole 2^32 range of global rays is usable: ray_base + n_rays == 2^32 passes validation (zero rays: no launch)
    edge = _rng(ray_base=2**32)
    assert lib.pnr_stratified_rng(one, 0, 8, 0, ctypes.byref(edge), one, null) == 0
    assert lib.pnr_rng_fill(ctypes.byref(_rng(ray_base=2**32 - 4)), 5, 8, 0, one, null) == -1


def _tiny_net(**kw):
    from panopticnerf_amd import make_network
    cfg = NS(N_samples=8, N_importance=8, num_classes=3, num_instances=2, D=2, W=128, skips=[], **kw)
    torch.manual_seed(0)
    return make_network(cfg), cfg


def test_renderer_rng_switch():
    from panopticnerf_amd import make_renderer
    net, cfg = _tiny_net()
    rend = make_renderer(cfg, net)
    assert rend.rng == "torch" and rend.rng_state is None                  # the default touches no RNG state of its own
    with pytest.raises(ValueError, match="cfg.rng"):
        make_renderer(NS(**vars(cfg), rng="philox"), net)
    torch.manual_seed(1234)
    before = torch.get_rng_state()
    rend = make_renderer(NS(**vars(cfg), rng="device"), net)
    assert torch.equal(torch.get_rng_state(), before)                     # the default seed is read, nothing is drawn
    assert rend.rng_state.dtype == torch.int64 and rend.rng_state.tolist() == [1234, 0]
    rend = make_renderer(NS(**vars(cfg), rng="device", rng_seed=2**64 - 1), net)
    assert rend.rng_state.tolist() == [-1, 0]                              # the seed's 64 bits, as int64
    rend = make_renderer(NS(**vars(cfg), rng="device", rng_seed=7), net)
    assert rend.rng_state.tolist() == [7, 0]
