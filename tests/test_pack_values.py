"""What the HOST weight packer (pnr_mlp_pack, pnr_mlp_pack_bwd) does to parameter VALUES, against a restatement of the layout
header's rule in numpy integer arithmetic (tests/_pack_cases.py): bf16 weight fragments are pnr_f32_to_bf16 of the float32 bits
-- round to nearest even, NaN -> (u >> 16) | 0x40 -- and fp32 images and every bias fragment carry the bits verbatim.  The host
packer is the reference that test_gpu_pack_device.py holds the device packer to, byte for byte.  SURVEY.md 8a row a5.

The values: NaNs (quiet, signalling, negative, with payload), +-Inf, +-0, the smallest and the largest subnormal, FLT_MAX (rounds to
bf16 Inf), both kinds of tie and their neighbours -- planted in a trunk layer, the gamma(x) columns behind the skip, the last logit
block, alpha_linear and rgb_linear.  torch's own float32 -> bfloat16 conversion, which the oracles' bf16 emulation uses, is held to
the same restatement, and two corrupted restatements (truncation, round half up) must fail."""
import numpy as np
import pytest
import torch

import _pack_cases as pc

CASES = [(pc.PLANT_GEOM, "bf16", 0), (pc.PLANT_GEOM, "fp32", 0), (pc.PLANT_GEOM_BWD, "bf16", 1), (pc.PLANT_GEOM_BWD, "bf16", 0)]
_ID = lambda c: "%s_%s_%s" % (pc.GEOM_ID % c[0], c[1], "bwd" if c[2] else "fwd")      # noqa: E731


@pytest.fixture(scope="module", params=CASES, ids=_ID)
def case(request):
    geom, prec, backward = request.param
    desc = pc.make_desc(geom, prec)
    params, places = pc.planted_params(geom, seed=3)
    img = pc.host_image(desc, params, backward)
    hdr = pc.header(img)
    return dict(geom=geom, desc=desc, backward=backward, prec=prec, params=params, places=places, hdr=hdr,
                data=img[hdr["data_off"]:].numpy(), smap=pc.source_map(geom, desc, backward))


def test_restatement_on_known_values():
    """the restatement itself, on values whose bf16 is known by hand"""
    got = pc.f32_to_bf16(np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0x7F800001, 0xFF80FFFF, 0x7FC12345,
                                   0x00000001, 0x007FFFFF, 0x00400000, 0x80000000, 0xFF800000, 0x3F800000], np.uint32))
    assert got.tolist() == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x7F80, 0x7FC0, 0xFFC0, 0x7FC1, 0x0000, 0x0080, 0x0040, 0x8000, 0xFF80, 0x3F80]


def test_every_parameter_element_is_packed_once(case):
    """the word -> element table read off the packer: a forward image holds every element of every parameter exactly once; the
    transposed image holds no bias, no element twice, and every weight that carries a gradient back to a hidden activation"""
    base, total = pc._numbering(pc.shapes(case["geom"]))
    count = np.bincount(case["smap"], minlength=total + 1)[1:]
    if not case["backward"]:
        assert (count == 1).all(), "%d elements not packed exactly once" % int((count != 1).sum())
        return
    assert count.max() == 1
    ex = 3 + 6 * case["geom"][7]
    for k, (o, n) in base.items():
        c = count[o - 1:o - 1 + n]
        if k.endswith(".bias") or k == "pts_linears.0.weight":
            assert not c.any(), k
        elif k == "pts_linears.2.weight":                   # behind the skip: the h columns alone
            c = c.reshape(-1, case["geom"][1] + ex)
            assert not c[:, :ex].any() and c[:, ex:].all()
        elif k == "views_linears.0.weight":                 # the feature columns alone
            c = c.reshape(-1, case["geom"][1] + 3 + 6 * case["geom"][8])
            assert c[:, :case["geom"][1]].all() and not c[:, case["geom"][1]:].any()
        else:
            assert c.all(), k


def test_host_packer_rounds_as_the_layout_header_says(case):
    """the whole data area: verbatim bits in fp32 images and bias fragments, RNE with quieted NaNs in bf16 weight fragments"""
    want = pc.expected_data(case["geom"], case["desc"], case["params"], case["backward"], smap=case["smap"])
    assert np.array_equal(case["data"], want)


def test_planted_values_arrive(case):
    """each planted bit pattern, where the table says it went: found, and holding what the rule gives for it"""
    wide = case["prec"] == "fp32" and not case["backward"]
    words = case["data"].view(np.uint32 if wide else np.uint16)
    found, ex = 0, 3 + 6 * case["geom"][7]
    for name, index, bits in case["places"]:
        at = pc.word_of(case["smap"], case["geom"], name, index)
        if case["backward"] and (name.endswith(".bias") or (name == "pts_linears.2.weight" and index % (case["geom"][1] + ex) < ex)):
            assert at.size == 0                              # the transposed image holds neither
            continue
        assert at.size == 1, (name, index)
        found += 1
        if wide:
            assert int(words[at[0]]) == bits, (name, index, hex(bits))
        elif name.endswith(".bias"):
            assert (int(words[at[0]]) << 16 | int(words[at[0] - 1])) == bits, (name, index, hex(bits))
        else:
            assert int(words[at[0]]) == int(pc.f32_to_bf16(np.array([bits], np.uint32))[0]), (name, index, hex(bits))
    assert found >= 4 * len(pc.PLANTED)
    print("%d planted values found" % found)


@pytest.mark.parametrize("wrong", [pc.f32_to_bf16_truncating, pc.f32_to_bf16_half_up], ids=["truncation", "half_up"])
def test_a_corrupted_restatement_fails(case, wrong):
    """the comparison can tell the rule from its two usual corruptions (bf16 images; an fp32 image is rounded by neither)"""
    want = pc.expected_data(case["geom"], case["desc"], case["params"], case["backward"], to_bf16=wrong, smap=case["smap"])
    assert np.array_equal(case["data"], want) == (case["prec"] == "fp32" and not case["backward"])


def test_torch_bfloat16_agrees_with_the_restatement():
    """torch.Tensor.to(torch.bfloat16) -- the rounding inside the oracles' bf16 emulation -- is the same function on every planted
    value that is not a NaN and on 2^20 random bit patterns (NaNs among them compared as NaNs: torch need not keep a payload)"""
    rng = np.random.default_rng(5)
    u = np.concatenate([pc.PLANTED, rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    got = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    want = pc.f32_to_bf16(u)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    assert nan[:len(pc.NANS)].all() and not nan[len(pc.NANS):len(pc.PLANTED)].any()
    assert np.array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7FFF) > 0x7F80).all() and ((want[nan] & 0x7FFF) > 0x7F80).all()
