"""CPU checks of tests/_render_cases.py: the generated matrix covers every admissible pair of factor values (by enumeration) and
every dispatch route with every value it can meet, is deterministic and inside the constraints; the expected key sets and routes
are right on hand-written examples."""
import itertools

import pytest

import _render_cases as rc

CASES = rc.generate()


def _case(**kw):
    assert set(kw) <= set(rc.FACTORS)
    return {f: kw.get(f, v[0]) for f, v in rc.FACTORS.items()}


def test_every_admissible_pair_is_covered():
    names = list(rc.FACTORS)
    want = set()
    for fa, fb in itertools.combinations(names, 2):             # enumerated here, not taken from the generator
        for va, vb in itertools.product(rc.FACTORS[fa], rc.FACTORS[fb]):
            if not ({(fa, va), (fb, vb)} == {("coarse_outputs", "weights"), ("samples", (64, 0))}):
                want.add(((fa, va), (fb, vb)))
    assert want == set(rc.admissible_pairs())
    got = set()
    for c in CASES:
        got |= {((fa, c[fa]), (fb, c[fb])) for fa, fb in itertools.combinations(names, 2)}
    assert want <= got, sorted(want - got)[:5]
    print("render matrix: %d cases cover %d pairs of %d factors" % (len(CASES), len(want), len(names)))
    assert len(CASES) <= 48                     # each is two small renders on the GPU


def test_every_route_meets_every_value_it_can():
    n = 0
    for target, templates in rc.ROUTE_TEMPLATES:
        assert any(rc.route_has(c, target) for c in CASES), target
        for tmpl in templates:
            for f, v in rc.route_pairs(target, tmpl):
                assert any(rc.route_has(c, target) and c[f] == v for c in CASES), (target, f, v)
                n += 1
    assert n > 100
    # the level kernels in every order a render can have them, and both resamplers / every preamble
    seen = {rc.route(c).levels for c in CASES}
    assert {("fused", "fused"), ("sigma", "fused"), ("sigma", "two_kernel"), ("fused", "two_kernel"), ("two_kernel", "two_kernel"),
            ("train", "train"), ("fused",), ("two_kernel",), ("train",)} <= seen
    assert {rc.route(c).preamble for c in CASES} == {"ray_setup", "bbox_hits", "convex_hits", "stratified"}
    assert {rc.route(c).resampler for c in CASES} == {None, "sample_pdf", "sample_pdf_labels"}
    assert sum(rc.route(c).two_streams for c in CASES) >= 3


def test_generator_is_deterministic():
    assert rc.generate() == CASES == rc.generate()
    ids = [rc.case_id(i, c) for i, c in enumerate(CASES)]
    assert len(set(ids)) == len(ids)


def test_every_factor_value_appears():
    for f, values in rc.FACTORS.items():
        assert {c[f] for c in CASES} == set(values), f


def test_no_case_violates_a_constraint():
    for c in CASES:
        assert list(c) == list(rc.FACTORS) and all(c[f] in rc.FACTORS[f] for f in c)
        assert rc.refused(c) is None
        assert not (c["coarse_outputs"] == "weights" and c["samples"][1] == 0)
    assert rc.refused(_case(coarse_outputs="weights", samples=(64, 0)))[2] == "needs a fine level"


def test_named_cases_exist():
    for name, want in list(rc.ANCHORS.items()) + list(rc.TEETH.items()):
        assert rc.find(CASES, **want) is not None, name


def test_restated_constants():
    ops = pytest.importorskip("panopticnerf_amd.ops")
    from panopticnerf_amd import renderer
    assert ops.RAY_SETUP_MAX_HITS == rc.RAY_SETUP_MAX_HITS
    assert renderer.chunk_plan(rc.R_RAYS, rc.CHUNK_SIZE) == [(0, 86), (86, 172), (172, 257)]
    assert renderer.chunk_plan(rc.R_RAYS, 65536) == [(0, 257)]


# --------------------------------------------------------------------------------------------------------------- key sets, by hand
def _keys(*names):
    return frozenset(names)


def test_keys_without_a_prior():
    assert rc.expected_keys(_case()) == _keys(
        "z_vals_0", "rgb_0", "depth_0", "acc_0", "weights_0", "semantic_0", "instance_0",
        "z_vals_1", "rgb_1", "depth_1", "acc_1", "weights_1", "semantic_1", "instance_1")
    assert rc.expected_keys(_case(heads=(0, 0), prior="box8")) == _keys(
        "z_vals_0", "rgb_0", "depth_0", "acc_0", "weights_0", "z_vals_1", "rgb_1", "depth_1", "acc_1", "weights_1")


def test_keys_with_a_prior():
    for prior in ("box8", "box33", "prim8"):
        assert rc.expected_keys(_case(prior=prior, heads=(19, 0))) == _keys(
            "z_vals_0", "rgb_0", "depth_0", "acc_0", "weights_0", "semantic_0", "fix_semantic_0",
            "z_vals_1", "rgb_1", "depth_1", "acc_1", "weights_1", "semantic_1", "fix_semantic_1")


def test_keys_without_kept_weights():
    # the fine level samples the coarse weights: weights_0 stays; without a fine level it goes too
    assert rc.expected_keys(_case(keep_weights=False, heads=(0, 0))) == _keys(
        "z_vals_0", "rgb_0", "depth_0", "acc_0", "weights_0", "z_vals_1", "rgb_1", "depth_1", "acc_1")
    assert rc.expected_keys(_case(keep_weights=False, heads=(0, 0), samples=(64, 0))) == _keys("z_vals_0", "rgb_0", "depth_0", "acc_0")
    # under autograd level_train returns the weights whatever the switch says
    assert "weights_1" in rc.expected_keys(_case(keep_weights=False, mode="train_grad"))
    assert "weights_1" not in rc.expected_keys(_case(keep_weights=False, mode="train_nograd"))


def test_keys_in_weights_mode():
    assert rc.expected_keys(_case(coarse_outputs="weights", prior="box8")) == _keys(
        "z_vals_0", "depth_0", "acc_0", "weights_0", "fix_semantic_0", "fix_instance_0",
        "z_vals_1", "rgb_1", "depth_1", "acc_1", "weights_1", "semantic_1", "instance_1", "fix_semantic_1", "fix_instance_1")
    # ... which autograd ignores; and the training maps carry the 3D cross-entropies of the labelled samples
    k = rc.expected_keys(_case(coarse_outputs="weights", prior="box8", mode="train_grad", heads=(19, 0)))
    assert k == _keys("z_vals_0", "rgb_0", "depth_0", "acc_0", "weights_0", "semantic_0", "fix_semantic_0", "ce3d_semantic_0",
                      "ce3d_semantic_n_0", "z_vals_1", "rgb_1", "depth_1", "acc_1", "weights_1", "semantic_1", "fix_semantic_1",
                      "ce3d_semantic_1", "ce3d_semantic_n_1")
    assert not any(x.startswith("ce3d") for x in rc.expected_keys(_case(mode="train_grad")))       # no prior: no labels


def test_keys_without_a_fine_level():
    assert rc.expected_keys(_case(samples=(64, 0), prior="prim8", heads=(19, 0), share_coarse_fine=True)) == _keys(
        "z_vals_0", "rgb_0", "depth_0", "acc_0", "weights_0", "semantic_0", "fix_semantic_0")


# --------------------------------------------------------------------------------------------------------------- routes, by hand
def test_preambles():
    assert rc.route(_case()).preamble == "stratified"
    assert rc.route(_case(prior="box8")).preamble == "ray_setup"
    assert rc.route(_case(prior="box33")).preamble == "bbox_hits"
    assert rc.route(_case(prior="prim8")).preamble == "convex_hits"
    calls, _ = rc.expected_calls(_case(prior="box8", chunks="three_cat"), 256)
    assert (calls["ray_setup"], calls["stratified"], calls["bbox_hits"], calls["convex_hits"]) == (3, 0, 0, 0)
    calls, _ = rc.expected_calls(_case(prior="box33", bbox_sampling="hull"), 256)
    assert (calls["ray_setup"], calls["stratified"], calls["bbox_hits"], calls["convex_hits"]) == (0, 1, 1, 0)
    calls, _ = rc.expected_calls(_case(prior="prim8"), 256)
    assert (calls["ray_setup"], calls["stratified"], calls["bbox_hits"], calls["convex_hits"]) == (0, 1, 0, 1)
    calls, _ = rc.expected_calls(_case(), 256)
    assert (calls["ray_setup"], calls["stratified"], calls["bbox_hits"], calls["convex_hits"]) == (0, 1, 0, 0)


def test_level_kernels():
    lv = lambda **kw: rc.route(_case(**kw)).levels          # noqa: E731
    assert lv() == ("fused", "fused")
    assert lv(semantic_activation="softmax", head_tap="feature") == ("fused", "fused")
    assert lv(samples=(32, 32)) == ("fused", "fused") and lv(samples=(64, 0)) == ("fused",)
    assert lv(samples=(64, 100)) == ("fused", "two_kernel")                         # 164 is no multiple of 32
    assert lv(coarse_outputs="weights") == ("sigma", "fused")
    assert lv(coarse_outputs="weights", samples=(64, 100)) == ("sigma", "two_kernel")
    assert lv(precision="fp32") == ("two_kernel", "two_kernel") == lv(fuse_composite=False)
    assert lv(coarse_outputs="weights", precision="fp32") == ("two_kernel", "two_kernel") == lv(coarse_outputs="weights", fuse_composite=False)
    assert lv(mode="train_nograd") == ("two_kernel", "two_kernel")                  # sigma noise
    assert lv(mode="train_nograd", coarse_outputs="weights") == ("two_kernel", "two_kernel")
    assert lv(mode="eval_explicit") == ("fused", "fused")                           # explicit uniforms are no noise
    assert lv(mode="train_grad") == ("train", "train") == lv(mode="train_grad", precision="fp32", coarse_outputs="weights")
    calls, wg = rc.expected_calls(_case(coarse_outputs="weights", chunks="three"), 256)
    assert (calls["mlp_forward_weights"], calls["mlp_forward_composite"], calls["mlp_forward"], calls["level_train"]) == (3, 3, 0, 0)
    assert wg == [0, 0, 0] and calls["_render_overlapped"] == 0
    calls, wg = rc.expected_calls(_case(mode="train_grad", chunks="three"), 256)
    assert (calls["mlp_forward_weights"], calls["mlp_forward_composite"], calls["mlp_forward"], calls["level_train"]) == (0, 0, 0, 6)


def test_resamplers_and_draws():
    assert rc.route(_case()).resampler == "sample_pdf"
    assert rc.route(_case(prior="prim8")).resampler == "sample_pdf_labels" == rc.route(_case(prior="box33")).resampler
    assert rc.route(_case(samples=(64, 0), prior="box8")).resampler is None
    assert [rc.route(_case(mode=m)).draws for m in rc.FACTORS["mode"]] == [False, True, True, False]
    assert [rc.route(_case(mode=m)).grad for m in rc.FACTORS["mode"]] == [False, False, True, False]


def test_frames():
    over = lambda cus=256, **kw: rc.overlap_caps(_case(**kw), cus)          # noqa: E731
    assert over(chunks="three") == (64, 192)                                 # 256 compute units, 64 : 192 samples
    assert over(chunks="three", samples=(32, 32)) == (88, 168)               # 32 : 64 -> 85.3 -> 88 + 168: 4.5 % off the ratio
    assert over(chunks="three", prior="box33", semantic_activation="softmax", keep_weights=False, share_coarse_fine=True) == (64, 192)
    for off in (dict(chunks="one"), dict(chunks="three_cat"), dict(overlap_levels=False), dict(mode="eval_explicit"),
                dict(mode="train_nograd"), dict(mode="train_grad"), dict(coarse_outputs="weights"), dict(fuse_composite=False),
                dict(precision="fp32"), dict(samples=(64, 100)), dict(samples=(64, 0))):
        assert over(**dict(dict(chunks="three"), **off)) is None, off
    assert over(304, chunks="three") is None                                 # 80 + 224: more than 5 % off
    assert over(252, chunks="three") is None                                 # no multiple of 8
    assert over(64, chunks="three") == (16, 48)
    calls, wg = rc.expected_calls(_case(chunks="three"), 256)
    assert calls["_render_overlapped"] == 1 and wg == [0, 192, 64, 192, 64, 0]
    calls, wg = rc.expected_calls(_case(chunks="three"), 304)
    assert calls["_render_overlapped"] == 0 and wg == [0] * 6
