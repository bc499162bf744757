"""The switches Renderer.render / render_rays read, as a table of factors; a deterministic greedy generator of a PAIRWISE covering
set of renders under the constructor's refusals; and, per case, the route the documented dispatch rules say the render takes.
CPU only: nothing here imports torch or the package, and nothing here asks the code under test (ops.fused_supported,
ops.sigma_pass_supported, Renderer._overlap_caps) which way it would go -- the rules are restated from their documentation:

  preamble   (Renderer._preamble; ops.ray_setup: "max_hits <= 8")   boxes with max_hits <= RAY_SETUP_MAX_HITS = 8: ray_setup alone;
             more hits: bbox_hits + restrict_rays (hull) + stratified + sample_labels; convex primitives: convex_hits + the same
             separate kernels ("no fused twin"); no prior: stratified alone.
  level      (Renderer.__init__ on fuse_composite / coarse_outputs, ops.fused_supported, ops.sigma_pass_supported, COVERAGE a5 / a6 / a9)
             under autograd train.level_train, whatever else is set ("Under autograd the switch has no effect");
             else the fused pass where: bf16, cfg.fuse_composite, no sigma noise, N a multiple of 32 in [32, 256], C + K <= 128 --
             softmax compositing included for every geometry of this table (heads of depth 2 on the 8 x 256 network: plan 2 has
             a softmax kernel) --; the coarse level of cfg.coarse_outputs = "weights" takes the sigma-only plan 3 under the same
             conditions; every other level is mlp_forward + composite (in "weights" mode with rgb / semantic / instance dropped).
             The image of a fused level of this table is plan 2 (include/pnr.h, pnr_mlp_fused_plan: D = 8, W = 256, skip = 4,
             L = 10 / 4; no heads, <= 64 classes, <= 64 classes + <= 32 instances; any head_tap).
  sigma noise is drawn in train mode (net.training) with cfg.raw_noise_std > 0, with or without autograd.
  resampler  (Renderer._resample) with a prior sample_pdf_labels, without one sample_pdf; none without a fine level.
  frame      (Renderer._overlap_caps) two streams only for: cfg.overlap_levels, eval mode, no autograd, >= 2 chunks,
             cfg.fuse_composite, cfg.frame_outputs, a fine level, no explicit t_rand / u, coarse_outputs = "all", both levels on
             the fused plan 2, and a compute-unit count that is a multiple of 8 and splits into two multiples of 8 in the ratio of
             the levels' samples within 5 %: cap_c = round(cus * Nc / (Nc + Nt) / 8) * 8, cap_f = cus - cap_c.

Switches that have NO effect in part of the space (the key sets and routes below say so, and the matrix renders them):
  keep_weights and coarse_outputs under autograd (level_train returns every map, weights included); bbox_sampling = "hull" without a
  prior; frame_outputs for one chunk and under autograd (chunks are concatenated); overlap_levels wherever the list above fails --
  in particular for max_hits > 8 and for primitives it still APPLIES (the preamble is not part of the rule); share_coarse_fine
  without a fine level; perturb and raw_noise_std in eval mode (nothing is drawn, rng_state stays)."""
import collections
import itertools

R_RAYS = 257                # three ragged chunks at chunk_size 100 (86 + 86 + 85: renderer.chunk_plan balances them)
CHUNK_SIZE = 100
RAY_SETUP_MAX_HITS = 8      # ops.RAY_SETUP_MAX_HITS, restated (test_render_cases.py compares)

# name -> values; the first value is the default of the code under test
FACTORS = collections.OrderedDict([
    ("precision", ("bf16", "fp32")),
    ("heads", ((45, 32), (19, 0), (0, 0))),
    ("head_tap", ("trunk", "feature")),
    ("prior", ("none", "box8", "box33", "prim8")),      # boxes with max_hits = 8 / 33; ConvexSet.from_boxes(...).batch() with 8
    ("bbox_sampling", ("none", "hull")),
    ("semantic_activation", ("none", "softmax")),
    ("coarse_outputs", ("all", "weights")),
    ("fuse_composite", (True, False)),
    ("samples", ((64, 128), (32, 32), (64, 100), (64, 0))),      # (64, 100): the fine level (164) falls off the fused pass
    ("chunks", ("one", "three", "three_cat")),          # three_cat: the three chunks with frame_outputs = False
    ("overlap_levels", (True, False)),
    ("white_bkgd", (False, True)),
    ("lindisp", (False, True)),
    ("keep_weights", (True, False)),
    ("share_coarse_fine", (False, True)),
    # eval inference | train mode under no_grad, device draws | train mode under autograd, device draws | eval with t_rand / u in the batch
    ("mode", ("eval", "train_nograd", "train_grad", "eval_explicit")),
])

# combinations Renderer.__init__ refuses BY NAME: ((factor, value), (factor, value), a fragment of the message).  Not cases of the matrix.
REFUSED = (
    (("coarse_outputs", "weights"), ("samples", (64, 0)), "needs a fine level"),
)

# cases every matrix starts from (they count towards the pairs): the default frame on two streams, and the softmax frame behind
# primitives with hull sampling on two streams -- eight values have to meet for _render_overlapped to run, no pair forces that
SEEDS = (
    dict(chunks="three"),
    dict(chunks="three", samples=(32, 32), prior="prim8", bbox_sampling="hull", semantic_activation="softmax", white_bkgd=True,
         keep_weights=False, heads=(19, 0), head_tap="feature"),
    dict(chunks="three", prior="box33", lindisp=True, share_coarse_fine=True, heads=(0, 0)),
)


def refused(case):
    """the REFUSED row a (partial) case falls under, or None"""
    for a, b, msg in REFUSED:
        if case.get(a[0], None) == a[1] and case.get(b[0], None) == b[1]:
            return a, b, msg
    return None


def _pair_ok(fa, va, fb, vb):
    return refused({fa: va, fb: vb}) is None


def admissible_pairs():
    """every ((factor, value), (factor, value)) of two different factors that some admissible case holds, in table order"""
    names = list(FACTORS)
    out = []
    for i, fa in enumerate(names):
        for fb in names[i + 1:]:
            for va in FACTORS[fa]:
                for vb in FACTORS[fb]:
                    if _pair_ok(fa, va, fb, vb):
                        out.append(((fa, va), (fb, vb)))
    return out


def pairs_of(case):
    names = list(FACTORS)
    return {((fa, case[fa]), (fb, case[fb])) for i, fa in enumerate(names) for fb in names[i + 1:]}


def case_id(i, case):
    c = case
    return "m%02d-%s-%s%s-%s-%dx%d-%s-%s" % (i, c["precision"], "%d+%d" % c["heads"], "f" if c["head_tap"] == "feature" else "",
                                          c["prior"], c["samples"][0], c["samples"][1], c["chunks"], c["mode"])


def generate():
    """[case]: SEEDS completed with defaults, then greedy: the next case starts from the first uncovered pair (table order) and
    gives every other factor, in table order, the value that covers most uncovered pairs with what is already set (ties: the
    value used least so far, then table order).  REFUSED is pairwise, so a partial case that holds no refused pair can always be
    completed.  A second pass (below) covers the dispatch.  Deterministic: no randomness, no hashing order."""
    names = list(FACTORS)
    todo = collections.OrderedDict((p, None) for p in admissible_pairs())
    used = collections.Counter()
    cases = []

    def commit(case):
        assert refused(case) is None, case
        cases.append(case)
        for p in pairs_of(case):
            todo.pop(p, None)
        for f in names:
            used[(f, case[f])] += 1

    for seed in SEEDS:
        commit({f: seed.get(f, FACTORS[f][0]) for f in names})
    while todo:
        (fa, va), (fb, vb) = next(iter(todo))
        case = {fa: va, fb: vb}
        for f in names:
            if f in case:
                continue
            best = None
            for v in FACTORS[f]:
                if any(not _pair_ok(f, v, g, w) for g, w in case.items()):
                    continue
                gain = 0
                for g, w in case.items():
                    p = ((f, v), (g, w)) if names.index(f) < names.index(g) else ((g, w), (f, v))
                    gain += p in todo
                key = (-gain, used[(f, v)], FACTORS[f].index(v))
                if best is None or key < best[0]:
                    best = (key, v)
            case[f] = best[1]
        commit({f: case[f] for f in names})
    # second pass, over the DISPATCH: pairs of inputs leave the routes that need many values to meet (the sigma pass, the two-stream
    # frame) to chance.  Every route value of ROUTE_TEMPLATES is rendered with every factor value it can be combined with -- "can":
    # setting that one value in one of the route's templates keeps the route
    for target, templates in ROUTE_TEMPLATES:
        for tmpl in templates:
            base = {f: tmpl.get(f, FACTORS[f][0]) for f in names}
            assert route_has(base, target), (target, tmpl)
            need = [(f, v) for f, v in route_pairs(target, tmpl) if not any(route_has(c, target) and c[f] == v for c in cases)]
            while need:
                case, spent = dict(base), set()
                for f, v in list(need):
                    if f in spent:
                        continue                    # this case already spends the factor on another needed value
                    trial = dict(case, **{f: v})
                    if refused(trial) is None and route_has(trial, target):
                        case = trial
                        spent.add(f)
                        need.remove((f, v))
                commit(case)
    return cases


# (route attribute, value) -> partial cases (defaults elsewhere) that take that route
ROUTE_TEMPLATES = (
    (("k0", "sigma"), (dict(coarse_outputs="weights"),)),
    (("k0", "fused"), (dict(),)),
    (("k0", "two_kernel"), (dict(precision="fp32"), dict(fuse_composite=False), dict(mode="train_nograd"))),
    (("k0", "train"), (dict(mode="train_grad"),)),
    (("k1", "fused"), (dict(),)),
    (("k1", "two_kernel"), (dict(precision="fp32"), dict(fuse_composite=False), dict(mode="train_nograd"), dict(samples=(64, 100)))),
    (("k1", "train"), (dict(mode="train_grad"),)),
    (("two_streams", True), (dict(chunks="three"),)),
)


def route_has(case, target):
    k, v = target
    r = route(case)
    if k == "k0":
        return r.levels[0] == v
    if k == "k1":
        return len(r.levels) > 1 and r.levels[1] == v
    return getattr(r, k) == v


def route_pairs(target, tmpl):
    """the (factor, value) pairs that keep `target` when set alone in the template"""
    base = {f: tmpl.get(f, FACTORS[f][0]) for f in FACTORS}
    out = []
    for f, values in FACTORS.items():
        for v in values:
            trial = dict(base, **{f: v})
            if refused(trial) is None and route_has(trial, target):
                out.append((f, v))
    return out


# ------------------------------------------------------------------------------------------------------------ the expected route
Route = collections.namedtuple("Route", "grad train draws n_chunks preamble levels resampler two_streams keys")


def n_levels(case):
    return 2 if case["samples"][1] > 0 else 1


def level_samples(case):
    Nc, Nf = case["samples"]
    return (Nc, Nc + Nf)[:n_levels(case)]


def _fused_ok(case, N, noise):
    C, K = case["heads"]
    return case["precision"] == "bf16" and case["fuse_composite"] and not noise and N % 32 == 0 and 32 <= N <= 256 and C + K <= 128


def level_kernel(case, lv):
    """'train' | 'sigma' | 'fused' | 'two_kernel' of level lv"""
    grad = case["mode"] == "train_grad"
    noise = case["mode"] in ("train_nograd", "train_grad")          # raw_noise_std = 1 in train mode
    if grad:
        return "train"
    ok = _fused_ok(case, level_samples(case)[lv], noise)
    if lv == 0 and case["coarse_outputs"] == "weights":
        return "sigma" if ok else "two_kernel"
    return "fused" if ok else "two_kernel"


def expected_keys(case):
    """the exact key set of the render's dict"""
    C, K = case["heads"]
    grad = case["mode"] == "train_grad"
    prior = case["prior"] != "none"
    fine = case["samples"][1] > 0
    keys = set()
    for lv in range(n_levels(case)):
        drop = lv == 0 and case["coarse_outputs"] == "weights" and not grad
        names = ["z_vals", "depth", "acc"]
        if not drop:
            names.append("rgb")
        if grad or case["keep_weights"] or (lv == 0 and fine):          # (the fine level samples the coarse weights)
            names.append("weights")
        for n, field in ((C, "semantic"), (K, "instance")):
            if n and not drop:
                names.append(field)
            if n and prior:
                names.append("fix_" + field)
                if grad:
                    names += ["ce3d_" + field, "ce3d_" + field + "_n"]
        keys |= {"%s_%d" % (n, lv) for n in names}
    return frozenset(keys)


def overlap_caps(case, cus):
    """(coarse, fine) workgroup caps of the two-stream frame on a device of `cus` compute units, or None: serial"""
    if not (case["overlap_levels"] and case["mode"] == "eval" and case["chunks"] == "three" and case["fuse_composite"]
            and case["samples"][1] > 0 and case["coarse_outputs"] == "all"):
        return None
    if any(level_kernel(case, lv) != "fused" for lv in (0, 1)):
        return None
    Nc, Nt = level_samples(case)
    cap_c = int(round(cus * Nc / float(Nc + Nt) / 8.0)) * 8
    cap_f = cus - cap_c
    if cus % 8 or cap_c < 8 or cap_f < 8 or abs((Nc / float(cap_c)) / (Nt / float(cap_f)) - 1.0) > 0.05:
        return None
    return cap_c, cap_f


def route(case):
    mode = case["mode"]
    train = mode in ("train_nograd", "train_grad")
    prior = case["prior"]
    return Route(grad=mode == "train_grad", train=train, draws=train, n_chunks=1 if case["chunks"] == "one" else 3,
                 preamble={"none": "stratified", "box8": "ray_setup", "box33": "bbox_hits", "prim8": "convex_hits"}[prior],
                 levels=tuple(level_kernel(case, lv) for lv in range(n_levels(case))),
                 resampler=None if case["samples"][1] == 0 else ("sample_pdf" if prior == "none" else "sample_pdf_labels"),
                 two_streams=overlap_caps(case, 256) is not None,       # on the MI355X's 256 compute units; overlap_caps for others
                 keys=expected_keys(case))


RECORDED = ("ray_setup", "bbox_hits", "convex_hits", "stratified", "mlp_forward_weights", "mlp_forward_composite", "mlp_forward",
            "sample_pdf_labels", "sample_pdf", "level_train", "_render_overlapped")


def expected_calls(case, cus):
    """({entry point: number of calls in one render}, [wg_cap of every mlp_forward_composite call in issue order]) on a device of
    `cus` compute units.  Every fused call of this table is on a plan-2 image."""
    r = route(case)
    n = r.n_chunks
    calls = dict.fromkeys(RECORDED, 0)
    calls[r.preamble] = n
    if r.preamble != "ray_setup":
        calls["stratified"] = n
    for k in r.levels:
        calls[{"sigma": "mlp_forward_weights", "fused": "mlp_forward_composite", "two_kernel": "mlp_forward", "train": "level_train"}[k]] += n
    if r.resampler:
        calls[r.resampler] = n
    caps = overlap_caps(case, cus)
    wg = [0] * calls["mlp_forward_composite"]
    if caps is not None:
        calls["_render_overlapped"] = 1
        # per chunk coarse then fine; the first coarse and the last fine launch have the device to themselves
        wg = list(itertools.chain.from_iterable((caps[0], caps[1]) for _ in range(n)))
        wg[0] = wg[-1] = 0
    return calls, wg


# ------------------------------------------------------------------------------------------------------------ named cases
def find(cases, **want):
    """index of the first case whose route / factors match: factor=value, k0= / k1= (level kernels), a Route field, prior_in=(...)"""
    for i, c in enumerate(cases):
        r = route(c)
        ok = True
        for k, v in want.items():
            if k == "k0":
                got = r.levels[0]
            elif k == "k1":
                got = r.levels[1] if len(r.levels) > 1 else None
            elif k in ("two_streams", "n_chunks", "preamble", "grad"):
                got = getattr(r, k)
            elif k == "prior_in":
                got, v = c["prior"] in v, True
            else:
                got = c[k]
            ok = ok and got == v
        if ok:
            return i
    return None


# one case per distinct level kernel, for the independent anchor (boxes or no prior: the oracle labels samples from box hit lists)
ANCHORS = collections.OrderedDict([
    ("fused_plan2_logits", dict(k1="fused", semantic_activation="none", heads=(45, 32), prior_in=("none", "box8", "box33"))),
    ("fused_softmax", dict(k1="fused", semantic_activation="softmax", prior_in=("none", "box8", "box33"))),
    ("sigma_only", dict(k0="sigma", prior_in=("none", "box8", "box33"))),
    ("two_kernel_bf16", dict(k0="two_kernel", k1="two_kernel", precision="bf16", prior_in=("none", "box8", "box33"))),
    ("two_kernel_fp32", dict(k0="two_kernel", k1="two_kernel", precision="fp32", prior_in=("none", "box8", "box33"))),
    ("train_bf16", dict(k0="train", k1="train", precision="bf16", prior_in=("none", "box8", "box33"))),
    ("train_fp32", dict(k0="train", k1="train", precision="fp32", prior_in=("none", "box8", "box33"))),
])

# the case each mis-wired renderer has to fail on
TEETH = collections.OrderedDict([
    ("ray_base_0", dict(mode="train_nograd", n_chunks=3)),                       # every chunk draws with ray base 0
    ("hull_ignored_for_primitives", dict(prior="prim8", bbox_sampling="hull")),
    ("white_bkgd_not_passed", dict(white_bkgd=True, k1="fused")),
    ("rows_one_chunk_late", dict(chunks="three", two_streams=False, grad=False)),         # a serial frame written in place
])
