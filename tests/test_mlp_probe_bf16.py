"""CPU pins of the bf16 probe networks and their check (tests/_mlp_probe_bf16.py), with launch = torch_oracle.mlp_forward with bf16
emulation on c_oracle.points and the oracle's own view directions (NOT the inference kernels: this validates the probe weights and
the checker; tests/test_gpu_mlp_bf16_infer_sweep.py validates the kernels):
  * every probe returns its region bit for bit -- the bf16-rounded activation the oracle's next Linear reads, taken from `restated`,
    a local restatement of the oracle's forward that hands its intermediates out and whose raw equals the oracle's bit for bit -- at
    the 15 geometries of test_gpu_mlp_sweep.py plus two wide depth-1 heads (200 + 33 at 3 x 128, 256 + 1 at 8 x 256), S = 35;
  * every probe descriptor is one the ping-pong launcher takes;
  * the whole checker passes on the oracle at each of them with every fp32 ratio at most 1/4 (test_mlp32_ref.py's margin for its
    restatement: room for the MFMA's accumulation order on the device);
  * ten corrupted launchers fail, each by region name and only there (layer-local: the layers behind the wrong one read its wrong
    output and still pass)."""
import pytest
import torch
import torch.nn.functional as F

import _mlp_probe_bf16 as pb
import _mlp_ref as mr
from oracle import torch_oracle as to
from panopticnerf_amd import ops
from test_gpu_mlp_sweep import GEOMS

R, N = 5, 7                                      # S = 35: a full 32-sample tile and a second one of three samples
WIDE = [(3, 128, 1, 200, 33, "trunk", 1, 10, 4), (8, 256, 4, 256, 1, "trunk", 1, 10, 4)]
SKIP = (3, 128, 0, 5, 3, "trunk", 2, 10, 4)      # the skip layer right behind layer 0; two-layer heads


def inputs(rays, z):
    """the oracle's inputs: c_oracle.points, and run_network's own normalisation of the view directions"""
    pts, _ = pb.points_dirs(rays, z)
    d = rays[:, 3:6]
    vd = (d / torch.norm(d, dim=-1, keepdim=True))[:, None, :].expand(z.shape[0], z.shape[1], 3).reshape(-1, 3)
    return pts, vd


def restated(p, cfg, pts, vd, corrupt=None):
    """torch_oracle.mlp_forward(emulate_bf16=True) with its intermediates: (region -> the bf16-rounded activation the next Linear
    reads, raw).  corrupt: one of CORRUPT below."""
    q = to.bf16_round
    lin = lambda name, x, b=None: F.linear(x, q(p[name + ".weight"]), p[name + ".bias"] if b is None else b)     # noqa: E731
    ex = to.embed(pts, cfg.xyz_L)
    if corrupt == "band_swap" and cfg.xyz_L > 1:
        ex = torch.cat([ex[:, :9], ex[:, 12:15], ex[:, 9:12], ex[:, 15:]], 1)        # band 1 stored as cos | sin
    X = {"EX": q(ex), "ED": q(to.embed(vd, cfg.dir_L))}
    h, y = X["EX"], None
    for i in range(cfg.D):
        name = "pts_linears.%d" % i
        if corrupt == "unrounded" and i == 2:
            h = y                                                                    # the fp32 accumulator, never rounded to bf16
        if corrupt == "bias_block" and i == 1:
            b = p[name + ".bias"].clone()
            b[64:96] = p[name + ".bias"][32:64]                                      # block 2 takes block 1's bias fragment
            y = F.relu(lin(name, h, b))
        else:
            y = F.relu(lin(name, h))
        if corrupt == "truncated" and i == 1:
            y = (y.view(torch.int32) & -65536).view(torch.float32)                   # bf16 by truncation
        X["X%d" % (i + 1)] = h = q(y)
        if i in cfg.skips:
            if corrupt == "skip_no_gamma":
                h = torch.cat([torch.zeros_like(X["EX"]), h], -1)
            elif corrupt == "skip_order":
                h = torch.cat([h, X["EX"]], -1)
            else:
                h = torch.cat([X["EX"], h], -1)
    xd = X["X%d" % cfg.D]
    sigma = lin("alpha_linear", xd)
    X["F"] = q(lin("feature_linear", xd))
    X["G"] = q(F.relu(lin("views_linears.0", torch.cat([X["F"], X["ED"]], -1))))
    outs = [lin("rgb_linear", X["G"]), sigma]
    tap = X["F"] if cfg.head_tap == "feature" else xd
    for name, n, sh in (("semantic_linears", cfg.n_sem, "SH_sem"), ("instance_linears", cfg.n_inst, "SH_inst")):
        if not n:
            continue
        if cfg.head_depth == 2:
            y = lin(name + ".0", tap)
            X[sh] = q(y if (corrupt == "no_relu_sh" and sh == "SH_sem") else F.relu(y))
            outs.append(lin(name + ".1", X[sh]))
        else:
            y = lin(name + ".0", tap)
            if corrupt == "ktile" and sh == "SH_sem" and n >= 192:
                t = tap.clone()
                t[:, 16:32] = 0.0                                                    # one k-step of 16 dropped in logit block 5
                y[:, 160:192] = F.linear(t, q(p[name + ".0.weight"])[160:192], p[name + ".0.bias"][160:192])
            outs.append(y)
    raw = torch.cat(outs, -1)
    if corrupt == "head_row" and cfg.n_sem % 32 and cfg.n_sem > 66:
        raw[:, 4 + 65:4 + cfg.n_sem] = raw[:, 4 + 64:3 + cfg.n_sem].clone()          # behind row 64 every row lands one channel late
    if corrupt == "neighbour":
        raw[33] = raw[34]                                                            # sample 33 evaluated at sample 34's inputs
    return X, raw


def launcher(corrupt=None):
    def launch(desc, params, rays, z):
        cfg = pb.cfg_of(pb.geom_of(desc))
        pts, vd = inputs(rays, z)
        if corrupt is None:
            return to.mlp_forward(params, cfg, pts, vd, emulate_bf16=True)
        return restated(params, cfg, pts, vd, corrupt)[1]
    return launch


@pytest.mark.parametrize("geom", GEOMS + WIDE, ids=lambda g: pb.GEOM_ID % g)
def test_every_probe_returns_the_region_bit_for_bit(geom):
    c = pb.make_case(geom, R, N, seed=(GEOMS + WIDE).index(geom))
    desc, params, rays, z = c["desc"], c["params"], c["rays"], c["z"]
    pb.assert_normal(desc, params, rays, z)
    for pr in pb.probes(desc, params):
        pb.assert_pp_takes(ops.pack_mlp(pr.desc, pr.params), (pr.region, pb.geom_of(pr.desc)))
        assert all(bool(((v == 0) | (v.abs() == 1)).all()) for k, v in pr.params.items() if v is not params.get(k))
    launch = launcher()
    real = launch(desc, params, rays, z)
    want, raw = restated(params, pb.cfg_of(geom), *inputs(rays, z))
    assert torch.equal(raw, real)                                     # the restatement is the oracle
    X, rgbs = pb.read_out(launch, desc, params, rays, z, real=real)
    assert set(X) == set(want) and rgbs is not None
    for nm in want:
        assert X[nm].shape == want[nm].shape and torch.equal(X[nm], want[nm]), nm
    rep = mr.Report()
    pb.check_regions(rep, desc, params, rays, z, X, real)
    rep.check()
    assert max(v for k, v in rep.worst.items() if k.startswith("fp32")) <= 0.25 and max(rep.worst.values()) <= 1.0, rep.worst


def _check(c, launch):
    rep = mr.Report()
    pb.check(rep, launch, c["desc"], c["params"], c["rays"], c["z"])
    return rep


@pytest.mark.parametrize("geom", [SKIP] + WIDE, ids=lambda g: pb.GEOM_ID % g)
def test_checker_passes_on_the_oracle_with_a_margin_of_four(geom):
    rep = _check(pb.make_case(geom, R, N, seed=1), launcher())
    rep.check()
    fp32 = {k: v for k, v in rep.worst.items() if k.startswith("fp32")}
    assert fp32 and max(fp32.values()) <= 0.25, rep.worst
    assert all(v <= 1.0 for v in rep.worst.values()), rep.worst


@pytest.fixture(scope="module")
def cases():
    return {"skip": pb.make_case(SKIP, R, N, seed=0), "wide": pb.make_case(WIDE[0], R, N, seed=0)}


CORRUPT = {     # name -> (case, regions that must fail, regions that may)
    "ktile": ("wide", {"raw[semantic_linears.0]"}, {"raw[semantic_linears.0]"}),
    "head_row": ("wide", {"raw[semantic_linears.0]"}, {"raw[semantic_linears.0]"}),
    "bias_block": ("skip", {"X2"}, {"X2"}),
    "truncated": ("skip", {"X2"}, {"X2"}),
    "unrounded": ("skip", {"X3"}, {"X3"}),
    "skip_no_gamma": ("skip", {"X2"}, {"X2"}),
    "skip_order": ("skip", {"X2"}, {"X2"}),
    "band_swap": ("skip", {"EX"}, {"EX"}),
    # every launch returns sample 34's row for sample 33: its points are not sample 33's; both samples share a ray, so ED agrees
    "neighbour": ("skip", {"EX"}, {"EX"}),
    "no_relu_sh": ("skip", {"SH_sem"}, {"SH_sem"}),
}


@pytest.mark.parametrize("what", sorted(CORRUPT))
def test_corrupted_launcher_fails_by_name(cases, what):
    which, must, may = CORRUPT[what]
    rep = _check(cases[which], launcher(what))
    got = {f.split(":")[0] for f in rep.fails}
    assert must <= got <= may, rep.fails


def test_the_restatement_corrupts_nothing_by_default(cases):
    c = cases["wide"]
    args = (c["params"], pb.cfg_of(c["geom"])) + inputs(c["rays"], c["z"])
    clean = restated(*args)[1]
    for what in ("ktile", "head_row"):
        bad = restated(*args, corrupt=what)[1]
        cols = (bad != clean).any(0).nonzero().flatten().tolist()
        assert cols and (set(cols) <= set(range(4 + 160, 4 + 192)) if what == "ktile" else min(cols) >= 4 + 65 and max(cols) < 204), cols
