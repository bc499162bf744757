"""CPU tests of the k_mlp_tt generator (panopticnerf_amd/csrc/asm): the wait counters, the order in which captured side work
reaches them, atomic groups, the register table's checker, and one whole run of main().  None needs the library or a GPU."""
import importlib.util
import os
import re
import sys

import pytest

ASM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "panopticnerf_amd", "csrc", "asm")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ASM, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def G():
    return _load("gen_mlp_tt")      # puts its own directory on sys.path: the tt_ modules load through it


@pytest.fixture(scope="module")
def emit(G):
    return sys.modules["tt_emit"]


@pytest.fixture(scope="module")
def regs(G):
    return sys.modules["tt_regs"]


@pytest.mark.parametrize("cap", [15, 63])
def test_sim_counts_certain_operations_behind_the_tag(emit, cap):
    s = emit.Sim("x", cap)
    old = s.push()
    tag = s.push()
    s.push()
    s.push(certain=False)           # some waves skip it: it may not be outstanding, so it cannot be waited past
    s.push()
    assert s.wait_count(tag) == 2
    assert s.wait_count(tag) is None and s.wait_count(old) is None      # covered by the wait above
    assert s.wait_count(None) is None
    tag = s.push()
    for _ in range(cap + 5):
        s.push()
    assert s.wait_count(tag) == cap                                     # what the instruction's field can hold
    tag = s.push()
    s.push()
    s.drain()
    assert s.wait_count(tag) is None


def _check_waits(lines, wanted):
    """every s_waitcnt lgkmcnt(n) in `lines` stands for the tag of `wanted` (in order): n = the LGKM operations between the
    tagged operation and the wait"""
    waits = [i for i, x in enumerate(lines) if "s_waitcnt" in x]
    assert len(waits) == len(wanted)
    for i, op in zip(waits, wanted):
        at = lines.index("\t" + op)
        assert at < i
        n = sum(1 for x in lines[at + 1:i] if x.startswith("\tds_"))
        assert lines[i] == "\ts_waitcnt lgkmcnt(%d)" % n, (op, lines)


def test_counters_see_captured_side_work_in_program_order(emit):
    em = emit.Emitter("k")
    tags = {}

    def side(name):
        def fn():
            em.e("v_nop ; %s a" % name)
            tags[name] = em.lgkm_op("ds_read_b32 v1, v2 ; %s" % name)
            em.e("v_nop ; %s b" % name)
            em.wait_lgkm(tags[name])
            em.e("v_nop ; %s c" % name)
        return fn
    em.q(side("s0"))
    em.q(side("s1"))
    main = []
    for i in range(12):
        main.append(em.lgkm_op("ds_read_b128 v[4:7], v3 ; m%d" % i))
        em.drain_side(1)
        if i in (5, 11):
            em.wait_lgkm(main[i - 3])
    assert not em.side_busy()
    lines = em.o
    assert sum(1 for x in lines if x.startswith("\tds_")) == 14 and len(lines) == 12 + 2 * 5 + 2
    _check_waits(lines, ["ds_read_b32 v1, v2 ; s0", "ds_read_b128 v[4:7], v3 ; m2", "ds_read_b32 v1, v2 ; s1", "ds_read_b128 v[4:7], v3 ; m8"])
    # queue order would count nothing behind a side read (its wait follows it in the closure with one instruction between);
    # in program order two main-stream reads stand between them, one per drain_side(1)
    assert [x for x in lines if "s_waitcnt" in x] == ["\ts_waitcnt lgkmcnt(%d)" % n for n in (2, 3, 2, 3)]


def test_atomic_group_stays_together(emit):
    em = emit.Emitter("k")

    def fn():
        em.e("v_nop ; before")
        with em.atomic():
            em.e("s_mov_b64 exec, s[56:57]")
            em.lgkm_op("ds_write_b32 v1, v2")
            em.e("s_mov_b64 exec, -1")
        em.e("v_nop ; after")
    em.q(fn)
    while em.side_busy():
        em.e("v_mfma ; main")
        em.drain_side(1)
    o = em.o
    i = o.index("\ts_mov_b64 exec, s[56:57]")
    assert o[i:i + 3] == ["\ts_mov_b64 exec, s[56:57]", "\tds_write_b32 v1, v2", "\ts_mov_b64 exec, -1"]
    assert o == ["\tv_mfma ; main", "\tv_nop ; before", "\tv_mfma ; main"] + o[i:i + 3] + ["\tv_mfma ; main", "\tv_nop ; after"]
    assert em.lgkm.state() == [True]


def test_register_table(regs):
    regs.check()
    regs.check(list(regs.RANGES), list(regs.OVERLAPS), dict(regs.TOPS))
    moved = [(f, n, regs.V_RING + 8 if n == "V_ZZ" else lo, c) for f, n, lo, c in regs.RANGES]
    with pytest.raises(ValueError, match="V_RING and V_ZZ|V_ZZ and V_RING"):
        regs.check(moved, regs.OVERLAPS, regs.TOPS)
    for gone in regs.OVERLAPS:
        with pytest.raises(ValueError, match="not declared"):
            regs.check(regs.RANGES, [o for o in regs.OVERLAPS if o is not gone], regs.TOPS)
    with pytest.raises(ValueError, match="does not exist"):
        regs.check(regs.RANGES, regs.OVERLAPS + [("V_ZZ", "V_ZN", "never")], regs.TOPS)
    for f, n, lo, c in (("v", "V_OVER", 255, 2), ("a", "A_OVER", 256, 1), ("s", "S_OVER", regs.NEXT_FREE_SGPR, 1)):
        with pytest.raises(ValueError, match="leaves its file"):
            regs.check(regs.RANGES + [(f, n, lo, c)], regs.OVERLAPS, regs.TOPS)
    # the names the table lists are the module's constants
    assert all(getattr(regs, n) == lo for _, n, lo, _ in regs.RANGES)


def test_main_writes_every_variant_once(G, tmp_path, monkeypatch):
    out, units = tmp_path / "k.s", tmp_path / "units.txt"
    monkeypatch.setattr(sys, "argv", ["gen_mlp_tt.py", str(out), str(units)])
    G.main()
    text = out.read_text()
    names = ["k_mlp_tt_s%di%d" % x for x in ((1, 1), (2, 1), (0, 0), (1, 0), (2, 0), (3, 0))]
    for tap in (0, 1):
        for depth in (2, 1):
            for sm in (False, True):
                if (tap, depth, sm) != (0, 2, False):
                    names += [G.variant_name(tap, depth, sm, nbs, nbi) for nbs, nbi in ((1, 1), (2, 1), (1, 0), (2, 0), (3, 0))]
    assert len(names) == 41 and len(set(names)) == 41
    assert re.findall(r"^\t\.globl\t(\S+)$", text, re.M) == names
    assert re.findall(r"^    \.name: +(\S+)$", text, re.M) == names
    assert re.findall(r"^(k_mlp_tt\w*):$", text, re.M) == names
    g = G.Gen(2, 1, "x")
    assert units.read_text().splitlines() == ["%s %s" % (g.layers[u["layer"]]["name"], u["blocks"]) for u in g.units]
    assert len(g.units) == sum(1 for _ in g.units) > 0 and g.NC == len(g.chunks)
