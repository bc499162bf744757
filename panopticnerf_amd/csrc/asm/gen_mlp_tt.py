#!/usr/bin/env python3
"""Generator of k_mlp_tt: the fused inference MLP (NeRF trunk + heads + compositing epilogue) as
HAND-PLACED gfx950 assembly in the two-tile form -- ONE wave per SIMD (4 waves per workgroup, 512 registers per lane), TWO
32-sample tiles per wave, every 1 KiB weight fragment read from the LDS feeds two v_mfma_f32_32x32x16_bf16.

Why assembly: the form needs the activations in AGPRs (MFMA B operand), the accumulators in VGPRs (the pack / ReLU reads them
without a move) and every filler instruction placed in a specific MFMA gap; hipcc's schedule of the same loop runs 46 cycles per
MFMA where the hand-placed one runs 35.4 and the 8-wave ping-pong kernel 39.2 (profiles/README.md, round 5: r05a).

Same arithmetic as k_mlp_pp<256, false, FUSE, plan 1> (pnr_mlp.hip, pnr_mlp_fuse.h), operation for operation and in the same
order per value: outputs (per-tile records, per-sample quadruples) are BIT-IDENTICAL (tests/test_gpu_stages.py).  Consumes the
plan-2 image (pnr_mlp_plan.h): plan 1's chunk order, every chunk <= 33 fragments, sem1 / inst1 one chunk each.

Geometry (fixed): D = 8, W = 256, skip = 4, xyz_L = 10, dir_L = 4, head_W = 128, head_tap 0; NBS = 0 | 1 | 2 semantic logit blocks, with
NBS >= 1 also NBI = 0 | 1 instance logit blocks -> five kernels k_mlp_tt_s<NBS>i<NBI> (s0i0: no heads; s<n>i0: no instance head), and
four more for head_depth = 1 (one Linear W -> n per head, read from h: k_mlp_tt_d1_s<NBS>i<NBI>).

Time structure per 256-sample group (one workgroup; tile = (wave, t), record index grp * 8 + wave * 2 + t):
  image chunk c lives in LDS slot c % 4 (33 KiB each); during chunk c every wave issues its LDS-DMA pieces of chunk c + 3; at
  the end of chunk c: s_waitcnt vmcnt (own pieces of chunk c + 2 landed) + ONE s_barrier, so chunk c + 2 is readable during chunk
  c + 1.  MFMAs are grouped in UNITS (<= 2 output blocks x all k-steps x 2 tiles, one accumulator per (block, tile)); a unit's
  accumulators are packed / reduced while the NEXT unit's MFMAs run, the unit after that finds its bias already in its
  accumulators.  Weight fragments pass through a ring of 4 register quads, 3 fragments ahead, counted lgkmcnt.
  Side work (input fetch and gamma(x) of the NEXT group, the compositing epilogue) is a queue of instructions drained a few
  per MFMA gap; what depends on the RAY alone (|d|, gamma(d / |d|)) is loaded from the table k_ray_aux (pnr_mlp.hip) wrote.

This file is the kernel itself.  Beside it: tt_regs.py (the register map, checked at import), tt_emit.py (text, wait counters, side
queue), tt_plan.py (chunks, units, pieces), tt_math.py (the transcribed arithmetic)."""
import os
import sys

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:      # (loaded by path: tests/test_pack.py)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tt_math  # noqa: E402
import tt_plan  # noqa: E402
from tt_emit import Emitter  # noqa: E402
from tt_regs import *  # noqa: E402,F401,F403

# The training-forward prototype of this kernel (every packed activation block also stored, what k_mlp_fused<TRAIN> saves for the
# backward pass) was measured and is gone: its 2 x 2 against the shipped kernel is recorded in profiles/r06/r06p and DESIGN.md 7.


def vr(lo, n):
    return "v[%d:%d]" % (lo, lo + n - 1) if n > 1 else "v%d" % lo


def ar(lo, n):
    return "a[%d:%d]" % (lo, lo + n - 1) if n > 1 else "a%d" % lo


def sr(lo, n=2):
    return "s[%d:%d]" % (lo, lo + n - 1) if n > 1 else "s%d" % lo


class Loc:
    """where 4 consecutive packed-bf16 registers (one k-step of B operand) or one packed register lives"""
    def __init__(self, kind, base):
        self.kind, self.base = kind, base       # kind: 'a' | 'v'

    def reg(self, i, n=1):
        return (ar if self.kind == "a" else vr)(self.base + i, n)


class Gen(Emitter):
    def __init__(self, nbs, nbi, name, trace=False, abl=0, depth=2, softmax=False, tap=0):
        Emitter.__init__(self, name)
        # abl (trace builds only; results invalid): 1 = no LDS-DMA pieces in the loop, 2 = no chunk hand-over (vmcnt + barrier),
        # 4 = no pack / ReLU of the hidden layers
        # depth: pnr_mlp_desc.head_depth -- 2: heads W -> W/2 -> n (sem0 | inst0 | sem1 | inst1); 1: one Linear W -> n per head, straight from
        # the trunk output h (round 6: SURVEY.md 9 item 4 as a kernel variant, k_mlp_tt_d1_s<n>i<m>)
        self.depth = depth
        # tap: pnr_mlp_desc.head_tap -- 0: the heads read the trunk output h; 1: the feature_linear output F (round 6: k_mlp_tt_f..).  F must
        # then outlive the views layer: the last g block goes to the gamma(d) registers instead of F[0:15] (g_block), and the head
        # hidden layers' outputs to h -- dead once the rgb / sigma unit is issued -- instead of F (shs_block, shi_block)
        self.tap = tap
        # softmax: semantic_activation = softmax (PNR_MLP_SOFTMAX) -- the learned fields composite softmax(logits) over their channels;
        # the tail normalises each head's transposed logit blocks per sample before the weighted sums (tail_softmax), operation for
        # operation fuse_softmax_t of the ping-pong kernel (pnr_mlp_fuse.h): k_mlp_tt_sm_s<n>i<m>
        self.softmax = softmax
        self.nbs, self.nbi, self.trace, self.abl = nbs, nbi, trace, abl
        self.nstamp, self.last_stamp = 0, None
        self.ring_tags = [None] * P
        self.piece_tag = {}
        self.pending_pack = None
        self.g2_acc = self.park_acc = None
        self.m0 = None
        self.logit_units = []
        self.acc_free = list(range(8))
        self.lwr_acc = self.lwr_tag = None
        self.aux_tags = {}
        self.layers, self.chunks = tt_plan.build_plan(nbs, nbi, depth)
        self.NC = len(self.chunks)
        self.units = tt_plan.build_units(self.layers, self.chunks)
        self.stream = []
        for u in self.units:
            u["frag0"] = len(self.stream)
            self.stream += [(sl, of) for sl, of, _, _ in self.unit_frags(u)]

    def unit_frags(self, u):
        return tt_plan.unit_frags(self.layers, self.chunks, u)

    # ------------------------------------------------------------------ LDS-DMA
    def chunk_base(self, chunk):
        """s[S_PIECE : S_PIECE + 1] = address of image chunk `chunk` (once per chunk, in front of its first piece)"""
        self.e("s_add_u32 s%d, s%d, 0x%x" % (S_PIECE, S_IMG, self.chunks[chunk]["off"] * 1024))
        self.e("s_addc_u32 s%d, s%d, 0" % (S_PIECE + 1, S_IMG + 1))

    def piece(self, chunk, j):
        """piece j of image chunk `chunk` -> its LDS slot: M0 and the load (the address is the chunk's base + this lane's constant
        offset register + an immediate; the first version's per-piece 64-bit SALU add cost a third of a piece)"""
        m, i, nw = tt_plan.piece_list(self.chunks, chunk)[j]
        slot = chunk % NSLOT
        skip = None
        certain = nw >= 4
        if not certain:
            skip = self.label()
            self.e("s_cmp_ge_u32 s%d, %d" % (S_WAVE, nw))
            self.e("s_cbranch_scc1 %s" % skip)
        # the instruction's immediate offset moves BOTH addresses (memory and LDS): M0 carries the run's base only -- and stays
        # what it is for the four pieces of a run (nothing else in the loop writes M0; trace builds do)
        m0 = slot * SLOT + 16 * m * 1024
        if self.m0 != m0 or skip or self.trace:
            self.e("s_add_u32 m0, s%d, 0x%x" % (S_W4K, m0))
            self.e("s_nop 0")                   # SALU write of M0 -> LDS-DMA: one wait state
        self.m0 = None if skip else m0          # (a guarded piece: the waves that skipped it did not write M0)
        # default cache policy: " nt" missed the L2 for 20 % of the weight stream and cost 7 % in clock (profiles/r05/r05p, r05q)
        tag = self.vm_op("global_load_lds_dwordx4 v%d, s[%d:%d] offset:%d" % (V_DMA + m, S_PIECE, S_PIECE + 1, i * 1024), certain)
        if skip:
            self.o.append(skip + ":")
        return tag

    def issue_piece(self, chunk, j):
        """piece j of `chunk` with what goes in front of the first one; its tag is what the chunk's hand-over waits for"""
        if j == 0:
            self.chunk_base(chunk)
        self.piece_tag[chunk] = self.piece(chunk, j)

    def hand_over(self, chunk):
        """end of `chunk`: this wave's pieces of chunk + 2 have landed, and after ONE barrier everybody's have"""
        if not self.abl & 2:
            self.wait_vm(self.piece_tag.get((chunk + 2) % self.NC))
            self.e("s_barrier")

    # ------------------------------------------------------------------ operand locations of the layer inputs
    def loc_of(self, seg, layer_index, t, ks):
        """Loc of the 4 registers of k-step `ks` of segment `seg` for tile t"""
        if seg == "ex":
            return Loc("v", V_EX + 16 * t + 4 * ks)
        if seg == "ed":
            return Loc("v", V_ED + 8 * t + 4 * ks)
        if seg == "h":                  # the trunk's ping-pong: L1 reads A0 ... (layer i reads what layer i - 1 wrote)
            src = self.trunk_out(layer_index - 1)
            return Loc("a", src + 64 * t + 4 * ks)
        if seg == "tap":                # what the heads read: h, or the feature (head_tap 1)
            return Loc("a", (self.F_base() if self.tap else self.trunk_out(D - 1)) + 64 * t + 4 * ks)
        if seg == "hh":                 # the trunk output h = what L7 wrote
            return Loc("a", self.trunk_out(D - 1) + 64 * t + 4 * ks)
        if seg == "F":
            return Loc("a", self.F_base() + 64 * t + 4 * ks)
        if seg == "g":                  # 4 blocks of 8 registers: blocks 0, 1 in VGPRs, 2, 3 in the F array (dead after views)
            blk, r = ks // 2, (ks % 2) * 4
            return self.g_block(blk, t, r)
        if seg == "shs":
            blk, r = ks // 2, (ks % 2) * 4
            return self.shs_block(blk, t, r)
        if seg == "shi":
            blk, r = ks // 2, (ks % 2) * 4
            return self.shi_block(blk, t, r)
        raise KeyError(seg)

    @staticmethod
    def trunk_out(i):
        """array that trunk layer i writes: L0 -> A0, L1 -> A1, ..."""
        return A0 if i % 2 == 0 else A1

    def F_base(self):
        return A0 if self.trunk_out(D - 1) == A1 else A1        # feature: h (A1) -> F (A0)

    def g_block(self, blk, t, r=0):
        # a block's registers may be written while LATER views units still read F, so only the LAST block may live in F
        if blk < 2:
            return Loc("v", V_G + 16 * t + 8 * blk + r)
        if blk == 2:
            return Loc("v", self.acc_reg(self.g2_acc) + 8 * t + r)                  # an idle accumulator (views / rgbs units take two)
        if self.tap:
            # head_tap 1: F is read by the heads.  gamma(d) of THIS group is dead once the views layer's MFMAs are issued (the pack runs
            # during the rgb / sigma unit) and the next group's is encoded behind that unit: exactly [2 tiles][8] registers
            return Loc("v", V_ED + 8 * t + r)
        return Loc("a", self.F_base() + 8 * t + r)                                  # F[0:15] (packed during the rgb / sigma unit)

    def shs_block(self, blk, t, r=0):
        if self.tap:
            return Loc("a", self.trunk_out(D - 1) + 32 * t + 8 * blk + r)           # h[0:63]: dead since the rgb / sigma unit
        return Loc("a", self.F_base() + 32 + 32 * t + 8 * blk + r)                  # F[32:95]

    def shi_block(self, blk, t, r=0):
        if self.tap:
            return Loc("a", self.trunk_out(D - 1) + 64 + 32 * t + 8 * blk + r)      # h[64:127]
        # the last inst0 unit is packed while sem1's MFMAs still read shs: its blocks go to h (dead once inst0's MFMAs are issued)
        if blk < 2:
            return Loc("a", self.F_base() + 96 + 16 * t + 8 * blk + r)              # F[96:127]
        return Loc("a", self.trunk_out(D - 1) + 16 * t + 8 * (blk - 2) + r)         # h[0:31]

    def out_block(self, layer, blk, t):
        """Loc of the 8 packed registers of output block `blk` of `layer` for tile t"""
        n = layer["name"]
        if n.startswith("L"):
            return Loc("a", self.trunk_out(int(n[1:])) + 64 * t + 8 * blk)
        if n == "feature":
            return Loc("a", self.F_base() + 64 * t + 8 * blk)
        if n == "views":
            return self.g_block(blk, t)
        if n == "sem0":
            return self.shs_block(blk, t)
        if n == "inst0":
            return self.shi_block(blk, t)
        raise KeyError(n)

    # ------------------------------------------------------------------ the pieces of side work
    # ---- next group's inputs: address, loads (tile t), masks
    def fetch_tile(self, t, grp_sreg):
        """issue the loads of tile t of group s[grp_sreg]: ox oy oz dx | dy dz | zz | zn -> V_IN + 8 t; masks -> S_NVALID / S_NLAST"""
        e = self.e
        vi = V_IN + 8 * t
        s_, sl, ray, a64 = V_PTMP, V_PTMP + 1, V_PTMP + 2, V_PTMP + 4       # a64: 2 registers
        # s = (grp * 8 + wave * 2 + t) * 32 + n
        e("s_lshl_b32 s%d, s%d, 3" % (S_T0, grp_sreg))
        e("s_lshl_b32 s%d, s%d, 1" % (S_T1, S_WAVE))
        e("s_add_u32 s%d, s%d, s%d" % (S_T0, S_T0, S_T1))
        e("s_add_u32 s%d, s%d, %d" % (S_T0, S_T0, t))
        e("s_lshl_b32 s%d, s%d, 5" % (S_T0, S_T0))
        e("v_and_b32 v%d, 31, v%d" % (s_, V_TID))
        e("v_or_b32 v%d, s%d, v%d" % (s_, S_T0, s_))
        e("v_cmp_gt_i32 s[%d:%d], s%d, v%d" % (S_NVALID + 2 * t, S_NVALID + 2 * t + 1, S_S, s_))        # valid: s < S
        e("s_add_i32 s%d, s%d, -1" % (S_T1, S_S))
        e("v_min_i32 v%d, s%d, v%d" % (sl, S_T1, s_))                                   # sl = min(s, S - 1)
        e("v_mul_hi_u32 v%d, v%d, s%d" % (ray, sl, S_MAGIC))                            # ray = (sl * magic) >> shift, shift >= 32 ...
        e("v_mul_lo_u32 v%d, v%d, s%d" % (a64, sl, S_MAGIC))
        e("v_mov_b32 v%d, v%d" % (a64 + 1, ray))
        e("v_lshrrev_b64 v[%d:%d], s%d, v[%d:%d]" % (a64, a64 + 1, S_SHIFT, a64, a64 + 1))
        e("v_mov_b32 v%d, v%d" % (ray, a64))
        # last = (sl - ray * N + 1 == N)
        e("v_mul_lo_u32 v%d, v%d, s%d" % (a64, ray, S_N))
        e("v_sub_u32 v%d, v%d, v%d" % (a64, sl, a64))
        e("v_add_u32 v%d, 1, v%d" % (a64, a64))
        e("v_cmp_eq_u32 s[%d:%d], s%d, v%d" % (S_NLAST + 2 * t, S_NLAST + 2 * t + 1, S_N, a64))
        # this lane's line of the per-ray table: ray * 128 + hi * 64 (kept until the point is formed: aux_x)
        e("v_lshlrev_b32 v%d, 7, v%d" % (V_AUXA + t, ray))
        e("v_and_b32 v%d, 32, v%d" % (a64, V_TID))
        e("v_lshl_add_u32 v%d, v%d, 1, v%d" % (V_AUXA + t, a64, V_AUXA + t))
        # loads
        e("v_lshlrev_b32 v%d, 5, v%d" % (a64, ray))                                     # ray * 32 bytes (R * 32 < 2^32: R * N < 2^31, N >= 32)
        self.vm_op("global_load_dwordx4 %s, v%d, s[%d:%d]" % (vr(vi, 4), a64, S_RAYS, S_RAYS + 1))
        self.vm_op("global_load_dwordx2 %s, v%d, s[%d:%d] offset:16" % (vr(vi + 4, 2), a64, S_RAYS, S_RAYS + 1))
        e("v_lshlrev_b32 v%d, 2, v%d" % (a64, sl))
        self.vm_op("global_load_dword v%d, v%d, s[%d:%d]" % (vi + 6, a64, S_Z, S_Z + 1))
        e("v_add_u32 v%d, 1, v%d" % (a64 + 1, sl))
        e("v_cmp_gt_i32 vcc, s%d, v%d" % (S_S, a64 + 1))
        e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (a64 + 1, sl, a64 + 1))                  # min(sl + 1, S - 1) as HEAD: (sl + 1 < S) ? sl + 1 : sl
        e("v_lshlrev_b32 v%d, 2, v%d" % (a64 + 1, a64 + 1))
        return self.vm_op("global_load_dword v%d, v%d, s[%d:%d]" % (vi + 7, a64 + 1, S_Z, S_Z + 1))

    # ---- gamma(x), gamma(d), |d| of tile t from V_IN (results: V_EX / V_ED, and zz zn dn of the NEXT group parked in V_IN + {6, 7, 3})
    def encode_tile(self, t, part):
        """closures (side-queue pieces) that encode tile t.  part "x": point, |d|, gamma(x), q = d / |d| (into V_IN + 3..5);
        part "d": gamma(d) from q"""
        vi = V_IN + 8 * t
        T = list(range(V_TMP, V_TMP + 16))          # 16 temporaries
        s = T[0:3]
        c = T[3:6]
        q = T[6:9]                                  # the 3-vector being encoded
        w = T[9:15]                                 # sincos temps (6)
        tt = T[15]
        e = self.e
        ex, ed = V_EX + 16 * t, V_ED + 8 * t
        out = []

        def hi_select(dst, v_hi1, v_hi0):           # dst = hi ? v_hi1 : v_hi0   (S_HI0: lanes with hi == 0)
            e("v_cndmask_b32 v%d, v%d, v%d, s[%d:%d]" % (dst, v_hi1, v_hi0, S_HI0, S_HI0 + 1))

        def points():
            # p = o + d * z (separate multiply and add)
            for a in range(3):
                e("v_mul_f32 v%d, v%d, v%d" % (q[a], vi + 3 + a, vi + 6))
                e("v_add_f32 v%d, v%d, v%d" % (q[a], vi + a, q[a]))
        if part == "x":
            out.append(points)

        def aux_x():
            # |d| = sqrt((dx dx + dy dy) + dz dz) and gamma(d / |d|) are PER-RAY values: k_ray_aux (pnr_mlp.hip) computed them once per
            # ray, with the operations this kernel used to spend on them per sample (sqrt, three divisions, three sincos, a band step:
            # 188 instructions per tile).  Here: |d| into the ray record's `ox` slot, the table address into the `dx` slot -- both are
            # parked across the views layer (PARK) --, gamma(d) is loaded behind the rgb / sigma unit (part "d")
            self.aux_tags[t] = self.vm_op("global_load_dword v%d, v%d, s[%d:%d] offset:32" % (vi + 0, V_AUXA + t, S_AUX, S_AUX + 1))
            e("v_mov_b32 v%d, v%d" % (vi + 3, V_AUXA + t))
        if part == "x":
            out.append(aux_x)

        def xyz_reg():
            # reg 0 of gamma(x): pack(hi ? pz : px, hi ? 0 : py)
            hi_select(w[0], q[2], q[0])
            e("v_mov_b32 v%d, 0" % w[1])
            hi_select(w[1], w[1], q[1])
            e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (ex, w[0], w[1]))
            # base band of the half-wave: 2^5 for hi = 1
            e("v_mov_b32 v%d, 0x42000000" % tt)
            e("v_mov_b32 v%d, 1.0" % w[1])
            hi_select(tt, tt, w[1])
            for a in range(3):
                e("v_mul_f32 v%d, v%d, v%d" % (q[a], q[a], tt))         # p * base
        if part == "x":
            out.append(xyz_reg)
            for a in range(3):
                out.append(lambda a=a: tt_math.sincos(self, s[a], c[a], q[a], w))
            for fp in range(5):
                out.append(lambda fp=fp: tt_math.band_pack(self, ex + 1 + 3 * fp, s, c))
                if fp < 4:
                    out.append(lambda: tt_math.band_next(self, s, c, tt))

        if part == "x":
            out.append(lambda: self.wait_vm(self.aux_tags[t]))       # |d| has landed before anything (park) copies it
            return out

        def d_load():
            # this lane's eight packed registers of gamma(d): [x|y or z|0] [band 0 triple] [band 1 triple] [0], as embed_lane writes them
            self.vm_op("global_load_dwordx4 %s, v%d, s[%d:%d]" % (vr(ed, 4), vi + 3, S_AUX, S_AUX + 1))
            self.aux_tags[2 + t] = self.vm_op("global_load_dwordx4 %s, v%d, s[%d:%d] offset:16" % (vr(ed + 4, 4), vi + 3, S_AUX, S_AUX + 1))
        out.append(d_load)
        out.append(lambda: self.wait_vm(self.aux_tags[2 + t]))
        return out

    # ---- the compositing epilogue of the rgb / sigma block (fuse_rgbs) of tile t; acc = VGPR base of its accumulator
    def rgbs_epilogue(self, t, acc):
        e = self.e
        T = list(range(V_PTMP, V_PTMP + 8))
        d, x, y, n, al, f = T[0], T[1], T[2], T[3], T[4], T[5]
        VAL, LAST = S_VALID + 2 * t, S_LAST + 2 * t

        def alpha():
            # dist = last ? 1e10 : (zn - zz); x = (dist * -|d|) * relu(sigma)
            e("v_sub_f32 v%d, v%d, v%d" % (d, V_ZN + t, V_ZZ + t))
            e("v_mov_b32 v%d, 0x501502f9" % x)
            e("v_cndmask_b32 v%d, v%d, v%d, s[%d:%d]" % (d, d, x, LAST, LAST + 1))
            e("v_mul_f32 v%d, v%d, -v%d" % (d, d, V_DN + t))
            e("v_max_f32 v%d, v%d, v%d" % (x, acc + 3, acc + 3))
            e("v_max_f32 v%d, 0, v%d" % (x, x))
            e("v_mul_f32 v%d, v%d, v%d" % (x, d, x))
            # expf(x) (OCML's sequence as hipcc inlines it)
            self.lit(S_K, 0x3fb8aa3b)
            e("v_mul_f32 v%d, 0x3fb8aa3b, v%d" % (y, x))
            e("v_fma_f32 v%d, v%d, s%d, -v%d" % (d, x, S_K, y))
            e("v_rndne_f32 v%d, v%d" % (n, y))
            e("v_fmac_f32 v%d, 0x32a5705f, v%d" % (d, x))
            e("v_sub_f32 v%d, v%d, v%d" % (y, y, n))
            e("v_add_f32 v%d, v%d, v%d" % (y, y, d))
            e("v_exp_f32 v%d, v%d" % (y, y))
            e("v_cvt_i32_f32 v%d, v%d" % (n, n))
            e("s_nop 0")
            e("v_ldexp_f32 v%d, v%d, v%d" % (y, y, n))
            self.lit(S_K, 0xc2ce8ed0)
            e("v_cmp_ngt_f32 s[%d:%d], s%d, v%d" % (S_T0, S_T0 + 1, S_K, x))
            e("v_cndmask_b32 v%d, 0, v%d, s[%d:%d]" % (y, y, S_T0, S_T0 + 1))
            self.lit(S_K, 0x42b17218)
            e("v_cmp_nlt_f32 s[%d:%d], s%d, v%d" % (S_T0, S_T0 + 1, S_K, x))
            e("v_mov_b32 v%d, 0x7f800000" % n)
            e("v_cndmask_b32 v%d, v%d, v%d, s[%d:%d]" % (y, n, y, S_T0, S_T0 + 1))
            e("v_sub_f32 v%d, 1.0, v%d" % (al, y))                                   # alpha = 1 - exp
            e("v_cndmask_b32 v%d, 0, v%d, s[%d:%d]" % (al, al, VAL, VAL + 1))        # invalid lanes: 0
            # f = valid ? (1 - alpha) + 1e-10 : 1
            e("v_sub_f32 v%d, 1.0, v%d" % (f, al))
            e("v_add_f32 v%d, 0x2edbe6ff, v%d" % (f, f))
            e("v_mov_b32 v%d, 1.0" % n)
            e("v_cndmask_b32 v%d, v%d, v%d, s[%d:%d]" % (f, n, f, VAL, VAL + 1))
        self.q(alpha)

        def scan():
            # inclusive product over lanes 0..31 of each half (tile_scan): row_shr 1, 2, 4, 8, row_bcast15 into rows 1 and 3
            for ctrl in ("row_shr:1", "row_shr:2", "row_shr:4", "row_shr:8"):
                e("v_mov_b32 v%d, 1.0" % n)
                e("s_nop 1")
                e("v_mov_b32_dpp v%d, v%d %s row_mask:0xf bank_mask:0xf" % (n, f, ctrl))
                e("v_mul_f32 v%d, v%d, v%d" % (f, f, n))
            e("v_mov_b32 v%d, 1.0" % n)
            e("s_nop 1")
            e("v_mov_b32_dpp v%d, v%d row_bcast:15 row_mask:0xa bank_mask:0xf" % (n, f))
            e("v_mul_f32 v%d, v%d, v%d" % (f, f, n))
            e("v_mov_b32 v%d, 1.0" % n)
            e("s_nop 1")
            e("v_readlane_b32 s%d, v%d, 31" % (S_Q, f))                               # q = total of the tile
            e("v_mov_b32_dpp v%d, v%d wave_shr:1 row_mask:0xf bank_mask:0xf" % (n, f))
            e("v_cndmask_b32 v%d, v%d, 1.0, s[%d:%d]" % (n, n, S_N0, S_N0 + 1))        # lane n == 0: 1
            e("v_mul_f32 v%d, v%d, v%d" % (V_LW + t, al, n))                          # lw = alpha * exclusive product
            if self.nbs:
                # ... and into this wave's LDS table (lanes 0..31: sample n's weight at 4 n): the logit tail reads its per-register weights
                # lwr[r] = lw[row(r, hi)] back with ds_read_b64 (round 6; 64 v_readlane + 64 v_mov per group before: 864 cycles in the open)
                with self.atomic():
                    e("v_add_u32 v%d, s%d, v%d" % (n, S_LWW, V_LB4))
                    e("s_mov_b64 exec, s[%d:%d]" % (S_HI0, S_HI0 + 1))
                    self.lgkm_op("ds_write_b32 v%d, v%d offset:%d" % (n, V_LW + t, 128 * t))
                    e("s_mov_b64 exec, -1")
        self.q(scan)

        def stores():
          with self.atomic():
            # rec pointer of this tile: rec + (grp * 8 + wave * 2 + t) * rec_floats * 4
            e("s_lshl_b32 s%d, s%d, 3" % (S_T0, S_GRP))
            e("s_lshl_b32 s%d, s%d, 1" % (S_SAVE, S_WAVE))
            e("s_add_u32 s%d, s%d, s%d" % (S_T0, S_T0, S_SAVE))
            e("s_add_u32 s%d, s%d, %d" % (S_T0, S_T0, t))
            e("s_mul_i32 s%d, s%d, s%d" % (S_SAVE, S_T0, S_RECF))
            e("s_mul_hi_i32 s%d, s%d, s%d" % (S_SAVE + 1, S_T0, S_RECF))
            e("s_lshl_b64 s[%d:%d], s[%d:%d], 2" % (S_SAVE, S_SAVE + 1, S_SAVE, S_SAVE + 1))
            e("s_add_u32 s%d, s%d, s%d" % (S_REC_T + 2 * t, S_REC, S_SAVE))
            e("s_addc_u32 s%d, s%d, s%d" % (S_REC_T + 2 * t + 1, S_REC + 1, S_SAVE + 1))
            e("s_lshl_b32 s%d, s%d, 2" % (S_SAVE, S_NSEM))                            # ... and of its instance columns
            e("s_add_u32 s%d, s%d, s%d" % (S_REC_I + 2 * t, S_REC_T + 2 * t, S_SAVE))
            e("s_addc_u32 s%d, s%d, 0" % (S_REC_I + 2 * t + 1, S_REC_T + 2 * t + 1))
            # ps[samp] = (lw, r, g, b): lanes hi == 0 and valid; byte offset (s0 * 16) fits 32 bits (S < 2^27 ... checked by the launcher)
            e("s_lshl_b32 s%d, s%d, 5" % (S_T0, S_T0))
            e("v_and_b32 v%d, 31, v%d" % (d, V_TID))
            e("v_or_b32 v%d, s%d, v%d" % (d, S_T0, d))
            e("v_lshlrev_b32 v%d, 4, v%d" % (d, d))
            e("v_mov_b32 v%d, v%d" % (T[4], V_LW + t))
            e("v_mov_b32 v%d, v%d" % (T[5], acc + 0))
            e("v_mov_b32 v%d, v%d" % (T[6], acc + 1))
            e("v_mov_b32 v%d, v%d" % (T[7], acc + 2))
            e("s_and_b64 s[%d:%d], s[%d:%d], s[%d:%d]" % (S_SAVE, S_SAVE + 1, VAL, VAL + 1, S_HI0, S_HI0 + 1))
            e("s_mov_b64 exec, s[%d:%d]" % (S_SAVE, S_SAVE + 1))
            # default cache policy of the record / quadruple stores: " nt" measured +-0 (profiles/README.md, round 5 ablation table)
            self.vm_op("global_store_dwordx4 v%d, %s, s[%d:%d]" % (d, vr(T[4], 4), S_PS, S_PS + 1))
            e("s_mov_b64 exec, 1")                                                   # lane 0: rec[0] = q
            e("v_mov_b32 v%d, s%d" % (x, S_Q))
            e("v_mov_b32 v%d, 0" % d)
            self.vm_op("global_store_dword v%d, v%d, s[%d:%d]" % (d, x, S_REC_T + 2 * t, S_REC_T + 2 * t + 1))
            e("s_mov_b64 exec, -1")
        self.q(stores)

    # ------------------------------------------------------------------ accumulators
    def acc_reg(self, i):
        return V_ACC + 16 * i           # in order: swapped / interleaved register blocks measured +-0 (profiles/r05/r05v)

    def acc_take(self, n):
        assert len(self.acc_free) >= n, ("accumulators exhausted", self.acc_free)
        got, self.acc_free = self.acc_free[:n], self.acc_free[n:]
        return got

    def acc_release(self, ids):
        self.acc_free = sorted(set(self.acc_free) | set(ids))

    # ------------------------------------------------------------------ arming: the bias of a unit into freshly taken accumulators
    def arm_plan(self, u):
        """per accumulator of unit u (block-major, tile-minor): a list of closures, one LDS read each, that put the bias into it;
        the first closure of an accumulator TAKES it (u['accs'] fills as the closures run)"""
        c = self.chunks[u["chunk"]]
        l = self.layers[u["layer"]]
        slot = u["chunk"] % NSLOT
        bias_off = c["nfb"] * l["nks"] * 1024
        u["accs"], u["arm_tags"] = {}, []
        plans = []
        for bi, blk in enumerate(u["blocks"]):
            b_in_chunk = blk - c["fb"]
            for t in range(2):
                key = (bi, t)
                ops = []

                def take(key=key):
                    while not self.acc_free and self.side_busy():       # a queued epilogue still holds accumulators: run it now
                        self.drain_side(8)
                    u["accs"][key] = self.acc_take(1)[0]
                if t == 1:
                    # the two tiles of a block start from the SAME bias: tile 1's first MFMA takes tile 0's armed accumulator as its
                    # C operand (emit_unit issues it in front of tile 0's) -- its own accumulator is only taken, never armed: half the
                    # arming reads (408 of the 816 LDS reads per group), same values: -1.9 % (profiles/r06/r06m)
                    plans.append([take])
                    continue
                if l["mode"] == "logits":       # transposed product: every register = bias of channel lane & 31
                    def first(key=key, slot=slot, take=take):           # the address lives in the accumulator's first register, read last
                        take()
                        self.e("v_add_u32 v%d, 0x%x, v%d" % (self.acc_reg(u["accs"][key]), slot * SLOT, V_LB4))
                    ops.append(first)
                    for r in list(range(1, 16)) + [0]:
                        ops.append(lambda key=key, r=r, off=bias_off + b_in_chunk * 128: u["arm_tags"].append(
                            self.lgkm_op("ds_read_b32 v%d, v%d offset:%d" % (self.acc_reg(u["accs"][key]) + r, self.acc_reg(u["accs"][key]), off))))
                else:
                    for m in range(4):
                        def rd(key=key, m=m, off=bias_off + b_in_chunk * 128 + m * 32, take=take):
                            if m == 0:
                                take()
                            a = self.acc_reg(u["accs"][key])
                            u["arm_tags"].append(self.lgkm_op("ds_read_b128 %s, v%d offset:%d" % (vr(a + 4 * m, 4), V_BIAS + slot, off)))
                        ops.append(rd)
                plans.append(ops)
        return plans

    # ------------------------------------------------------------------ pack / ReLU of a unit's accumulators -> list of (dst, closure)
    def pack_ops(self, u):
        l = self.layers[u["layer"]]
        if not self.trace:
            return self.pack_ops_pipelined(u)
        out = []
        for bi, blk in enumerate(u["blocks"]):
            for t in range(2):
                a = self.acc_reg(u["accs"][(bi, t)])
                dst = self.out_block(l, blk, t)
                for p in range(8):
                    def fn(a=a, p=p, dst=dst, relu=(l["mode"] == "relu"), k=len(out)):
                        tmp = V_T0 if (k & 1) else V_T1
                        if dst.kind == "v" and relu:
                            self.e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (tmp, a + 2 * p, a + 2 * p + 1))
                            self.e("v_pk_max_i16 v%d, v%d, 0" % (dst.base + p, tmp))
                        elif dst.kind == "v":
                            self.e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (dst.base + p, a + 2 * p, a + 2 * p + 1))
                        else:
                            self.e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (tmp, a + 2 * p, a + 2 * p + 1))
                            if relu:
                                self.e("v_pk_max_i16 v%d, v%d, 0" % (tmp, tmp))
                            self.e("v_accvgpr_write_b32 a%d, v%d" % (dst.base + p, tmp))
                    out.append(((dst.kind, dst.base + p), fn, u["accs"][(bi, t)]))
        return out

    def pack_ops_pipelined(self, u):
        """-> [([destinations final after this closure], closure, accumulator)]: the pack / ReLU / v_accvgpr_write triples as a
        three-stage software pipeline over the packed registers of a unit (closure j: write of pair j - 2, ReLU of pair j - 1,
        convert of pair j; three rotating temporaries) -- no instruction of a closure depends on another one of the same closure,
        where the plain form is three DEPENDENT instructions back to back: -0.35 % (profiles/r06/r06s)"""
        l = self.layers[u["layer"]]
        relu = l["mode"] == "relu"
        pairs = []
        for bi, blk in enumerate(u["blocks"]):
            for t in range(2):
                a = self.acc_reg(u["accs"][(bi, t)])
                dst = self.out_block(l, blk, t)
                for p in range(8):
                    pairs.append((a + 2 * p, dst.kind, dst.base + p, u["accs"][(bi, t)]))
        T = (V_T0, V_T1, V_T2)
        n = len(pairs)

        def convert(k):
            src, kind, d, _ = pairs[k]
            self.e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (d if (kind == "v" and not relu) else T[k % 3], src, src + 1))

        def activate(k):
            _, kind, d, _ = pairs[k]
            if relu:
                self.e("v_pk_max_i16 v%d, v%d, 0" % (d if kind == "v" else T[k % 3], T[k % 3]))

        def store(k):
            _, kind, d, _ = pairs[k]
            if kind == "a":
                self.e("v_accvgpr_write_b32 a%d, v%d" % (d, T[k % 3]))

        def final_at(k):
            kind = pairs[k][1]
            return k + 2 if kind == "a" else (k + 1 if relu else k)
        out = []
        for j in range(n + 2):
            def fn(j=j):
                if 0 <= j - 2 < n:
                    store(j - 2)
                if 0 <= j - 1 < n:
                    activate(j - 1)
                if j < n:
                    convert(j)
            done = [(pairs[k][1], pairs[k][2]) for k in range(max(0, j - 2), min(n, j + 1)) if final_at(k) == j]
            out.append((done, fn, pairs[min(j, n - 1)][3]))
        return out

    # ------------------------------------------------------------------ one unit of MFMAs with its fillers
    @staticmethod
    def tile_at(ks, t):
        """the tile of the t-th MFMA of a fragment: (0, 1), except at a block's first k-step (the shared bias, arm_plan): (1, 0)"""
        return 1 - t if ks == 0 else t

    def b_operand(self, u, ks, t):
        seg, k = tt_plan.seg_of_ks(self.layers[u["layer"]], ks)
        return self.loc_of(seg, u["layer"], t, k)

    def emit_unit(self, ui):
        u = self.units[ui]
        l = self.layers[u["layer"]]
        nm = 2 * len(self.unit_frags(u))
        self.e("; ==== unit %d: %s blocks %s (chunk %d, slot %d), %d MFMAs" % (ui, l["name"], u["blocks"], u["chunk"], u["chunk"] % NSLOT, nm))
        self.stamp(ui)
        hook = self.group_hooks().get((l["name"], u["blocks"][0]))
        if hook:
            hook()
        musts, lwr_from = self.unit_musts(ui)
        # nothing to pack (the previous unit's results go through the side queue and hold their accumulators until then): arm in
        # the unit's last third
        late = bool(musts) and ui + 1 < len(self.units) and not any(is_pack for _, _, is_pack in musts)
        must_at = self.place_musts(musts, nm, lwr_from, late)
        piece_at = self.place_pieces(ui, nm, musts, must_at)
        self.mfma_loop(u, [fn for fn, _, _ in musts], must_at, piece_at,
                       1 if l["name"].startswith("L") or l["name"] in ("feature", "views") else 3 if late else 2)
        self.unit_results(u)
        if u["last_of_chunk"]:
            self.end_chunk(u["chunk"])

    def group_hooks(self):
        """(layer, first block) of the unit in front of which something happens once per group -> what"""
        first_head = ("sem0" if self.nbs else "inst0") if self.depth == 2 else "sem1"
        return {("L%d" % (SKIP + 2), 0): self.queue_inputs_early,
                ("views", 0): self.drain_side,          # (nothing left normally) the early side work uses the g area
                ("views", 1): self.park,
                ("views", 2): self.take_g2,
                (first_head, 0): self.unpark}

    def take_g2(self):
        self.g2_acc = self.acc_take(1)[0]           # home of g block 2 (packed during the next unit) until the rgb / sigma unit is issued

    def unit_musts(self, ui):
        """what has to happen inside unit ui, in program order -> ([(closure, deadline, is_pack)], index of the first local-weight
        read or None); deadline: the MFMA (index in the unit) that must find the closure done, or None"""
        u = self.units[ui]
        frags = self.unit_frags(u)
        # (1) the previous unit's pack / ReLU, each before the first MFMA of THIS unit that reads its destination
        prev = self.pending_pack
        self.pending_pack = None
        packs = prev["ops"] if prev else []
        reads = {}
        for i in range(2 * len(frags)):
            f, t = i // 2, i % 2
            loc = self.b_operand(u, frags[f][2], self.tile_at(frags[f][2], t))
            for r in range(4):
                reads.setdefault((loc.kind, loc.base + r), i)
        # ... and, pipelined with it, the NEXT unit's bias: as soon as an accumulator is packed it is released and re-armed.  One list
        # of "musts" in program order, spread evenly over the unit's gaps (the first version packed in the first 60 % of the gaps
        # and armed in the last 25 %: up to seven fillers per gap where five hide, and nothing to do in between)
        nxt = self.units[ui + 1] if ui + 1 < len(self.units) else None
        plans = self.arm_plan(nxt) if nxt is not None else []
        musts = []
        by_acc = {}
        for dst, fn, a in packs:
            by_acc.setdefault(a, []).append((dst, fn))
        k = 0
        for a, lst in by_acc.items():
            for dst, fn in lst:
                if isinstance(dst, list):           # pipelined packs: every destination that becomes final in this closure
                    dd = [reads[d] for d in dst if d in reads]
                    dl = min(dd) if dd else None
                else:
                    dl = reads.get(dst)
                musts.append((fn if not self.abl & 4 else (lambda: None), dl, True))
            musts.append((lambda a=a: self.acc_release([a]), None, False))
            if k < len(plans):
                musts += [(op, None, False) for op in plans[k]]
                k += 1
        for kk in range(k, len(plans)):
            musts += [(op, None, False) for op in plans[kk]]
        lwr_from = None
        if nxt is None and (self.logit_units or self.layers[u["layer"]]["mode"] == "logits"):
            # the group's last unit: the logit tail's per-register weights lwr[r] = lw[row(r, hi)] of both tiles come back from the LDS
            # table (rgbs_epilogue: scan) into the two accumulators nobody holds any more -- behind the packs that release them
            lwr_from = len(musts)
            musts += [(op, None, False) for op in self.lwr_ops()]
        return musts, lwr_from

    @staticmethod
    def place_musts(musts, nm, lwr_from, late):
        """-> {gap: [indices into musts]}: the musts spread over the unit's nm gaps, none behind its deadline"""
        n = len(musts)
        pos = []
        for j, (_, dl, _) in enumerate(musts):
            spread = 1 + (j * max(1, nm - 6)) // max(1, n) if not late else (2 * nm) // 3 + (j * max(1, nm // 3 - 5)) // max(1, n)
            pos.append(spread if dl is None else min(spread, max(0, dl - 2)))
        if lwr_from is not None:                        # the local-weight reads: in the unit's second half (the side queue drains first)
            nl = n - lwr_from
            for j in range(lwr_from, n):
                pos[j] = max(pos[j], min(nm - 2, nm // 2 + ((j - lwr_from) * max(1, nm // 2 - 3)) // nl))
        for j in range(n - 2, -1, -1):                  # program order: a must never after a later must's position
            pos[j] = min(pos[j], pos[j + 1])
        must_at = {}
        for j, g in enumerate(pos):
            assert g < nm, (g, nm)                      # (positions beyond the last gap: none by construction)
            must_at.setdefault(g, []).append(j)
        return must_at

    def place_pieces(self, ui, nm, musts, must_at):
        """-> {gap: [piece indices]}: this unit's share of the LDS-DMA pieces of chunk + 3 (they are spread over the chunk's units),
        each in the cheapest gap of its stretch"""
        U = self.units
        piece_at = {}
        cu = [k for k, x in enumerate(U) if x["chunk"] == U[ui]["chunk"]]
        npieces = tt_plan.pieces_of(self.chunks, (U[ui]["chunk"] + 3) % self.NC)
        k_in = cu.index(ui)
        mine = [j for j in range(npieces) if (j * len(cu)) // npieces == k_in]
        # what a gap already holds: a pack or a must with a deadline weighs 4, any other must 1, a piece 2
        cost = [sum(4 if musts[j][1] is not None or musts[j][2] else 1 for j in must_at.get(g, [])) for g in range(nm)]
        for idx, j in enumerate(mine):
            span = max(len(mine) + 1, nm - 3)       # over all of the unit's gaps (the first half only: measured slower, round 5)
            lo = 1 + (idx * span) // max(1, len(mine))
            hi = max(lo + 1, 1 + ((idx + 1) * span) // max(1, len(mine)))
            g = min(range(lo, min(hi, nm - 1)), key=lambda x: (cost[x], x))
            cost[g] += 2
            piece_at.setdefault(g, []).append(j)
        return piece_at

    def mfma_loop(self, u, fillers, must_at, piece_at, side_budget):
        """the unit's MFMAs; in the gap behind each: the ring's next fragment, the gap's musts (fillers[j] for j in must_at), its
        pieces of chunk + 3 and side_budget instructions of side work"""
        e = self.e
        frags = self.unit_frags(u)
        swap = self.layers[u["layer"]]["mode"] == "logits"
        c3 = (u["chunk"] + 3) % self.NC
        first_wait_done = False
        for i in range(2 * len(frags)):
            f, t = i // 2, i % 2
            slot, off, ks, bi = frags[f]
            gi = u["frag0"] + f                                    # index in the group's fragment stream
            if t == 0:
                if not first_wait_done:
                    for tg in u["arm_tags"][-1:]:
                        self.wait_lgkm(tg)                          # the unit's bias has landed (in-order: the last read covers all)
                    first_wait_done = True
                self.wait_lgkm(self.ring_tags[gi % P])          # one counted wait per fragment (per TWO: +-0, profiles/r06/r06m)
            tile = self.tile_at(ks, t)
            a = self.acc_reg(u["accs"][(bi, tile)])
            # a block's first k-step: tile 1 first, reading the bias out of tile 0's accumulator, then tile 0 in place
            c_in = self.acc_reg(u["accs"][(bi, 0)]) if ks == 0 else a
            bloc = self.b_operand(u, ks, tile)
            ring = vr(V_RING + 4 * (gi % P), 4)
            if swap:
                e("v_mfma_f32_32x32x16_bf16 %s, %s, %s, %s" % (vr(a, 16), bloc.reg(0, 4), ring, vr(c_in, 16)))
            else:
                e("v_mfma_f32_32x32x16_bf16 %s, %s, %s, %s" % (vr(a, 16), ring, bloc.reg(0, 4), vr(c_in, 16)))
            # ---- fillers of gap i
            if t == 1:
                gn = gi + P - 1
                if gn < len(self.stream):
                    sl, of = self.stream[gn]
                    self.ring_tags[gn % P] = self.lgkm_op("ds_read_b128 %s, v%d offset:%d" % (vr(V_RING + 4 * (gn % P), 4), V_FRAG + sl, of))
            for j in must_at.get(i, []):
                fillers[j]()
            for j in ([] if self.abl & 1 else piece_at.get(i, [])):
                self.issue_piece(c3, j)
            self.drain_side(side_budget)

    def unit_results(self, u):
        """what becomes of the unit's accumulators: packed during the next unit, or reduced by the side queue, or kept for the tail"""
        l = self.layers[u["layer"]]
        if l["mode"] in ("relu", "linear"):
            self.pending_pack = dict(ops=self.pack_ops(u), accs=list(u["accs"].values()))
        elif l["mode"] == "rgbs":
            for t in range(2):
                self.rgbs_epilogue(t, self.acc_reg(u["accs"][(0, t)]))
            ids = list(u["accs"].values())
            self.q(lambda: self.defer(lambda: self.acc_release(ids)))
            self.queue_inputs_late()
            self.acc_release([self.g2_acc])         # g is dead: every MFMA of the rgb / sigma unit has been issued
            self.g2_acc = None
            if not self.nbs:                        # no head follows (its first unit would do this): the parked inputs go home
                self.unpark()
        else:
            # logit blocks keep their accumulators until the group's tail (tail_logits): all blocks of a tile are reduced TOGETHER there,
            # three independent FMA chains beside each other -- one block at a time is a chain of 16 dependent FMAs and two LDS
            # round trips with nothing to overlap them (the first version's tail: 2650 cycles)
            self.logit_units.append(u)

    def end_chunk(self, chunk):
        """the hand-over behind a chunk's last unit, and the dummy chunks behind the group's last real chunk: their share of the
        weight stream (the pieces of chunk + 3) and their hand-over, with whatever side work is queued between the pieces"""
        self.hand_over(chunk)
        d = chunk + 1
        while d < self.NC and self.chunks[d].get("dummy"):
            self.e("; ==== dummy chunk %d (slot %d)" % (d, d % NSLOT))
            for j in ([] if self.abl & 1 else range(tt_plan.pieces_of(self.chunks, (d + 3) % self.NC))):
                self.issue_piece((d + 3) % self.NC, j)
                self.drain_side(2)
            self.hand_over(d)
            d += 1

    def tail_softmax(self, blocks, lwr_reg, tag_lwr):
        """semantic_activation = softmax: per head and tile, IN PLACE -- the head's logit accumulators become e = exp(x - max) and the
        tile's lwr registers become lwr / denominator, so that the FMA chains that follow (the logits tail, unchanged) form
        sum_r (lwr[r] / den[r]) e[r] = the record column of softmax(logits).  Lane = channel, register r = sample row(r, hi): maximum
        and denominator of a sample are reductions over the 32 lanes of each half-wave -- quad_perm / row_half_mirror / row_mirror
        DPP steps and v_permlane16_swap for the xor-16 step, all sixteen registers of both tiles per step back to back (independent).
        Operation for operation fuse_softmax_t (pnr_mlp_fuse.h): max_raw chain, xor_max 1 2 4 8 16, mm = -m log2e, e = exp2(fma(x, log2e,
        mm)), d = e_0 (+ e_1), xor_add 1 2 4 8, swap-add 16, lwr * rcp(d).  Channels past the head's last are set to -inf first (the
        ping-pong kernel starts their accumulators there): exp makes them 0.  The lwr registers are consumed head by head: the
        semantic head's FMA chains are issued before the instance head rescales them."""
        e = self.e
        M = (V_TMP, V_RING)                         # m / d of the tile: 16 registers each (g area; the fragment ring is idle at a group's end)
        TMP = [V_SMX + i for i in range(4)]         # temporaries of the xor-16 steps
        ninf = V_PTMP + 6
        heads = []
        for inst in (False, True):
            hb = [(u, bi, blk) for (u, bi, blk, i2) in blocks if i2 == inst]
            if hb:
                heads.append((inst, hb))
        for t in (0, 1):
            self.wait_lgkm(tag_lwr[t])
        e("v_mov_b32 v%d, 0xff800000" % ninf)

        def xor16(op):
            # x op x[lane ^ 16] through v_permlane16_swap on two copies (one ends up with rows {0, 0, 2, 2}, the other {1, 1, 3, 3}); four
            # registers at a time: a VALU write needs two wait states before v_permlane16_swap reads it, and so does the swap's result
            regs = [M[t] + r for t in (0, 1) for r in range(16)]
            for g in range(0, 32, 4):
                for i in range(4):
                    e("v_mov_b32 v%d, v%d" % (TMP[i], regs[g + i]))
                for i in range(4):
                    e("v_permlane16_swap_b32 v%d, v%d" % (regs[g + i], TMP[i]))
                for i in range(4):
                    e("%s v%d, v%d, v%d" % (op, regs[g + i], regs[g + i], TMP[i]))
        for inst, hb in heads:
            accs = [[self.acc_reg(u["accs"][(bi, t)]) for (u, bi, blk) in hb] for t in (0, 1)]      # [tile][block] -> first register
            NB = len(hb)
            vm = S_VMSK + 2 * (1 if inst else 0)
            for t in (0, 1):                        # the head's LAST block: channels >= n_out -> -inf
                for r in range(16):
                    e("v_cndmask_b32 v%d, v%d, v%d, s[%d:%d]" % (accs[t][NB - 1] + r, ninf, accs[t][NB - 1] + r, vm, vm + 1))
            # m[r] = max over the head's blocks (max_raw chain), then the 32-lane butterfly
            first_src = None
            if NB > 1:
                for t in (0, 1):
                    for r in range(16):
                        e("v_max_f32 v%d, v%d, v%d" % (M[t] + r, accs[t][0] + r, accs[t][1] + r))
                        for b in range(2, NB):
                            e("v_max_f32 v%d, v%d, v%d" % (M[t] + r, M[t] + r, accs[t][b] + r))
            else:
                first_src = [accs[t][0] for t in (0, 1)]
            for k, ctrl in enumerate(("quad_perm:[1,0,3,2]", "quad_perm:[2,3,0,1]", "row_half_mirror", "row_mirror")):
                for t in (0, 1):
                    for r in range(16):
                        src = (first_src[t] + r) if (k == 0 and first_src) else (M[t] + r)
                        e("v_max_f32_dpp v%d, v%d, v%d %s row_mask:0xf bank_mask:0xf bound_ctrl:1" % (M[t] + r, src, src, ctrl))
            xor16("v_max_f32")
            # mm = -m log2(e);  e = exp2(fma(x, log2 e, mm));  d = e_0 + e_1 ...
            for t in (0, 1):
                for r in range(16):
                    e("v_mul_f32 v%d, 0xbfb8aa3b, v%d" % (M[t] + r, M[t] + r))
            for t in (0, 1):
                for r in range(16):
                    for b in range(NB):
                        e("v_fmamk_f32 v%d, v%d, 0x3fb8aa3b, v%d" % (accs[t][b] + r, accs[t][b] + r, M[t] + r))
                        e("v_exp_f32 v%d, v%d" % (accs[t][b] + r, accs[t][b] + r))
            first_src = None
            if NB > 1:
                for t in (0, 1):
                    for r in range(16):
                        e("v_add_f32 v%d, v%d, v%d" % (M[t] + r, accs[t][0] + r, accs[t][1] + r))
                        for b in range(2, NB):
                            e("v_add_f32 v%d, v%d, v%d" % (M[t] + r, M[t] + r, accs[t][b] + r))
            else:
                first_src = [accs[t][0] for t in (0, 1)]
            for k, ctrl in enumerate(("quad_perm:[1,0,3,2]", "quad_perm:[2,3,0,1]", "row_half_mirror", "row_mirror")):
                for t in (0, 1):
                    for r in range(16):
                        src = (first_src[t] + r) if (k == 0 and first_src) else (M[t] + r)
                        e("v_add_f32_dpp v%d, v%d, v%d %s row_mask:0xf bank_mask:0xf bound_ctrl:1" % (M[t] + r, src, src, ctrl))
            xor16("v_add_f32")
            # wr[r] = lwr[r] * rcp(d[r]): kept in M (the lwr registers stay what they are for the next head)
            for t in (0, 1):
                for r in range(16):
                    e("v_rcp_f32 v%d, v%d" % (M[t] + r, M[t] + r))
            for t in (0, 1):
                for r in range(16):
                    e("v_mul_f32 v%d, v%d, v%d" % (M[t] + r, lwr_reg(t, r), M[t] + r))
            # this head's FMA chains against wr (fmas() is told to skip them): s = sum_r wr[r] e[r]
            for r in range(16):
                for t in (0, 1):
                    for (u, bi, blk) in hb:
                        kk = [i for i, (u2, bi2, blk2, i2) in enumerate(blocks) if u2 is u and bi2 == bi][0]
                        a = self.acc_reg(u["accs"][(bi, t)])
                        dst = self.sm_sums[t][kk]
                        if r == 0:
                            e("v_fma_f32 v%d, v%d, v%d, 0" % (dst, M[t], a))
                        else:
                            e("v_fmac_f32 v%d, v%d, v%d" % (dst, M[t] + r, a + r))

    def lwr_ops(self):
        """closures (one instruction each) that load lwr of both tiles: 8 ds_read_b64 per tile.  lw[8 q + 4 hi + j], j = 0..3, is
        register 4 q + ((j + 2) & 3) of the tile's block -- two positions round its quad, so that the tail's FMA (lwr[r] x register r
        of a 16-aligned accumulator) reads its two operands from different VGPR banks (register number mod 4)"""
        ops = []

        def first():
            # the table is written by the rgb / sigma unit's epilogue (scan), which is side work: everything of it that is still queued
            # goes out NOW, in front of the reads (head_depth 1 without an instance head: the last unit follows the rgb / sigma unit
            # directly -- the reads returned the previous group's weights), and with it the accumulators that epilogue holds
            while self.side or self.outbox or (len(self.acc_free) < 2 and self.side_busy()):
                self.drain_side(8)
            assert len(self.acc_free) >= 2, ("no free accumulators for the local weights", self.acc_free)
            self.lwr_acc = self.acc_take(2)
            self.e("v_add_u32 v%d, s%d, v%d" % (V_LWA, S_LWR, V_BIAS + 0))
        ops.append(first)
        for t in range(2):
            for q in range(4):
                for h2 in range(2):
                    def rd(t=t, q=q, h2=h2):
                        dst = self.acc_reg(self.lwr_acc[t]) + 4 * q + ((2 * h2 + 2) & 3)
                        self.lwr_tag = self.lgkm_op("ds_read_b64 %s, v%d offset:%d" % (vr(dst, 2), V_LWA, 128 * t + 32 * q + 8 * h2))
                    ops.append(rd)
        return ops

    def logit_blocks(self):
        return [(b, False) for b in range(self.nbs)] + [(0, True)] * self.nbi

    def tail_logits(self):
        """the group's logit blocks -> record columns (fuse_logits_t).  Both tiles pipelined: lwr of tile 0 and tile 1 (the fragment
        ring is idle at a group's end: its registers hold tile 1's), tile 0's FMAs -- every block's chain side by side --, its
        exchanges between the half-waves, tile 1's FMAs beside them, then the stores.  Masks and the instance columns' pointers are
        precomputed (S_MSK, S_REC_I)."""
        e = self.e
        if not self.logit_units:
            return
        blocks = []
        for u in self.logit_units:
            inst = self.layers[u["layer"]]["name"] == "inst1"
            for bi, blk in enumerate(u["blocks"]):
                blocks.append((u, bi, blk, inst))
        nb = len(blocks)
        lwr = tuple(self.acc_reg(a) for a in self.lwr_acc)

        def lwr_reg(t, r):
            return lwr[t] + 4 * (r >> 2) + (((r & 3) + 2) & 3)            # see lwr_ops
        sums = ([V_PTMP + k for k in range(nb)], [V_IN + 1 + k for k in range(nb)])
        oth = ([V_PTMP + 3 + k for k in range(nb)], [V_IN + 4, V_IN + 5, V_IN + 9][:nb])
        adr = V_PTMP + 7
        tag_lwr = [self.lwr_tag, self.lwr_tag]          # (in order: the last read covers all sixteen)
        e("v_xor_b32 v%d, 32, v%d" % (adr, V_TID))
        e("v_and_b32 v%d, 63, v%d" % (adr, adr))
        e("v_lshlrev_b32 v%d, 2, v%d" % (adr, adr))
        tags = [None, None]

        self.sm_sums = sums

        def fmas(ts):
            # the chains of the tiles in `ts` side by side: a chain is 16 DEPENDENT FMAs, and three of them interleaved still ran at
            # ~10 cycles per instruction (one wave per SIMD: nobody else fills the result latency); six run at the issue rate
            for t in ts:
                self.wait_lgkm(tag_lwr[t])
            for r in ([] if self.softmax else range(16)):
                for t in ts:
                    for k, (u, bi, blk, inst) in enumerate(blocks):
                        a = self.acc_reg(u["accs"][(bi, t)])
                        if r == 0:
                            e("v_fma_f32 v%d, v%d, v%d, 0" % (sums[t][k], lwr_reg(t, 0), a))
                        else:
                            e("v_fmac_f32 v%d, v%d, v%d" % (sums[t][k], lwr_reg(t, r), a + r))
            for t in ts:
                tags[t] = [self.lgkm_op("ds_bpermute_b32 v%d, v%d, v%d" % (oth[t][k], adr, sums[t][k])) for k in range(nb)]

        def stores(t):
            for k in range(nb):                     # the sums under the FULL exec mask, then the masked stores
                self.wait_lgkm(tags[t][k])
                e("v_add_f32 v%d, v%d, v%d" % (oth[t][k], sums[t][k], oth[t][k]))
            for k, (u, bi, blk, inst) in enumerate(blocks):
                e("s_mov_b64 exec, s[%d:%d]" % (S_MSK + 2 * k, S_MSK + 2 * k + 1))
                base = (S_REC_I if inst else S_REC_T) + 2 * t
                self.vm_op("global_store_dword v%d, v%d, s[%d:%d] offset:%d" % (V_LB4, oth[t][k], base, base + 1, 4 + 128 * blk))
            e("s_mov_b64 exec, -1")
        self.stamp(len(self.units) + 4)
        if self.softmax:
            self.tail_softmax(blocks, lwr_reg, tag_lwr)
        fmas((0, 1))
        self.stamp(len(self.units) + 5)
        stores(0)
        stores(1)
        for u in self.logit_units:
            self.acc_release(list(u["accs"].values()))
        self.acc_release(self.lwr_acc)
        self.lwr_acc = None
        self.logit_units = []

    def queue_inputs_early(self):
        """side work from the first unit behind the skip layer on (gamma(x) of this group is dead): the next group's inputs, its
        point, gamma(x), and |d| from the per-ray table.  Temporaries and inputs live in the g area (free until views' first pack)."""
        def which():
            # g2 = grp + n_wg < n_groups ? grp + n_wg : grp
            with self.atomic():
                self.e("s_add_u32 s%d, s%d, s%d" % (S_GRP2, S_GRP, S_NWG))
                self.e("s_cmp_lt_i32 s%d, s%d" % (S_GRP2, S_NGRP))
                self.e("s_cselect_b32 s%d, s%d, s%d" % (S_GRP2, S_GRP2, S_GRP))
        self.q(which)
        tags = {}
        for t in range(2):
            self.q(lambda t=t: tags.__setitem__(t, self.fetch_tile(t, S_GRP2)))
        for t in range(2):
            self.q(lambda t=t: self.wait_vm(tags[t]))      # (deferred: the holder is filled when the load is emitted)
            for fn in self.encode_tile(t, "x"):
                self.q(fn)

    PARK = (3, 6, 7, 0)             # what of V_IN outlives gamma(x): the per-ray table address, z, z_next, |d|

    def park(self):
        """views' packs of tile 1 land on V_IN: its six live values per tile wait in an idle accumulator until the rgb / sigma unit"""
        self.park_acc = self.acc_take(1)[0]
        for t in range(2):
            for i, k in enumerate(Gen.PARK):
                self.e("v_mov_b32 v%d, v%d" % (self.acc_reg(self.park_acc) + len(Gen.PARK) * t + i, V_IN + 8 * t + k))

    def unpark(self):
        for t in range(2):
            for i, k in enumerate(Gen.PARK):
                self.e("v_mov_b32 v%d, v%d" % (V_IN + 8 * t + k, self.acc_reg(self.park_acc) + len(Gen.PARK) * t + i))
        self.acc_release([self.park_acc])
        self.park_acc = None

    def queue_inputs_late(self):
        """behind the rgb / sigma unit (gamma(d) of this group is dead): gamma(d) of the next group -- since the per-ray table two
        16-byte loads per tile; before it ~250 instructions of division, sincos and packing per tile.  (Round 6 tried the skip layer's
        one-block units of the SAME group instead -- the emptiest gaps of the loop: bit-identical, and no faster: the skip layer's units
        grew by what the head units shrank, profiles/r06/r06f.  What the kernel pays for is the NUMBER of non-MFMA instructions, not
        where they stand.)"""
        for t in range(2):
            for fn in self.encode_tile(t, "d"):
                self.q(fn, low=True)

    # ------------------------------------------------------------------ trace builds (k_mlp_tt_*_trace): s_memtime per unit
    def stamp(self, idx):
        """lane idx of V_TRACE := low word of s_memtime here (written one stamp later: the scalar load has returned by then); the
        clock output of a trace build is the 64 stamps of workgroup 0's first wave in its LAST group"""
        if not self.trace:
            return
        pair = S_CLK0 + 2 * (self.nstamp & 1)
        prev = S_CLK0 + 2 * ((self.nstamp + 1) & 1)
        if self.last_stamp is not None:
            self.o.append("\tv_writelane_b32 v%d, s%d, %d" % (V_TRACE, prev, self.last_stamp))
        self.o.append("\ts_memtime s[%d:%d]" % (pair, pair + 1))
        self.last_stamp = idx
        self.nstamp += 1
        if idx == len(self.units) + 3:
            # the group's end also goes to lane 56 + (group counter & 7): the durations of the last eight groups
            skip = self.label()
            self.o += ["\ts_waitcnt lgkmcnt(0)", "\ts_and_b32 s%d, s%d, 7" % (S_T0, S_NDONE), "\ts_add_u32 s%d, s%d, 56" % (S_T0, S_T0),
                       "\ts_mov_b32 m0, s%d" % S_T0, "\ts_nop 1",
                       "\tv_writelane_b32 v%d, s%d, m0" % (V_TRACE, pair),
                       # every 32nd group's end (groups 0, 32, .., 160) to lanes 48..53: the average group time per window
                       "\ts_and_b32 s%d, s%d, 31" % (S_T0, S_NDONE), "\ts_cmp_eq_u32 s%d, 0" % S_T0, "\ts_cbranch_scc0 %s" % skip,
                       "\ts_lshr_b32 s%d, s%d, 5" % (S_T0, S_NDONE), "\ts_add_u32 s%d, s%d, 48" % (S_T0, S_T0), "\ts_mov_b32 m0, s%d" % S_T0,
                       "\ts_nop 1", "\tv_writelane_b32 v%d, s%d, m0" % (V_TRACE, pair), skip + ":",
                       "\ts_add_u32 s%d, s%d, 1" % (S_NDONE, S_NDONE)]

    # ------------------------------------------------------------------ group boundary
    def prefetch_first_unit(self):
        """bias of unit 0 into fresh accumulators + the ring's first three fragments (the only LGKM operations in flight at a
        group's start)"""
        u0 = self.units[0]
        for plan in self.arm_plan(u0):
            for op in plan:
                op()
        for g in range(P - 1):
            sl, of = self.stream[g]
            self.ring_tags[g % P] = self.lgkm_op("ds_read_b128 %s, v%d offset:%d" % (vr(V_RING + 4 * (g % P), 4), V_FRAG + sl, of))

    def advance_group_state(self):
        """the prefetched group becomes the current one: z, z_next, |d| and the masks"""
        e = self.e
        for t in range(2):
            vi = V_IN + 8 * t
            e("v_mov_b32 v%d, v%d" % (V_ZZ + t, vi + 6))
            e("v_mov_b32 v%d, v%d" % (V_ZN + t, vi + 7))
            e("v_mov_b32 v%d, v%d" % (V_DN + t, vi + 0))
            e("s_mov_b64 s[%d:%d], s[%d:%d]" % (S_VALID + 2 * t, S_VALID + 2 * t + 1, S_NVALID + 2 * t, S_NVALID + 2 * t + 1))
            e("s_mov_b64 s[%d:%d], s[%d:%d]" % (S_LAST + 2 * t, S_LAST + 2 * t + 1, S_NLAST + 2 * t, S_NLAST + 2 * t + 1))

    def group_body(self):
        self.m0 = None
        assert self.acc_free == [i for i in range(8) if i not in self.units[0]["accs"].values()], self.acc_free
        self.last_stamp = None
        for ui in range(len(self.units)):
            self.emit_unit(ui)
        self.stamp(len(self.units))
        self.drain_side()                               # whatever the last units could not cover
        self.tail_logits()
        self.stamp(len(self.units) + 1)
        assert self.acc_free == list(range(8)), self.acc_free
        self.e("s_waitcnt lgkmcnt(0)")
        self.lgkm.drain()
        self.advance_group_state()
        self.stamp(len(self.units) + 2)
        if self.trace:
            self.o.append("\ts_waitcnt lgkmcnt(0)")
            self.stamp(len(self.units) + 3)

    # ------------------------------------------------------------------ the kernel
    def kernel(self):
        e, name = self.e, self.name
        self.o += ["\t.text", "\t.globl\t%s" % name, "\t.p2align\t8", "\t.type\t%s,@function" % name, "%s:" % name]
        for dst, off, n in ((S_IMG, 0x0, 2), (S_RAYS, 0x8, 2), (S_Z, 0x10, 2), (S_S, 0x18, 2), (S_MAGIC, 0x20, 2), (S_NGRP, 0x28, 2),
                            (S_REC, 0x30, 2), (S_RECF, 0x38, 1), (S_PS, 0x40, 2), (S_NSEM, 0x48, 2), (S_CLK, 0x50, 2), (S_AUX, 0x58, 2)):
            e("s_load_dword%s %s, %s, 0x%x" % ("x2" if n == 2 else "", sr(dst, n), sr(S_KARG), off))
        # wave id from v0 itself (never written): a v_readfirstlane of a register that is re-used a few instructions later was
        # observed to return the LATER value while scalar-load data was returning (tools/probe/gen_two_tile_asm.py)
        e("v_readfirstlane_b32 s%d, v0" % S_WAVE)
        e("s_nop 4")
        e("s_lshr_b32 s%d, s%d, 6" % (S_WAVE, S_WAVE))
        e("s_lshl_b32 s%d, s%d, 12" % (S_W4K, S_WAVE))                    # wave * 4 KiB
        e("v_and_b32 v%d, 63, v0" % V_T0)
        e("v_lshlrev_b32 v%d, 4, v%d" % (V_LANE16, V_T0))
        e("v_lshrrev_b32 v%d, 5, v0" % V_LB4)
        e("v_and_b32 v%d, 1, v%d" % (V_LB4, V_LB4))
        e("v_lshlrev_b32 v%d, 4, v%d" % (V_LB4, V_LB4))                  # hi * 16
        for sl in range(NSLOT):
            self.lit(S_T0, sl * SLOT)
            e("v_add_u32 v%d, s%d, v%d" % (V_FRAG + sl, S_T0, V_LANE16))
            e("v_add_u32 v%d, s%d, v%d" % (V_BIAS + sl, S_T0, V_LB4))
        for k in range(3):
            e("v_add_u32 v%d, s%d, v%d" % (V_DMA + k, S_W4K, V_LANE16))
            if k:
                e("v_add_u32 v%d, 0x%x, v%d" % (V_DMA + k, 16384 * k, V_DMA + k))
        e("v_and_b32 v%d, 31, v0" % V_LB4)
        e("v_lshlrev_b32 v%d, 2, v%d" % (V_LB4, V_LB4))
        e("s_mov_b32 s%d, -1" % S_LO32)
        e("s_mov_b32 s%d, 0" % (S_LO32 + 1))
        e("s_mov_b32 s%d, 1" % S_N0)
        e("s_mov_b32 s%d, 1" % (S_N0 + 1))
        e("s_mov_b32 s%d, -1" % S_HI0)
        e("s_mov_b32 s%d, 0" % (S_HI0 + 1))
        e("s_lshr_b32 s%d, s%d, 4" % (S_LWW, S_W4K))                      # wave * 256: this wave's [2 tiles][32] local-weight table
        e("s_add_u32 s%d, s%d, 0x%x" % (S_LWW, S_LWW, LW_BASE))
        e("s_sub_u32 s%d, s%d, 0x%x" % (S_LWR, S_LWW, 0))          # + V_BIAS[0] (= slot 0's base + 16 hi) = table + 16 hi
        e("s_waitcnt lgkmcnt(0)")
        # store masks of the logit blocks (constant): channel = 32 blk + (lane & 31) < n_out, lanes 0..31 only
        for k, (blk, inst) in enumerate(self.logit_blocks()):
            e("v_and_b32 v%d, 31, v0" % V_T0)
            if blk:
                e("v_add_u32 v%d, %d, v%d" % (V_T0, 32 * blk, V_T0))
            e("v_cmp_gt_i32 vcc, s%d, v%d" % (S_NINST if inst else S_NSEM, V_T0))
            e("s_and_b64 s[%d:%d], vcc, s[%d:%d]" % (S_MSK + 2 * k, S_MSK + 2 * k + 1, S_HI0, S_HI0 + 1))
        if self.softmax:
            # ALL lanes (both halves) whose channel of the head's last block exists: 32 (blocks - 1) + (lane & 31) < n_out
            for k, (nblk, sreg) in enumerate(((self.nbs, S_NSEM), (self.nbi, S_NINST))):
                if nblk:
                    e("v_and_b32 v%d, 31, v0" % V_T0)
                    if nblk > 1:
                        e("v_add_u32 v%d, %d, v%d" % (V_T0, 32 * (nblk - 1), V_T0))
                    e("v_cmp_gt_i32 s[%d:%d], s%d, v%d" % (S_VMSK + 2 * k, S_VMSK + 2 * k + 1, sreg, V_T0))
        lend, lloop, lfin = self.label(), self.label(), self.label()
        e("s_mov_b32 s%d, s%d" % (S_GRP, S_WG))
        e("s_cmp_ge_i32 s%d, s%d" % (S_GRP, S_NGRP))
        e("s_cbranch_scc1 %s" % lend)
        # chunks 0, 1, 2 -> slots 0, 1, 2
        for c in range(3):
            for j in range(tt_plan.pieces_of(self.chunks, c)):
                self.issue_piece(c, j)
        e("s_waitcnt vmcnt(0)")
        self.vm.drain()
        e("s_barrier")
        # the first group's inputs and encodings (exposed, once per workgroup)
        e("s_mov_b32 s%d, s%d" % (S_GRP2, S_GRP))
        tags = [self.fetch_tile(t, S_GRP2) for t in range(2)]
        for t in range(2):
            self.wait_vm(tags[t])
            for part in ("x", "d"):
                for fn in self.encode_tile(t, part):
                    fn()
        self.advance_group_state()
        if not self.trace:
            e("s_memtime s[%d:%d]" % (S_CLK0, S_CLK0 + 1))
            e("s_memrealtime s[%d:%d]" % (S_CLK0 + 2, S_CLK0 + 3))
        else:
            e("v_mov_b32 v%d, 0" % V_TRACE)
            e("s_mov_b32 s%d, 0" % S_NDONE)
            e("s_memtime %s" % sr(S_WGCLK))                                  # the workgroup's start
            e("s_waitcnt lgkmcnt(0)")
        e("s_waitcnt lgkmcnt(0)")
        self.lgkm.drain()
        self.prefetch_first_unit()
        # pass 1 (discarded): brings the counters to their steady state at the loop's head
        keep = self.o
        self.o = []
        self.group_body()
        self.prefetch_first_unit()
        self.o = keep
        # pass 2: the loop body
        self.o.append(lloop + ":")
        self.group_body()
        e("s_add_u32 s%d, s%d, s%d" % (S_GRP, S_GRP, S_NWG))
        e("s_cmp_ge_i32 s%d, s%d" % (S_GRP, S_NGRP))
        e("s_cbranch_scc1 %s" % lend)
        self.prefetch_first_unit()
        e("s_branch %s" % lloop)
        self.o.append(lend + ":")
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e("s_cmp_eq_u64 s[%d:%d], 0" % (S_CLK, S_CLK + 1))
        e("s_cbranch_scc1 %s" % lfin)
        if self.trace:              # every workgroup: cycles of its first wave from start to end -> clk[64 + workgroup]
            lw = self.label()
            e("s_cmp_lg_u32 s%d, 0" % S_WAVE)
            e("s_cbranch_scc1 %s" % lw)
            e("s_memtime s[%d:%d]" % (S_CLK0, S_CLK0 + 1))
            e("s_waitcnt lgkmcnt(0)")
            e("s_sub_u32 s%d, s%d, s%d" % (S_CLK0, S_CLK0, S_WGCLK))
            e("s_lshl_b32 s%d, s%d, 2" % (S_T0, S_WG))
            e("s_add_u32 s%d, s%d, 256" % (S_T0, S_T0))
            e("v_mov_b32 v%d, s%d" % (V_T0, S_T0))
            e("v_mov_b32 v%d, s%d" % (V_T1, S_CLK0))
            e("s_mov_b64 exec, 1")
            e("global_store_dword v%d, v%d, s[%d:%d]" % (V_T0, V_T1, S_CLK, S_CLK + 1))
            e("s_mov_b64 exec, -1")
            e("s_waitcnt vmcnt(0)")
            self.o.append(lw + ":")
        e("s_cmp_lg_u32 s%d, 0" % S_WG)
        e("s_cbranch_scc1 %s" % lfin)
        if self.trace:
            e("s_cmp_lg_u32 s%d, 0" % S_WAVE)
            e("s_cbranch_scc1 %s" % lfin)
            e("v_and_b32 v%d, 63, v0" % V_T0)
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_T0, V_T0))
            e("global_store_dword v%d, v%d, s[%d:%d]" % (V_T0, V_TRACE, S_CLK, S_CLK + 1))
            e("s_waitcnt vmcnt(0)")
            e("s_branch %s" % lfin)
        e("s_memtime s[%d:%d]" % (S_T0, S_T0 + 1))
        e("s_memrealtime s[%d:%d]" % (S_SAVE, S_SAVE + 1))
        e("s_waitcnt lgkmcnt(0)")
        e("s_sub_u32 s%d, s%d, s%d" % (S_T0, S_T0, S_CLK0))
        e("s_subb_u32 s%d, s%d, s%d" % (S_T1, S_T1, S_CLK0 + 1))
        e("s_sub_u32 s%d, s%d, s%d" % (S_SAVE, S_SAVE, S_CLK0 + 2))
        e("s_subb_u32 s%d, s%d, s%d" % (S_SAVE + 1, S_SAVE + 1, S_CLK0 + 3))
        e("v_cmp_eq_u32 vcc, 0, v0")
        e("s_and_saveexec_b64 s[%d:%d], vcc" % (S_VALID, S_VALID + 1))
        e("s_cbranch_execz %s" % lfin)
        e("v_mov_b32 v%d, s%d" % (V_CLKOUT, S_T0))
        e("v_mov_b32 v%d, s%d" % (V_CLKOUT + 1, S_T1))
        e("v_mov_b32 v%d, s%d" % (V_CLKOUT + 2, S_SAVE))
        e("v_mov_b32 v%d, s%d" % (V_CLKOUT + 3, S_SAVE + 1))
        e("v_mov_b32 v%d, 0" % V_T0)
        e("global_store_dwordx4 v%d, %s, s[%d:%d]" % (V_T0, vr(V_CLKOUT, 4), S_CLK, S_CLK + 1))
        e("s_waitcnt vmcnt(0)")
        self.o.append(lfin + ":")
        e("s_endpgm")
        self.o += [".Lend_%s:" % name, "\t.size\t%s, .Lend_%s-%s" % (name, name, name), ""]
        self.o += ["\t.rodata", "\t.p2align\t6", "\t.amdhsa_kernel %s" % name,
                   "\t\t.amdhsa_group_segment_fixed_size %d" % (NSLOT * SLOT + 1024),
                   "\t\t.amdhsa_private_segment_fixed_size 0", "\t\t.amdhsa_kernarg_size %d" % KERNARG_BYTES, "\t\t.amdhsa_user_sgpr_count 2",
                   "\t\t.amdhsa_user_sgpr_kernarg_segment_ptr 1", "\t\t.amdhsa_system_sgpr_workgroup_id_x 1",
                   "\t\t.amdhsa_system_vgpr_workitem_id 0", "\t\t.amdhsa_next_free_vgpr 512", "\t\t.amdhsa_next_free_sgpr %d" % NEXT_FREE_SGPR,
                   "\t\t.amdhsa_accum_offset 256", "\t\t.amdhsa_reserve_vcc 1", "\t\t.amdhsa_float_denorm_mode_32 3",
                   "\t\t.amdhsa_float_denorm_mode_16_64 3", "\t\t.amdhsa_dx10_clamp 1", "\t\t.amdhsa_ieee_mode 1",
                   "\t.end_amdhsa_kernel", ""]
        return "\n".join(self.o)


KERNARG_BYTES = 104


def metadata(names):
    o = ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for n in names:
        o += ["  - .agpr_count:     256", "    .args:", "      - .offset:         0", "        .size:           %d" % KERNARG_BYTES,
              "        .value_kind:     by_value", "    .group_segment_fixed_size: %d" % (NSLOT * SLOT + 1024),
              "    .kernarg_segment_align: 8", "    .kernarg_segment_size: %d" % KERNARG_BYTES, "    .max_flat_workgroup_size: 256",
              "    .name:           %s" % n, "    .private_segment_fixed_size: 0", "    .sgpr_count:     108",
              "    .sgpr_spill_count: 0", "    .symbol:         %s.kd" % n, "    .uniform_work_group_size: 1",
              "    .uses_dynamic_stack: false", "    .vgpr_count:     512", "    .vgpr_spill_count: 0", "    .wavefront_size: 64"]
    o += ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "amdhsa.version:", "  - 1", "  - 2", "...", "\t.end_amdgpu_metadata", ""]
    return "\n".join(o)


def variant_name(tap, depth, sm, nbs, nbi):
    tag = ("f" if tap else "") + ("d1" if depth == 1 else "") + ("sm" if sm else "")
    return "k_mlp_tt_%ss%di%d" % (tag + "_" if tag else "", nbs, nbi)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "/dev/stdout"
    parts = ['\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"', "\t.amdhsa_code_object_version 5", ""]
    names = []
    for nbs, nbi in ((1, 1), (2, 1), (0, 0), (1, 0), (2, 0), (3, 0)):
        n = "k_mlp_tt_s%di%d" % (nbs, nbi)
        names.append(n)
        parts.append(Gen(nbs, nbi, n).kernel())
    # the variants of the networks WITH heads: head_tap (f) x head_depth 1 (d1) x softmax compositing (sm): k_mlp_tt[_f][_d1][sm]... as
    # variant_name() spells them (pnr_mlp_tt.cpp builds the same names)
    for tap in (0, 1):
        for depth in (2, 1):
            for sm in (False, True):
                if (tap, depth, sm) == (0, 2, False):
                    continue
                for nbs, nbi in ((1, 1), (2, 1), (1, 0), (2, 0), (3, 0)):
                    n = variant_name(tap, depth, sm, nbs, nbi)
                    names.append(n)
                    parts.append(Gen(nbs, nbi, n, depth=depth, softmax=sm, tap=tap).kernel())
    # diagnostics builds only (make EXTRA_TT=trace | abl): the production library carries no kernel that writes (64 + n_wg) * 4 bytes
    # to the clock buffer (a 16-byte clk_probe buffer under PNR_MLP_TRACE was an out-of-bounds device write)
    extra = sys.argv[3] if len(sys.argv) > 3 else ""
    if extra in ("trace", "abl"):
        names.append("k_mlp_tt_s2i1_trace")     # debug: per-unit s_memtime stamps instead of the clock pair (tools/tt_trace.py)
        parts.append(Gen(2, 1, "k_mlp_tt_s2i1_trace", trace=True).kernel())
    if extra == "abl":                          # timing-only ablations of the trace build (results invalid)
        for abl in (1, 2, 3, 4, 7):
            names.append("k_mlp_tt_s2i1_trace_a%d" % abl)
            parts.append(Gen(2, 1, names[-1], trace=True, abl=abl).kernel())
    unit_names = ["%s %s" % (g.layers[u["layer"]]["name"], u["blocks"]) for g in [Gen(2, 1, "x")] for u in g.units]
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write("\n".join(unit_names) + "\n")
    parts.append(metadata(names))
    with open(out, "w") as f:
        f.write("\n".join(parts))


if __name__ == "__main__":
    main()
