"""Register and LDS map of k_mlp_tt (gen_mlp_tt.py): the names the generator formats into its instructions, one table of every
range the kernel uses, and the list of overlaps that are meant.  check() runs at import: two ranges of one register file that
intersect must be a declared overlap (and a declared overlap must intersect), and no range passes the top of its file.

Accumulators lent out as homes (Gen.g2_acc, park_acc, lwr_acc) are dynamic -- taken and released through Gen.acc_take /
acc_release inside V_ACC -- and are not in the table."""

NSLOT, SLOT = 4, 33 * 1024              # chunk c in LDS slot c % 4 at (c % 4) * SLOT: other strides / slot orders +-0 (profiles/r05/r05t, r05v)
P = 4                                   # fragment ring (quads)
D, SKIP = 8, 4
LW_BASE = NSLOT * SLOT                  # [4 waves][2 tiles][32 floats] behind the weight slots (1 KiB)

# ---- VGPR map
V_TID, V_LANE16, V_FRAG, V_BIAS, V_T0, V_DMA, V_LB4, V_TRACE = 0, 1, 2, 6, 10, 11, 14, 15
# V_DMA + m: lane * 16 + wave * 4 KiB + m * 16 KiB: the LDS-DMA pieces' address offsets.  A wave copies the fragments
# 16 m + 4 wave + i (i < 4: the instruction's immediate offset i KiB) of a chunk -- runs of four, round-robin over the waves.
V_T1 = 1    # second pack temporary (lane * 16 is only needed to build the bases): one temporary for consecutive packs let the
            # v_accvgpr_write of a pack see the NEXT pack's value (measured: records differed)
V_T2 = 15                               # third pack temporary (V_TRACE's register: trace builds keep the plain pack form)
V_RING, V_ACC = 16, 32                  # ring: v[16:31]; accumulators 0..7: v[32 + 16 i : +16]
V_CLKOUT = 20                           # v[20:23]: the clock quadruple of a plain build's last store (the kernel's end: the ring is idle)
V_EX, V_ED = 160, 192                   # gamma(x) [2 tiles][16], gamma(d) [2][8]
V_G = 208                               # g blocks 0, 1 of both tiles [2][16]  (views' first two blocks; the other two live in A0)
V_ZZ, V_ZN, V_DN, V_LW = 240, 242, 244, 246      # [2] each: per-tile compositing state of the CURRENT group
V_IN = 224                              # next group's inputs [2][8]: ox oy oz dx dy dz zz zn   (v[224:239])
V_TMP = 208                             # encoder / epilogue temporaries share the g area once g is dead: v[208:223]
V_PTMP = 248                            # 8 more temporaries v[248:255]
V_AUXA = V_PTMP + 6                     # [2 tiles]: the lane's address in the per-ray table between the fetch of a tile and its point (v[254:255])
V_LWA = V_IN + 2                        # address of the local-weight table reads in a group's last unit (the next group's o_z: dead since its point)
V_SMX = V_IN + 10                       # v[234:237]: temporaries of tail_softmax's xor-16 steps: the next group's o_z and q of tile 1 (dead: its
                                        # gamma(d) is encoded) -- NOT the logits tail's sums / oth registers (V_IN + 1..5, 9)
# ---- AGPR map: two activation arrays of [2 tiles][64]
A0, A1 = 0, 128
# ---- SGPR map
S_KARG, S_WG = 0, 2                     # as the dispatch leaves them: s[0:1] the kernel-argument segment, s2 the workgroup id
S_IMG, S_RAYS, S_Z, S_S, S_N, S_MAGIC, S_SHIFT, S_NGRP, S_NWG, S_REC, S_RECF, S_PS, S_NSEM, S_NINST, S_CLK = 4, 6, 8, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 23, 24
S_WAVE, S_W4K, S_GRP, S_PIECE, S_T0, S_T1 = 26, 27, 28, 30, 34, 35
S_VALID, S_LAST = 36, 40                # [2 tiles] x 64-bit masks of the CURRENT group: s[36:39], s[40:43]
S_NVALID, S_NLAST = 44, 48              # the same of the NEXT group (filled at fetch time): s[44:47], s[48:51]
S_LO32, S_N0, S_HI0 = 52, 54, 56        # constants: lanes 0..31, lanes {0, 32}, lanes with hi == 0 (= lanes 0..31)
S_SAVE, S_REC_T = 58, 60                # saved exec; the two tiles' record pointers s[60:61], s[62:63]
S_MSK = 64                              # store masks of the (up to) three logit blocks: s[64:69] = lanes with hi == 0 and channel < n_out
S_REC_I = 70                            # the two tiles' record pointers + 4 n_sem (the instance columns): s[70:73]
S_AUX = 82                              # s[82:83]: the per-ray table k_ray_aux wrote (gamma(d) of both half-waves and |d|: 128 B per ray)
S_VMSK = 76                             # softmax kernels: s[76:77] / s[78:79] = ALL lanes whose channel of the semantic / instance head's last block exists
S_LWW, S_LWR = 74, 75                   # LDS addresses of this wave's local-weight table: + 4 (lane & 31) to write, + (V_BIAS[0] = slot 0 + 16 hi) to read
S_WGCLK = 90                            # s[90:91]: trace builds: the workgroup's start clock
S_CLK0 = 96                             # s[96:99] clocks at start
S_K = 100                               # s100: literal constants that VOP3 cannot carry
S_NDONE = 101                           # s101: trace builds: the groups this workgroup has finished
S_Q = 19                                # the tile's Q (v_readlane) between the scan and its store
S_GRP2 = 29                             # the group whose inputs are being prefetched

NEXT_FREE_SGPR = 102                    # .amdhsa_next_free_sgpr
TOPS = {"v": 256, "a": 256, "s": NEXT_FREE_SGPR}

# (file, name, first, count) of every range the kernel uses
RANGES = [
    ("v", "V_TID", V_TID, 1), ("v", "V_LANE16", V_LANE16, 1), ("v", "V_T1", V_T1, 1), ("v", "V_FRAG", V_FRAG, NSLOT),
    ("v", "V_BIAS", V_BIAS, NSLOT), ("v", "V_T0", V_T0, 1), ("v", "V_DMA", V_DMA, 3), ("v", "V_LB4", V_LB4, 1),
    ("v", "V_TRACE", V_TRACE, 1), ("v", "V_T2", V_T2, 1), ("v", "V_RING", V_RING, 4 * P), ("v", "V_CLKOUT", V_CLKOUT, 4),
    ("v", "V_ACC", V_ACC, 8 * 16), ("v", "V_EX", V_EX, 2 * 16), ("v", "V_ED", V_ED, 2 * 8), ("v", "V_G", V_G, 2 * 16),
    ("v", "V_TMP", V_TMP, 16), ("v", "V_IN", V_IN, 2 * 8), ("v", "V_LWA", V_LWA, 1), ("v", "V_SMX", V_SMX, 4),
    ("v", "V_ZZ", V_ZZ, 2), ("v", "V_ZN", V_ZN, 2), ("v", "V_DN", V_DN, 2), ("v", "V_LW", V_LW, 2),
    ("v", "V_PTMP", V_PTMP, 8), ("v", "V_AUXA", V_AUXA, 2),
    ("a", "A0", A0, 2 * 64), ("a", "A1", A1, 2 * 64),
    ("s", "S_KARG", S_KARG, 2), ("s", "S_WG", S_WG, 1), ("s", "S_IMG", S_IMG, 2), ("s", "S_RAYS", S_RAYS, 2), ("s", "S_Z", S_Z, 2),
    ("s", "S_S", S_S, 1), ("s", "S_N", S_N, 1), ("s", "S_MAGIC", S_MAGIC, 1), ("s", "S_SHIFT", S_SHIFT, 1), ("s", "S_NGRP", S_NGRP, 1),
    ("s", "S_NWG", S_NWG, 1), ("s", "S_REC", S_REC, 2), ("s", "S_RECF", S_RECF, 1), ("s", "S_Q", S_Q, 1), ("s", "S_PS", S_PS, 2),
    ("s", "S_NSEM", S_NSEM, 1), ("s", "S_NINST", S_NINST, 1), ("s", "S_CLK", S_CLK, 2), ("s", "S_WAVE", S_WAVE, 1),
    ("s", "S_W4K", S_W4K, 1), ("s", "S_GRP", S_GRP, 1), ("s", "S_GRP2", S_GRP2, 1), ("s", "S_PIECE", S_PIECE, 2),
    ("s", "S_T0", S_T0, 1), ("s", "S_T1", S_T1, 1), ("s", "S_VALID", S_VALID, 4), ("s", "S_LAST", S_LAST, 4),
    ("s", "S_NVALID", S_NVALID, 4), ("s", "S_NLAST", S_NLAST, 4), ("s", "S_LO32", S_LO32, 2), ("s", "S_N0", S_N0, 2),
    ("s", "S_HI0", S_HI0, 2), ("s", "S_SAVE", S_SAVE, 2), ("s", "S_REC_T", S_REC_T, 4), ("s", "S_MSK", S_MSK, 6),
    ("s", "S_REC_I", S_REC_I, 4), ("s", "S_LWW", S_LWW, 1), ("s", "S_LWR", S_LWR, 1), ("s", "S_VMSK", S_VMSK, 4),
    ("s", "S_AUX", S_AUX, 2), ("s", "S_WGCLK", S_WGCLK, 2), ("s", "S_CLK0", S_CLK0, 4), ("s", "S_K", S_K, 1),
    ("s", "S_NDONE", S_NDONE, 1),
]

# the overlaps that are meant: (name, name, why both can live there)
OVERLAPS = [
    ("V_LANE16", "V_T1", "lane * 16 is only needed to build the bases in the prologue; the packs start behind it"),
    ("V_TRACE", "V_T2", "trace builds keep the plain pack form, which has no third temporary"),
    ("V_RING", "V_CLKOUT", "the clock store is the kernel's last: the fragment ring is idle"),
    ("V_G", "V_TMP", "encoder / epilogue temporaries share the g area once g is dead"),
    ("V_G", "V_IN", "views' packs of tile 1 land on the next group's inputs: what of them is live waits in an accumulator (Gen.park)"),
    ("V_G", "V_LWA", "inside V_IN; g is dead since the rgb / sigma unit"),
    ("V_G", "V_SMX", "inside V_IN; g is dead since the rgb / sigma unit"),
    ("V_IN", "V_LWA", "the next group's o_z: dead since its point"),
    ("V_IN", "V_SMX", "the next group's o_z and q of tile 1: dead once its gamma(d) is encoded"),
    ("V_PTMP", "V_AUXA", "the table address lives between the fetch of a tile and its point; the temporaries below it go on being used"),
]


def check(ranges=RANGES, overlaps=OVERLAPS, tops=TOPS):
    """raise ValueError unless the table is sound: names unique, every range inside its file, every intersection declared in
    `overlaps`, every declared overlap an intersection"""
    names = [n for _, n, _, _ in ranges]
    if len(set(names)) != len(names):
        raise ValueError("register table: a name appears twice")
    for f, n, lo, cnt in ranges:
        if not (cnt >= 1 and 0 <= lo and lo + cnt <= tops[f]):
            raise ValueError("register table: %s = %s[%d:%d] leaves its file (top %d)" % (n, f, lo, lo + cnt - 1, tops[f]))
    meant = {frozenset(o[:2]) for o in overlaps}
    found = set()
    for i, (f, n, lo, cnt) in enumerate(ranges):
        for f2, n2, lo2, cnt2 in ranges[i + 1:]:
            if f == f2 and lo < lo2 + cnt2 and lo2 < lo + cnt:
                found.add(frozenset((n, n2)))
    for pair in sorted(sorted(p) for p in found - meant):
        raise ValueError("register table: %s and %s overlap and are not declared" % tuple(pair))
    for pair in sorted(sorted(p) for p in meant - found):
        raise ValueError("register table: declared overlap %s / %s does not exist" % tuple(pair))


check()
