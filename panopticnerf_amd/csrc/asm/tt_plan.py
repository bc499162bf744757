"""The chunk plan of k_mlp_tt (gen_mlp_tt.py) and what follows from it alone: the MFMA units of a group, a unit's fragments, the
LDS-DMA pieces of a chunk.  Functions of (nbs, nbi, depth); mirrors pnr_build_plan, plan 2 (pnr_mlp_plan.h) -- tests/test_pack.py
holds the two against each other."""
from tt_regs import D, NSLOT, SKIP


def build_plan(nbs, nbi, depth):
    """-> (layers, chunks) of the network with nbs semantic and nbi instance logit blocks and head_depth `depth`"""
    L = []

    def add(name, nblk, segs, fbc, mode):
        nks = sum(n for _, n in segs)
        if fbc * nks + 1 > 33:
            fbc = 1
        L.append(dict(name=name, nblk=nblk, segs=segs, nks=nks, fbc=fbc, mode=mode))
    for i in range(D):
        if i == 0:
            add("L0", 8, [("ex", 4)], 8, "relu")
        elif i - 1 == SKIP:
            add("L%d" % i, 8, [("ex", 4), ("h", 16)], 2, "relu")
        else:
            add("L%d" % i, 8, [("h", 16)], 2, "relu")
    add("feature", 8, [("h", 16)], 2, "linear")
    add("views", 4, [("F", 16), ("ed", 2)], 2, "relu")
    add("rgbs", 1, [("g", 8), ("hh", 16)], 1, "rgbs")
    # heads: sem0 | inst0 | sem1 | inst1 -- a logit layer never follows its own hidden layer directly (the hidden layer's last
    # blocks would have to be packed inside the logit unit's first MFMA gaps), sem1's reduction runs beside inst1
    if depth == 1:                  # one Linear per head: the logit layers read h itself (16 k-steps)
        if nbs:
            add("sem1", nbs, [("tap", 16)], nbs, "logits")
        if nbi:
            add("inst1", 1, [("tap", 16)], 1, "logits")
    else:
        if nbs:
            add("sem0", 4, [("tap", 16)], 2, "relu")
        if nbi:
            add("inst0", 4, [("tap", 16)], 2, "relu")
        if nbs:
            add("sem1", nbs, [("shs", 8)], nbs, "logits")
        if nbi:
            add("inst1", 1, [("shi", 8)], 1, "logits")
    chunks = []
    off = 0
    for li, l in enumerate(L):
        for fb in range(0, l["nblk"], l["fbc"]):
            nfrag = l["fbc"] * l["nks"] + 1
            chunks.append(dict(layer=li, fb=fb, nfb=l["fbc"], off=off, nfrag=nfrag))
            off += nfrag
    # slot = chunk % 4 is static, so a group is a multiple of four chunks: geometries whose image has 42 (no heads) or 45 (no
    # instance head) chunks get DUMMY chunks at the group's end -- one piece of image fragment 0 into the slot, a hand-over,
    # no unit.  The image itself is unchanged (pnr_build_plan knows nothing of them)
    while len(chunks) % NSLOT:
        chunks.append(dict(layer=None, fb=0, nfb=0, off=0, nfrag=1, dummy=True))
    assert len(chunks) % NSLOT == 0, len(chunks)
    assert max(c["nfrag"] for c in chunks) <= 33
    return L, chunks


def build_units(layers, chunks):
    """the MFMA stream of one group: list of units, each = (chunk, layer, blocks, ...)"""
    U = []
    for ci, c in enumerate(chunks):
        if c.get("dummy"):
            continue
        l = layers[c["layer"]]
        step = 2 if l["mode"] != "logits" else min(c["nfb"], 2)        # (a third semantic block, nbs = 3: units [0, 1] and [2])
        if l["name"] == "rgbs":
            step = 1
        blocks = list(range(c["fb"], c["fb"] + c["nfb"]))
        first = True
        for i in range(0, len(blocks), step):
            U.append(dict(chunk=ci, layer=c["layer"], blocks=blocks[i:i + step], first_of_chunk=first,
                          last_of_chunk=(i + step >= len(blocks))))
            first = False
    return U


def unit_frags(layers, chunks, u):
    """fragments of a unit in consumption order: (lds slot, byte offset in slot, ks, b index in unit)"""
    c = chunks[u["chunk"]]
    l = layers[u["layer"]]
    out = []
    for ks in range(l["nks"]):
        for bi, blk in enumerate(u["blocks"]):
            out.append((u["chunk"] % NSLOT, ((blk - c["fb"]) * l["nks"] + ks) * 1024, ks, bi))
    return out


def seg_of_ks(layer, ks):
    for seg, n in layer["segs"]:
        if ks < n:
            return seg, ks
        ks -= n
    raise IndexError


def piece_list(chunks, chunk):
    """(m, i, waves) of the LDS-DMA pieces of a chunk: fragment 16 m + 4 wave + i, issued by waves 0 .. waves - 1"""
    n = chunks[chunk]["nfrag"]
    out = []
    for m in range((n + 15) // 16):
        for i in range(4):
            nw = max(0, min(4, -(-(n - 16 * m - i) // 4)))
            if nw:
                out.append((m, i, nw))
    return out


def pieces_of(chunks, chunk):
    return len(piece_list(chunks, chunk))
