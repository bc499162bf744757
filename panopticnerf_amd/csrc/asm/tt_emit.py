"""How the text and the wait counts of k_mlp_tt are produced (gen_mlp_tt.py) -- nothing here knows the MLP.

Emitter.o is the list of finished lines.  Instructions go through e(); labels, directives and the trace stamps, which are only
ever written from the main stream, are appended to o directly.

Side work is written as closures; when one is taken off the queue it runs in CAPTURE mode: plain instructions become strings
in the outbox, operations the counters must see (LGKM and vector-memory operations, waits, accumulator releases) become
deferred calls that run when the outbox entry is actually emitted -- so the counters see every operation in PROGRAM order."""
from contextlib import contextmanager


class Sim:
    """in-order counters: every issued operation is appended; wait(tag) = "at most N outstanding" with N = the CERTAIN operations
    issued after `tag` (operations some waves skip do not count: conservative)."""
    def __init__(self, name, cap):
        self.name, self.cap, self.q, self.n = name, cap, [], 0

    def push(self, certain=True):
        self.n += 1
        self.q.append((self.n, certain))
        return self.n

    def wait_count(self, tag):
        if tag is None or not any(t == tag for t, _ in self.q):
            return None                         # already covered by an earlier wait
        idx = [t for t, _ in self.q].index(tag)
        n = sum(1 for _, c in self.q[idx + 1:] if c)
        n = min(n, self.cap)
        # everything up to tag is known complete once the wait passes -- but only if counts were exact; drop them anyway: a later
        # wait on an older tag returns None (covered)
        self.q = self.q[idx + 1:]
        return n

    def drain(self):
        self.q = []

    def state(self):
        return [c for _, c in self.q]


class Holder:
    """the tag of a counted operation: v is filled when the operation is actually emitted"""
    def __init__(self, v=None):
        self.v = v


class Emitter:
    def __init__(self, name):
        self.name = name
        self.o = []
        self.nlabel = 0
        self.lgkm = Sim("lgkm", 15)
        self.vm = Sim("vm", 63)
        self.side, self.side_lo, self.outbox, self.capture = [], [], [], None

    def e(self, s):
        if self.capture is not None:
            self.capture.append("\t" + s)
        else:
            self.o.append("\t" + s)

    def defer(self, fn):
        if self.capture is not None:
            self.capture.append(fn)
        else:
            fn()

    @contextmanager
    def atomic(self):
        """side-work instructions that must not be separated by main-stream instructions: a changed EXEC mask (the MFMA stream's
        LDS reads, packs and LDS-DMA pieces must run on all lanes) or a dependence on SCC (the pieces' s_add_u32 clobbers it)"""
        if self.capture is None:
            yield
            return
        outer, self.capture = self.capture, []
        try:
            yield
        finally:
            grp, self.capture = self.capture, outer
            outer.append(grp)

    def label(self):
        self.nlabel += 1
        return ".L%s_%d" % (self.name, self.nlabel)

    def lgkm_op(self, instr):
        """an operation lgkmcnt counts: the LDS reads, ds_bpermute, and the ds_write_b32 of the local-weight table"""
        h = Holder()

        def now():
            self.o.append("\t" + instr)
            h.v = self.lgkm.push()
        self.defer(now)
        return h

    def vm_op(self, instr, certain=True):
        h = Holder()

        def now():
            self.o.append("\t" + instr)
            h.v = self.vm.push(certain)
        self.defer(now)
        return h

    def wait_lgkm(self, h):
        def now():
            n = self.lgkm.wait_count(h.v)
            if n is not None:
                self.o.append("\ts_waitcnt lgkmcnt(%d)" % n)
        if h is not None:
            self.defer(now)

    def wait_vm(self, h):
        def now():
            n = self.vm.wait_count(h.v)
            if n is not None:
                self.o.append("\ts_waitcnt vmcnt(%d)" % n)
        if h is not None:
            self.defer(now)

    def lit(self, sreg, val):
        """s_mov of a 32-bit literal (VOP3 instructions cannot carry one on gfx9)"""
        self.e("s_mov_b32 s%d, 0x%x" % (sreg, val & 0xffffffff))

    def q(self, fn, low=False):
        """queue side work; low: work that holds no accumulator (the encoders) -- it waits for everything else"""
        (self.side_lo if low else self.side).append(fn)

    def side_busy(self):
        return bool(self.side or self.side_lo or self.outbox)

    def drain_side(self, budget=None):
        """emit queued side work: all of it (budget None) or `budget` instructions"""
        spent = 0
        while self.side_busy() and (budget is None or spent < budget):
            if not self.outbox:
                fn = self.side.pop(0) if self.side else self.side_lo.pop(0)
                self.capture = []
                fn()
                self.outbox, self.capture = self.capture, None
                continue
            x = self.outbox.pop(0)
            for y in (x if isinstance(x, list) else [x]):
                if callable(y):
                    y()
                else:
                    self.o.append(y)
                spent += 1
