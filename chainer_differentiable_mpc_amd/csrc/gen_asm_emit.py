"""What the stream generators (gen_lqr_asm.py, gen_mpc_fwd_asm.py) share: the instruction emitter with its hazard
tracker, the VGPR allocator and the few instruction sequences both spell the same way.  Reads no environment.

Hazards (hipcc pads nothing inside asm) are tracked by the emitter: VALU write -> DPP read of the same VGPR needs
two wait states; a transcendental's result needs one before a non-trans VALU reads it (gfx940 forwarding hazard;
two are kept); s_mov m0 -> LDS-DMA needs one.  Labels reset the tracker pessimistically.
"""
import contextlib

VBASE = 128   # first VGPR owned by the asm block (operands chosen by hipcc live below)


def mask64(lanes):
    """the 64-bit exec mask that selects `lanes` (0..15) in each of the four 16-lane rows, as its 32-bit half"""
    m16 = sum(1 << l for l in lanes)
    return m16 | (m16 << 16)


def vrange(regs):
    a, b = int(regs[0][1:]), int(regs[-1][1:])
    assert b - a + 1 == len(regs)
    return "v[%d:%d]" % (a, b)


def v2(pair):
    a = int(pair[0][1:])
    return "v[%d:%d]" % (a, a + 1)


def sgpr_lo(pair):
    """number of the first register of an SGPR pair "s[lo:hi]" """
    return int(pair[2:pair.index(":")])


class LabelCounter:
    """numbers for the labels of sequences that are emitted more than once"""

    def __init__(self):
        self.n = 0

    def next(self):
        self.n += 1
        return self.n


class Regs:
    def __init__(self, base):
        self.next = base

    def take(self, n=1, align=1):
        while self.next % align:
            self.next += 1
        r = list(range(self.next, self.next + n))
        self.next += n
        return ["v%d" % i for i in r]


class Prog:
    """instruction emitter with a small hazard tracker (ages are in wait states since the VALU write).
    mfma_use: wait states kept before a non-accumulating use of an MFMA result; mfma_dep: before an accumulation into
    the same tile.  A label resets the MFMA table too, so every instruction behind a label keeps mfma_use wait states
    to it whether the stream has a matrix instruction or not."""

    def __init__(self, mfma_use, mfma_dep):
        self.mfma_use, self.mfma_dep = mfma_use, mfma_dep
        self.lines = []
        self.age = {}       # vgpr -> wait states since a VALU wrote it
        self.trans = {}     # vgpr -> wait states since a transcendental wrote it
        self.mf = {}        # vgpr -> wait states since an MFMA wrote it
        self.n_instr = 0

    def fresh(self):
        """an empty emitter with the same wait-state counts"""
        return Prog(self.mfma_use, self.mfma_dep)

    def scratch(self):
        """an empty emitter in the same hazard state: to emit into, count and throw away"""
        p = self.fresh()
        p.age, p.trans, p.mf = dict(self.age), dict(self.trans), dict(self.mf)
        return p

    def _tick(self, n=1):
        for d in (self.age, self.trans, self.mf):
            for r in list(d):
                d[r] += n
                if d[r] > 12:
                    del d[r]

    def raw(self, text, ticks=1):
        self.lines.append(text)
        self.n_instr += 1
        self._tick(ticks)

    def nop(self, n):      # n wait states
        if n > 0:
            self.raw("s_nop %d" % (n - 1), ticks=n)

    def comment(self, text):
        self.lines.append("; " + text)

    def align(self, log2):
        self.lines.append(".p2align %d" % log2)

    def append(self, other):
        """the instructions of another emitter, as they are"""
        self.lines += other.lines
        self.n_instr += other.n_instr

    def label(self, name, reset=True):
        self.lines.append(name + ":")
        if reset:  # anything may have been written right before a jump here
            self.age = {"*": 0}
            self.trans = {"*": 0}
            self.mf = {"*": 0}

    def exec_written(self):
        # SALU write of EXEC -> DPP: not a documented hazard (the documented one is a VALU write, 5 wait states);
        # two wait states are kept anyway
        self.age = {"*": 0}

    def _need(self, table, reg, states):
        have = table.get(reg, table.get("*", 99))
        if have < states:
            self.nop(states - have)

    def mfma(self, dst, a, b, c, abid):
        """v_mfma_f32_4x4x1_16b_f32 dst[4], a, b, c[4] | 0, A broadcast from block `abid` of each 16-lane row.
        Wait states kept: mfma_use (5; the ISA asks passes + 2 = 4 for this 2-pass, non-XDL op) before anything
        but an accumulating MFMA reads an MFMA result, mfma_dep (2 = passes) before a dependent accumulation, 2 after
        a VALU write of any source.  GEN_MFMA_USE=4 / 8 give bit-identical results (scripts/asm_variant_check.sh)."""
        for r in (a, b):
            self._need(self.age, r, 2)
            self._need(self.trans, r, 2)
            self._need(self.mf, r, self.mfma_use)
        if c:
            for r in c:
                self._need(self.age, r, 2)
                self._need(self.mf, r, self.mfma_dep)
        self.raw("v_mfma_f32_4x4x1_16b_f32 %s, %s, %s, %s cbsz:2 abid:%d" % (vrange(dst), a, b, vrange(c) if c else "0", abid))
        for r in dst:
            self.mf[r] = 0

    def uses(self, regs):
        """a non-VALU instruction (LDS / memory) is about to read or overwrite these VGPRs"""
        for r in regs:
            self._need(self.mf, r, self.mfma_use)

    def v(self, text, writes=(), reads=(), dpp=None, trans=False):
        """a VALU instruction: `dpp` is the VGPR it reads through DPP, `trans` marks a transcendental"""
        for r in tuple(reads) + tuple(writes) + ((dpp,) if dpp else ()):
            self._need(self.mf, r, self.mfma_use)
        if dpp is not None:
            self._need(self.age, dpp, 2)
        for r in tuple(reads) + ((dpp,) if dpp else ()):
            if not trans:
                self._need(self.trans, r, 2)
        self.raw(text)
        for w in writes:
            self.age[w] = 0
            if trans:
                self.trans[w] = 0
            else:
                self.trans.pop(w, None)

    # ---- instruction helpers ------------------------------------------------------------------------------
    def fmac_dpp(self, acc, a, b, lane):
        self.v("v_fmac_f32_dpp %s, %s, %s row_newbcast:%d row_mask:0xf bank_mask:0xf" % (acc, a, b, lane),
               writes=(acc,), reads=(b, acc), dpp=a)

    def mul_dpp(self, dst, a, b, lane):
        self.v("v_mul_f32_dpp %s, %s, %s row_newbcast:%d row_mask:0xf bank_mask:0xf" % (dst, a, b, lane),
               writes=(dst,), reads=(b,), dpp=a)

    def mov_dpp(self, dst, a, lane):
        self.v("v_mov_b32_dpp %s, %s row_newbcast:%d row_mask:0xf bank_mask:0xf" % (dst, a, lane),
               writes=(dst,), dpp=a)

    # ---- sequences both generators use ----------------------------------------------------------------------
    def load_mask(self, pair, lanes):
        """the exec mask of `lanes` in every 16-lane row into the SGPR pair `pair`"""
        lo, val = sgpr_lo(pair), mask64(lanes) & 0xffffffff
        self.raw("s_mov_b32 s%d, 0x%x" % (lo, val))
        self.raw("s_mov_b32 s%d, 0x%x" % (lo + 1, val))

    def exec_all(self):
        """every lane on again after a stretch under an exec mask"""
        self.raw("s_mov_b64 exec, -1")
        self.exec_written()

    @contextlib.contextmanager
    def under_exec(self, mask):
        """what the body emits runs under the exec mask `mask`; every lane is on again behind it"""
        self.raw("s_mov_b64 exec, " + mask)
        yield
        self.exec_all()

    def store_part(self, part, store):
        """the store instruction `store` for the first `part` of a group of 64 chunks, one per lane: under a partial
        exec mask when there are fewer than 64 (32 or fewer: a 32-bit literal, zero-extended)"""
        if part <= 32:
            self.raw("s_mov_b64 exec, 0x%x" % ((1 << part) - 1))
        elif part < 64:
            self.raw("s_mov_b32 exec_hi, 0x%x" % ((1 << (part - 32)) - 1))
        self.raw(store)
        if part < 64:
            self.exec_all()

    def text(self):
        return self.lines
