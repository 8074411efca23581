"""The fused LQR solve as an instruction stream, second half: the rollout behind the backward sweep of an LqrStream
(gen_lqr_stream.py).  Three schedules, kept apart on purpose - they differ in what is prepared how far ahead:

  * RingRollout: F and f come back from HBM through the forward ring (a loop over the ring's slots);
  * StashRollout: F comes back from the stash registers, unrolled over the horizon, entered through a table of stubs;
  * AdjRollout: the stash schedule that also computes the co-states and writes dC, dc, dF, df (the one-pass gradient).

They share what is literally the same: reading a step's rows, the step's FMAs and store, the jump into a stub table.
"""
from gen_asm_emit import VBASE, sgpr_lo, vrange
from gen_lqr_stream import BSTUB, S_HI, S_JMP, S_N, S_RET, S_SM, S_TF, S_TMP, S_UM, S_XM


class Rollout:
    def __init__(self, st):
        self.st = st

    def read_rows(self, c, a, aff_too=True):
        st = self.st
        if st.K.no_ldsread and st.in_loop:
            return
        P, ns, Mc = st.P, st.ns, st.M[c]
        if ns % 2 == 0:
            i = 0
            while i + 4 <= ns:
                P.raw("ds_read2_b64 %s, %%[arow] offset0:%d offset1:%d" % (vrange(Mc[i:i + 4]), i // 2, i // 2 + 1))
                i += 4
            if i < ns:
                P.raw("ds_read_b64 %s, %%[arow] offset:%d" % (vrange(Mc[i:i + 2]), i * 4))
        else:
            i = 0
            while i + 2 <= ns:
                P.raw("ds_read2_b32 %s, %%[arow] offset0:%d offset1:%d" % (vrange(Mc[i:i + 2]), i, i + 1))
                i += 2
            if i < ns:
                P.raw("ds_read_b32 %s, %%[arow] offset:%d" % (Mc[i], i * 4))
        if aff_too:
            P.raw("ds_read_b32 %s, %%[aaff]" % st.ACC[a])

    def fcompute(self, c, a, ap, mask, last, fillers=()):
        """fillers: independent work emitted in the wait states between the dependent control FMAs"""
        st = self.st
        P, nx, nu, M, ACC = st.P, st.nx, st.nu, st.M, st.ACC
        fillers = list(fillers)
        skip = st.K.fwd_skip if st.in_loop else set()
        for jj in range(nx):                       # u_t = K_t x_t + k_t (lanes nx+m) ; f_t + Fx x_t (lanes < nx)
            if "xpart" not in skip:
                P.fmac_dpp(ACC[a], ACC[ap], M[c][jj], jj)
        if not last:
            for m in range(nu):                    # x_{t+1} += Fu u_t : the gain rows hold 0 in these columns
                if fillers:
                    fillers.pop(0)()
                if "upart" not in skip:
                    P.fmac_dpp(ACC[a], ACC[a], M[c][nx + m], nx + m)
        for f in fillers:
            f()
        if st.adj:        # d_tau leaves as dc, through the staging area
            return
        if "store" not in skip:
            with P.under_exec(mask):
                P.raw("global_store_dword %%[pst], %s, off" % ACC[a])
        if not last and "pst" not in skip:
            P.v("v_lshl_add_u64 %[pst], %[pst], 0, %[dst]")

    def begin(self):
        st = self.st
        P = st.P
        P.comment("---- forward rollout")
        st.stamp(2)
        P.raw("s_waitcnt vmcnt(0) lgkmcnt(0)")
        P.v("v_mov_b32_e32 %[xvout], 0")
        P.raw("v_readfirstlane_b32 %s, %%[bwd_only]" % S_TMP)   # (a VGPR operand: hipcc ran out of SGPRs for an "s" one at (1,1))
        P.raw("s_cmp_lg_u32 %s, 0" % S_TMP)                    # LqrRecursion.backward(): gains only
        P.raw("s_cbranch_scc1 Ldone_%=")
        if not st.adj:
            with P.under_exec(S_XM):                           # x_0 = x_init
                P.raw("global_store_dword %%[px0], %s, off" % st.XV0)

    def entry_jump(self, fstub):
        """jump to entry (T-1) - 1 of the stub table at Lfstub, `fstub` bytes per stub"""
        P = self.st.P
        lo = sgpr_lo(S_JMP)
        P.raw("s_getpc_b64 " + S_JMP)
        P.label("Lpcf_%=", reset=False)
        P.raw("s_sub_i32 %s, %%[T], 2" % S_TMP)                 # entry stub index: (T-1) - 1
        P.raw("s_mul_i32 %s, %s, %d" % (S_TMP, S_TMP, fstub))
        P.raw("s_add_u32 s%d, s%d, Lfstub_%%=-Lpcf_%%=" % (lo, lo))
        P.raw("s_addc_u32 s%d, s%d, 0" % (lo + 1, lo + 1))
        P.raw("s_add_u32 s%d, s%d, %s" % (lo, lo, S_TMP))
        P.raw("s_addc_u32 s%d, s%d, 0" % (lo + 1, lo + 1))
        P.raw("s_setpc_b64 " + S_JMP)


class RingRollout(Rollout):
    def __init__(self, st):
        Rollout.__init__(self, st)
        self.rare = []      # ghbm: out-of-line tails of the pointer steps

    def advance_f(self):
        """the forward DMA pointers go one timestep on.  ghbm: the gain rows have a slice T-1, F and f have not - the
        last step moves the gain lanes alone (`fstrl`: their stride, 0 in the F / f lanes); it lives out of line, the
        common path is the same four instructions"""
        st = self.st
        P = st.P
        if not st.ghbm:
            st.advance(st.fptr, st.fstr)
            return
        n_ = st.labels.next()
        lab_r, lab_b = "Lfrare%d_%%=" % n_, "Lfback%d_%%=" % n_
        P.raw("s_cmp_gt_i32 %s, 1" % S_TF)
        P.raw("s_cbranch_scc0 " + lab_r)
        for p_, s_ in zip(st.fptr, st.fstr):
            P.v("v_lshl_add_u64 %s, %s, 0, %s" % (p_, p_, s_))
        P.raw("s_sub_i32 %s, %s, 1" % (S_TF, S_TF))
        P.label(lab_b, reset=False)
        self.rare.append((lab_r, lab_b))

    def rare_tails(self):
        st = self.st
        P = st.P
        for lab_r, lab_b in self.rare:       # (reached by their branches only)
            P.label(lab_r, reset=False)
            P.raw("s_cmp_eq_i32 %s, 1" % S_TF)
            P.raw("s_cbranch_scc0 " + lab_b)
            for q_, p_ in enumerate(st.fptr):
                P.v("v_lshl_add_u64 %s, %s, 0, %%[fstrl%d]" % (p_, p_, q_))
            P.raw("s_sub_i32 %s, %s, 1" % (S_TF, S_TF))
            P.raw("s_branch " + lab_b)

    def emit(self):
        st = self.st
        P, L, ACC, DF = st.P, st.L, st.ACC, st.L.DF
        P.raw("s_sub_i32 %s, %%[T], %d" % (S_TF, 1 if st.ghbm else 2))
        for j in range(DF):
            st.issue_group(st.fptr, j, L.SLOT_F)
            self.advance_f()
        P.raw("s_waitcnt vmcnt(%d)" % ((DF - 1) * L.ndma_f))
        self.read_rows(0, 0)
        P.v("v_mov_b32_e32 %s, %s" % (ACC[2], st.XV0), writes=(ACC[2],))
        P.raw("s_sub_i32 %s, %%[T], 1" % S_N)      # full steps t = 0 .. T-2
        P.raw("s_cmp_lg_u32 %s, 0" % S_N)
        P.raw("s_cbranch_scc0 Lfin0_%=")
        if st.K.skip_fwd:
            P.raw("s_branch Lfin0_%=")
        st.in_loop = True
        P.label("Lfwd_%=")
        n_fwd0 = P.n_instr
        for j in range(DF):
            c, a = j % 2, j % 3
            o, an, ap = 1 - c, (a + 1) % 3, (a + 2) % 3
            P.comment("---- forward step, slot %d" % j)
            P.raw("s_waitcnt lgkmcnt(0)")
            st.issue_group(st.fptr, j, L.SLOT_F)
            self.advance_f()
            st.vmwait((DF - 1) * L.ndma_f)
            d = "2" if j == DF - 1 else ""
            P.v("v_add_u32_e32 %%[arow], %%[drow%s], %%[arow]" % d)
            P.v("v_add_u32_e32 %%[aaff], %%[daff%s], %%[aaff]" % d)
            self.read_rows(o, an)
            self.fcompute(c, a, ap, S_SM, False)
            P.raw("s_sub_i32 %s, %s, 1" % (S_N, S_N))
            P.raw("s_cmp_lg_u32 %s, 0" % S_N)
            if j < DF - 1:
                P.raw("s_cbranch_scc0 Lfin%d_%%=" % (j + 1))
            else:
                P.raw("s_cbranch_scc1 Lfwd_%=")
                P.raw("s_branch Lfin0_%=")
        st.n_fwd, st.n_fwd_steps = P.n_instr - n_fwd0, DF
        st.in_loop = False
        for j in range(DF):                            # t = T-1: only u_{T-1}
            c, a = j % 2, j % 3
            ap = (a + 2) % 3
            P.label("Lfin%d_%%=" % j)
            P.raw("s_waitcnt lgkmcnt(0)")
            self.fcompute(c, a, ap, S_UM, True)
            P.v("v_mov_b32_e32 %%[xvout], %s" % ACC[a])
            P.raw("s_branch Ldone_%=")
        self.rare_tails()


class StashRollout(Rollout):
    """F comes back from the stash registers through two staging buffers in the (now idle) ring: the code is
    unrolled over n = T-1-t (the stash slot is a register NUMBER), entered at n = T-1 through a table of
    entry stubs, and runs down to n = 1 without any loop control; n = 0 is the u-only step t = T-1.
    Rows are prepared TWO steps ahead (three row sets, four accumulators): a step is only ~25 instructions,
    shorter than the LDS round trip stash -> staging -> rows."""

    @staticmethod
    def sets(n):
        return n % 3, n % 4, (n + 1) % 4     # row set, accumulator, x_t register of step n

    def prefetch_a(self, m, move=True):
        """first half of the preparation of step m (>= 0): F_t rows out of the stash registers (lanes < 8 get
        columns [0, H) directly and columns [H, ns) from lane + 8 by a row rotation), row pointers moved"""
        st = self.st
        P, L = st.P, st.L
        Mc = st.M[self.sets(m)[0]]
        if m >= 1 and not ("stage" in st.K.fwd_skip and st.in_loop):
            regs = [r for p in range(len(L.stash_pieces)) for r in st.stash_regs_of(p, m - 1)]
            for jj in range(L.H):
                P.v("v_accvgpr_read_b32 %s, a%d" % (Mc[jj], regs[jj]), writes=(Mc[jj],))
            for jj in range(L.H):
                if L.H + jj < st.ns:
                    P.v("v_mov_b32_dpp %s, %s row_ror:8 row_mask:0xf bank_mask:0xf" % (Mc[L.H + jj], Mc[jj]),
                        writes=(Mc[L.H + jj],), dpp=Mc[jj])
        if move:   # the gain-row / f pointers go from step m+1 to step m
            P.v("v_add_u32_e32 %[arow], %[drowo], %[arow]")
            P.v("v_add_u32_e32 %[aaff], %[daff], %[aaff]")

    def prefetch_b(self, m):
        """second half: the gain rows of step m into lanes nx..15 of the same registers (AFTER the VALU writes
        above - a later VALU write would clobber them), then f_t / k_t into the accumulator of step m"""
        st = self.st
        c, a, _ = self.sets(m)
        if "read" in st.K.fwd_skip and st.in_loop:
            return
        with st.P.under_exec(S_HI):
            self.read_rows(c, a, aff_too=False)
        st.P.raw("ds_read_b32 %s, %%[aaff]" % st.ACC[a])

    def prefetch(self, m, move=True):
        """stage + read the rows of step m (>= 0); returns the number of LDS operations issued"""
        P = self.st.P
        before = len(P.lines)
        self.prefetch_a(m, move)
        self.prefetch_b(m)
        return sum(1 for ln in P.lines[before:] if ln.startswith("ds_"))

    def group_size(self, m):
        """LDS operations of prefetch(m): emitted into a scratch copy of the emitter and counted"""
        if m < 0:
            return 0
        st = self.st
        with st.emitting(st.P.scratch()) as scratch:
            k = self.prefetch(m)
        # the MFMA ages alone run on through the counted instructions: behind the step's label they are what spares
        # its first FMAs the post-label padding, and the pinned streams have it so
        st.P.mf = scratch.mf
        return k

    def emit(self):
        st = self.st
        P, L, ACC = st.P, st.L, st.ACC
        fstub = 64
        while fstub < 8 * (2 * (2 * L.H + st.ns // 2 + 6) + 4):
            fstub *= 2
        self.entry_jump(fstub)
        n_fwd0 = P.n_instr
        st.in_loop = True
        for n in range(L.NSTASH, 0, -1):
            c, a, ap = self.sets(n)
            P.label("Lfs%d_%%=" % n)
            P.raw("s_waitcnt lgkmcnt(%d)" % self.group_size(n - 1))   # rows of step n are in; those of n-1 may be in flight
            fill = []
            if n >= 2:
                fill = [lambda m=n - 2: self.prefetch_a(m), lambda m=n - 2: self.prefetch_b(m)]
                if st.nu == 1:
                    fill = [lambda m=n - 2: self.prefetch(m)]
            self.fcompute(c, a, ap, S_SM, False, fill)
        st.n_fwd, st.n_fwd_steps = P.n_instr - n_fwd0, L.NSTASH
        st.in_loop = False
        c, a, ap = self.sets(0)
        P.raw("s_waitcnt lgkmcnt(0)")
        self.fcompute(c, a, ap, S_UM, True)
        P.v("v_mov_b32_e32 %%[xvout], %s" % ACC[a])
        P.raw("s_branch Ldone_%=")
        # ---- entry stubs: stage F of the first two steps, read their rows, place x_init
        P.align(fstub.bit_length() - 1)
        P.label("Lfstub_%=")
        for n in range(1, L.NSTASH + 1):
            c, a, ap = self.sets(n)
            P.align(fstub.bit_length() - 1)
            self.prefetch(n, move=False)
            self.prefetch(n - 1)
            P.v("v_mov_b32_e32 %s, %s" % (ACC[ap], st.XV0), writes=(ACC[ap],))
            P.raw("s_branch Lfs%d_%%=" % n)


class AdjRollout(StashRollout):
    """The one-pass gradient's forward sweep.  Step n (time t = T-1-n) rolls d_tau out as the stash rollout does and, with
    [V | v | x | u] of time t+1 from the ring,
      lambda_{t+1} = V_{t+1} x_{t+1} + v_{t+1}        d_lambda_{t+1} = V_{t+1} dx_{t+1} + v'_{t+1}
      dC_t = wa dtau (x) tau + wb tau (x) dtau   dc_t = dtau   dF_t = d_lambda_{t+1} (x) tau + lambda_{t+1} (x) dtau
      df_t = d_lambda_t (the reference's index, differentiable_lqr.py:133) or d_lambda_{t+1} (strict)
    (differentiable_lqr.py:128-134; wa = 0.5, wb = 1 reproduce :128's precedence).  Rows are columns-per-lane
    registers (lane j = column j), written to the staging area under the mask of the tau lanes and sent to
    HBM as the contiguous 16-byte chunks they form there: [dC | dc | dF | df] of the wave's four trajectories."""
    DFA = 4                                     # ring slots of [Vv | x | u]
    S_DFSEL = "s[86:87]"

    def __init__(self, st):
        StashRollout.__init__(self, st)
        nx, nu, ns, L, DFA = st.nx, st.nu, st.ns, st.L, self.DFA
        nVv, nX, nU = nx * (nx + 1), nx, nu         # 16-byte chunks per wave-step
        self.nda = (nVv + nX + nU + 63) // 64
        self.SLOTA = self.nda * 1024
        self.STG = DFA * self.SLOTA                 # staging area, byte offset in the ring
        self.nout = L.nchunk_b                      # [dC | dc | dF | df]: ns^2 + ns + nx ns + nx chunks
        self.nst = (self.nout + 63) // 64
        assert self.STG + 16 * self.nout <= L.RING and (DFA - 1) * self.nda + 4 * self.nst <= 63
        self.O_dc, self.O_dF, self.O_df = 16 * ns * ns, 16 * (ns * ns + ns), 16 * (ns * ns + ns + nx * ns)
        fixed = set(r_ for grp in st.M for r_ in grp) | set(st.ACC) | {st.MINPIV, st.XV0} | set(st.TS)
        self.pool = ["v%d" % i for i in range(VBASE, 256) if "v%d" % i not in fixed]
        take = self.take
        self.VR = [take(nx, align=2) for _ in range(2)]  # row min(lane, nx-1) of V of the step two ahead / one ahead
        self.LN = take(2)                                # v -> lambda_{t+1}
        self.DLN = take(3)                               # v' -> d_lambda: accumulating, current (df), being loaded
        self.TAUR = take(3)
        self.DTAU, self.HDT, self.WT, self.DFV = take(4)
        self.RC = take(ns)
        self.RFm = take(nx)
        self.SD = [take(4, align=4) for _ in range(self.nst)]

    def take(self, k, align=1):
        """k consecutive registers of those the rollout does not keep from the backward sweep"""
        pool = self.pool
        for st in range(len(pool)):
            blk = pool[st:st + k]
            if len(blk) == k and int(blk[0][1:]) % align == 0 and int(blk[-1][1:]) - int(blk[0][1:]) == k - 1:
                del pool[st:st + k]
                return blk
        raise AssertionError("out of forward registers")

    def load_data(self, m):
        """LDS reads of [V | v | tau] of step m from its ring slot (v' comes with prefetch_b) - issued two steps
        ahead of their use, behind the counted wait for the slot's DMA group"""
        P, nx, DFA = self.st.P, self.st.nx, self.DFA
        off = (m % DFA) * self.SLOTA
        Vs = self.VR[m % 2]
        av = "%%[avr%d]" % (m % DFA)           # (ds_read2_b32 reaches 1 KB: one row address per slot)
        for j in range(0, nx - 1, 2):
            P.raw("ds_read2_b32 %s, %s offset0:%d offset1:%d" % (vrange(Vs[j:j + 2]), av, j, j + 1))
        if nx % 2:
            P.raw("ds_read_b32 %s, %s offset:%d" % (Vs[nx - 1], av, (nx - 1) * 4))
        P.raw("ds_read_b32 %s, %s offset:%d" % (self.LN[m % 2], av, nx * 4))
        P.raw("ds_read_b32 %s, %%[atx] offset:%d" % (self.TAUR[m % 3], off))

    def issue_data(self, m):
        """LDS-DMA group of step m (time T-1-m; the pointers walk forward in time) into slot m % DFA"""
        if m < 0:
            return
        st = self.st
        st.issue_group(st.fptr[:self.nda], m % self.DFA, self.SLOTA)
        for q in range(self.nda):
            st.P.v("v_lshl_add_u64 %s, %s, 0, %s" % (st.fptr[q], st.fptr[q], st.fstr[q]))

    def adj_prefetch_b(self, m):
        """gain rows of step m into lanes nx..15, k_t into the accumulator (f = 0 in its state lanes), v'_t"""
        P, ACC = self.st.P, self.st.ACC
        c, a, _ = self.sets(m)
        P.v("v_mov_b32_e32 %s, 0" % ACC[a], writes=(ACC[a],))
        P.raw("ds_read_b32 %s, %%[aaff]" % self.DLN[m % 3])
        with P.under_exec(S_HI):
            self.read_rows(c, a, aff_too=False)
            P.raw("ds_read_b32 %s, %%[aaff]" % ACC[a])

    def outputs(self, n, last):
        """everything of step n after its rollout"""
        st = self.st
        P, nx, ns, ACC = st.P, st.nx, st.ns, st.ACC
        VR, LN, DLN, DTAU, HDT, WT, DFV, RC, RFm, SD, STG = self.VR, self.LN, self.DLN, self.DTAU, self.HDT, self.WT, self.DFV, self.RC, self.RFm, self.SD, self.STG
        c, a, ap = self.sets(n)
        TAU = self.TAUR[n % 3]
        P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (DTAU, ACC[a], ACC[ap], S_XM), writes=(DTAU,), reads=(ACC[a], ACC[ap]))
        P.v("v_mul_f32_e32 %s, %%[wa], %s" % (HDT, DTAU), writes=(HDT,), reads=(DTAU,))
        P.v("v_mul_f32_e32 %s, %%[wb], %s" % (WT, TAU), writes=(WT,), reads=(TAU,))
        if not last:      # d_lambda_{t+1} += V_{t+1} dx_{t+1}
            Vs, dl = VR[(n - 1) % 2], DLN[(n - 1) % 3]
            for j in range(nx):
                P.fmac_dpp(dl, ACC[a], Vs[j], j)
        for i in range(ns):
            P.mul_dpp(RC[i], HDT, TAU, i)
        for i in range(ns):
            P.fmac_dpp(RC[i], WT, DTAU, i)
        if not last:
            ln, dl = LN[(n - 1) % 2], DLN[(n - 1) % 3]
            for i in range(nx):
                P.mul_dpp(RFm[i], dl, TAU, i)
            for i in range(nx):
                P.fmac_dpp(RFm[i], ln, DTAU, i)
            P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (DFV, DLN[n % 3], dl, self.S_DFSEL), writes=(DFV,), reads=(DLN[n % 3], dl))
        P.raw("s_mov_b64 exec, " + S_SM)
        for i in range(ns):
            P.raw("ds_write_b32 %%[awc], %s offset:%d" % (RC[i], STG + i * ns * 4))
        P.raw("ds_write_b32 %%[awe], %s offset:%d" % (DTAU, STG + self.O_dc))
        if not last:
            for i in range(nx):
                P.raw("ds_write_b32 %%[awf], %s offset:%d" % (RFm[i], STG + self.O_dF + i * ns * 4))
            P.raw("s_mov_b64 exec, " + S_XM)
            P.raw("ds_write_b32 %%[awd], %s offset:%d" % (DFV, STG + self.O_df))
        P.exec_all()
        # the first n_valid chunks of the staging area -> HBM, then the store pointers move on one timestep
        n_valid = self.nout if not last else ns * ns + ns
        nq = (n_valid + 63) // 64
        for q in range(nq):
            P.raw("ds_read_b128 %s, %%[ach] offset:%d" % (vrange(SD[q]), STG + q * 1024))
        P.raw("s_waitcnt lgkmcnt(0)")
        if not last and n - 2 - self.DFA >= 0:
            self.issue_data(n - 2 - self.DFA)       # the slot read at the top of this step is free (the wait above)
        P.uses([r_ for q in range(nq) for r_ in SD[q]])
        for q in range(nq):
            P.store_part(n_valid - 64 * q, "global_store_dwordx4 %%[pso%d], %s, off" % (q, vrange(SD[q])))
        if not last:
            for q in range(self.nst):
                P.v("v_lshl_add_u64 %%[pso%d], %%[pso%d], 0, %%[sso%d]" % (q, q, q))

    def data_wait(self, n):
        """counted wait for the DMA group of step n-2 at the top of step n: younger are the groups of the steps in
        between that exist, and the stores of the DFA steps since it was issued"""
        younger = len([m for m in range(n - 1 - self.DFA, n - 2) if m >= 0])
        self.st.P.raw("s_waitcnt vmcnt(%d)" % (younger * self.nda + self.DFA * self.nst))

    def emit_stub(self, n):
        """entry at step n = T-1 (time 0): the first DFA groups, everything landed once (the only exposed round
        trip), tau_0, d_lambda_0 = v'_0 = dx_init, the data of time 1, the rows of the first two steps; then the
        next two groups - and, so that the counted waits of the first steps see as many younger stores as later
        ones do, dx_init stored 2 nst + 1 times instead of once"""
        P, ACC, DFA = self.st.P, self.st.ACC, self.DFA
        c, a, ap = self.sets(n)
        for m in range(n, n - DFA, -1):
            self.issue_data(m)
        P.raw("s_waitcnt vmcnt(0)")
        self.prefetch_a(n, move=False)
        self.adj_prefetch_b(n)
        P.raw("ds_read_b32 %s, %%[atx] offset:%d" % (self.TAUR[n % 3], (n % DFA) * self.SLOTA))
        self.prefetch_a(n - 1)
        self.adj_prefetch_b(n - 1)
        self.load_data(n - 1)
        P.v("v_mov_b32_e32 %s, 0" % ACC[ap], writes=(ACC[ap],))       # dx_0 = 0
        P.raw("s_waitcnt lgkmcnt(0)")
        self.issue_data(n - DFA)
        self.issue_data(n - DFA - 1)
        with P.under_exec(S_XM):
            for _ in range(2 * self.nst + 1):
                P.raw("global_store_dword %%[px0], %s, off" % self.DLN[n % 3])
        P.raw("s_branch Lfs%d_%%=" % n)

    def emit(self):
        st = self.st
        P, L, nx, ACC = st.P, st.L, st.nx, st.ACC
        stubs = []
        for n in range(1, L.NSTASH + 1):
            with st.emitting(P.fresh()) as stub:
                self.emit_stub(n)
            stubs.append(stub)
        fstub = 64
        while fstub < 8 * max(q.n_instr for q in stubs):
            fstub *= 2
        P.v("v_cmp_ne_u32_e64 %s, 0, %%[dfshift]" % self.S_DFSEL)
        self.entry_jump(fstub)
        n_fwd0 = P.n_instr
        for n in range(L.NSTASH, 0, -1):
            c, a, ap = self.sets(n)
            P.label("Lfs%d_%%=" % n)
            P.raw("s_waitcnt lgkmcnt(0)")
            Vn, ln = self.VR[(n - 1) % 2], self.LN[(n - 1) % 2]
            lam = [lambda j=j: P.fmac_dpp(ln, self.TAUR[(n - 1) % 3], Vn[j], j) for j in range(nx)]   # lambda_{t+1} += V x_{t+1}
            if n >= 2:
                self.data_wait(n)
                fill = [lambda m=n - 2: self.prefetch_a(m), lambda m=n - 2: (self.adj_prefetch_b(m), self.load_data(m))]
            else:
                fill = []
            self.fcompute(c, a, ap, S_SM, False, fill + lam)
            self.outputs(n, False)
        st.n_fwd, st.n_fwd_steps = P.n_instr - n_fwd0, L.NSTASH
        c, a, ap = self.sets(0)
        P.raw("s_waitcnt lgkmcnt(0)")
        self.fcompute(c, a, ap, S_UM, True)
        self.outputs(0, True)
        P.v("v_mov_b32_e32 %%[xvout], %s" % ACC[a])
        P.raw("s_branch Ldone_%=")
        P.align(fstub.bit_length() - 1)
        P.label("Lfstub_%=")
        for stub in stubs:
            P.align(fstub.bit_length() - 1)
            P.append(stub)


def backward_stubs(st):
    """F block of ring slot (n % D) -> stash slot n-1, one stub per step, called from the backward sweep"""
    P, L = st.P, st.L
    P.align(5)
    P.label("Lbstub_%=")
    for n in range(1, L.NSTASH + 1):
        P.align(5)
        for p, (w, off) in enumerate(L.stash_pieces):
            regs = st.stash_regs_of(p, n - 1)
            if w == 2:
                P.raw("ds_read2_b32 a[%d:%d], %%[sr%d] offset0:%d offset1:%d" % (regs[0], regs[1], n % st.D, off, off + 1))
            else:
                P.raw("ds_read_b32 a%d, %%[sr%d] offset:%d" % (regs[0], n % st.D, off * 4))
        if st.K.ret_direct:   # stub n is called from step n-1: the peeled first step, then body positions 1 .. LC, 1, ...
            P.raw("s_branch Lret%d_%%=" % (st.bret["first"] if n == 1 else st.bret[(n - 2) % st.LC + 1]))
        else:
            P.raw("s_setpc_b64 " + S_RET)


def emit_rollout(st):
    """the rollout of stream `st` behind its backward sweep (and, stash forms, the backward sweep's stub table)"""
    rollout = (AdjRollout if st.adj else StashRollout if st.stash else RingRollout)(st)
    rollout.begin()
    rollout.emit()
    if st.stash:
        backward_stubs(st)
