"""The fused LQR solve as an instruction stream, first half: the knobs, the slot layout, the forms that exist, and
LqrStream - the register and operand plan of one stream with its backward (Riccati) sweep.  The rollouts that follow
the sweep are in gen_lqr_rollout.py, the C++ text around the stream in gen_lqr_asm.py (where the overview is).
"""
import collections
import contextlib

from gen_asm_emit import LabelCounter, Prog, Regs, VBASE, sgpr_lo, vrange

SHAPES = [(8, 2), (3, 1), (4, 2), (6, 2), (2, 2), (1, 1), (2, 1), (3, 2), (4, 4)]   # (4,4): round 4, plain / gains-out / any-horizon forms
DB = 3        # backward ring depth == number of rotating register sets
KROW = 12     # floats per gain row in LDS: [K_m (nx) | 0 (nu) | k_m | pad], 8-byte aligned rows


class Knobs(collections.namedtuple("Knobs", "fwd_depth no_vmwait no_dma no_ldsread skip_fwd skip_bwd fwd_skip timing newton "
                                            "warm_stubs ret_direct mfma_use mfma_dep qp_valu g10_mix ring_depth nt use_mfma")):
    """the GEN_* variables of the LQR stream generator, one field each"""
    __slots__ = ()

    @classmethod
    def from_env(cls, env):
        return cls(
            fwd_depth=int(env.get("GEN_FWD_DEPTH", "6")),   # forward ring depth == unroll (a multiple of 6: lcm of 2 row sets and 3 accumulators)
            # timing experiments only (scripts/asm_variants.sh): the results of such builds are wrong on purpose
            no_vmwait=env.get("GEN_NO_VMWAIT") == "1",      # drop the counted vmcnt waits inside the loops
            no_dma=env.get("GEN_NO_DMA") == "1",            # issue no DMA inside the loops
            no_ldsread=env.get("GEN_NO_LDSREAD") == "1",    # no ds_read inside the loops
            skip_fwd=env.get("GEN_SKIP_FWD") == "1",
            skip_bwd=env.get("GEN_SKIP_BWD") == "1",
            fwd_skip=frozenset(env.get("GEN_FWD_SKIP", "").split(",")),   # forward-sweep parts to drop: store,pst,stage,read,xpart,upart
            timing=env.get("GEN_TIMING") == "1",            # s_memtime at the phase boundaries -> info[] (no flags then)
            newton=env.get("GEN_NEWTON") == "1",            # one Newton step on each v_rcp_f32 (1 ulp -> ~0.5 ulp)
            warm_stubs=env.get("GEN_WARM_STUBS") == "1",    # experiment: run every stash stub once during the prologue wait
            ret_direct=env.get("GEN_RET_SETPC") != "1",     # stash stubs return by a direct s_branch (else s_setpc_b64)
            mfma_use=int(env.get("GEN_MFMA_USE", "5")),     # wait states kept before a non-accumulating use of an MFMA result
            mfma_dep=int(env.get("GEN_MFMA_DEP", "2")),     # wait states kept before an accumulation into the same tile
            # box QP: the clamped-set test on the VALU alone (6 VALU per control instead of 4 VALU + 3 SALU that wait for them): MPC step
            # at config-3 size 101.7 -> 99.0 us.  (Replacing the scalar OR behind the off-diagonal mask by two selects: no change.)
            qp_valu=env.get("GEN_QP_VALU", "1") == "1",
            g10_mix=env.get("GEN_G10_MIX") == "1",          # g1 DPP FMAs between (not before) the G MFMAs
            # Ring depth of the plain / saving / affine streams (the masked and MPC streams keep DB slots of whole 1 KB pieces: their
            # flags and bounds ride in the slot padding).  With more than DB slots the slot stride is the slot's own size (rounded up
            # to 64 B) and the last DMA of a group runs under an exec mask - whole pieces would not fit the 160 KB of a CU.
            ring_depth=int(env.get("GEN_RING_DEPTH", "3")),
            # nt (streaming) cache policy on the backward groups' LDS-DMA, per kind of stream (plain, save, affine, masked, mpc):
            # the inputs of a solve are read once; with the default policy they displace each other from L2 / the Infinity Cache on
            # their way through (HBM-streamed headline solve 38-40 -> 33.5-35 us, B = 8192: 78 -> 64 us; profiles/r03/ring_ab.txt).
            # With steady clocks (profiles/r03/nt_steady_state_variants.txt): save / affine / adj (DiffLqr's two launches) 110 -> 103.7 us
            # per training step; masked: no change; mpc: 99 -> 104 us - so the DiffLqr streams carry it too, the other two do not.
            nt=frozenset(env.get("GEN_NT", "plain,save,affine,adj").split(",")),
            use_mfma=env.get("GEN_NO_MFMA") != "1",         # F^T V F on v_mfma_f32_4x4x1_16b_f32 (else DPP FMAs)
        )


class Layout:
    """ring slots of one shape.  depth: slots of the backward ring of this stream; ring_depth, fwd_depth: the knobs that
    size the ring every stream of the shape shares"""

    def __init__(self, nx, nu, ring_depth, fwd_depth, depth=DB, ghbm=False):
        self.nx, self.nu, self.ns = nx, nu, nx + nu
        self.depth = depth
        self.DF = DF = fwd_depth
        ns = self.ns
        self.nC, self.nc, self.nF, self.nf = ns * ns, ns, nx * ns, nx          # 16-byte chunks per wave-step
        self.OFF_C = 0
        self.OFF_c = 16 * self.nC
        self.OFF_F = self.OFF_c + 16 * self.nc
        self.OFF_f = self.OFF_F + 16 * self.nF
        self.nchunk_b = self.nC + self.nc + self.nF + self.nf
        self.ndma_b = (self.nchunk_b + 63) // 64
        self.compact = depth > DB
        self.SLOT_B = self.ndma_b * 1024 if not self.compact else (16 * self.nchunk_b + 63) // 64 * 64
        # lanes of a group's last DMA that stay inside the slot (compact: the others would land in the next slot)
        self.last_lanes = (self.SLOT_B - (self.ndma_b - 1) * 1024) // 16
        self.FOFF_f = 16 * self.nF
        assert (nu * KROW) % 4 == 0
        self.nG = nu * KROW if ghbm else 0               # 16-byte chunks: 4 trajectories x nu x KROW floats / 4
        self.FOFF_G = 16 * (self.nF + self.nf)
        self.nchunk_f = self.nF + self.nf + self.nG
        self.ndma_f = (self.nchunk_f + 63) // 64
        self.SLOT_F = self.ndma_f * 1024
        # one ring size per shape, whatever the stream: ring_depth compact slots or DB slots of whole pieces
        deep = ring_depth * ((16 * self.nchunk_b + 63) // 64 * 64) if ring_depth > DB else 0
        self.RING = max(deep, DB * self.ndma_b * 1024, DF * self.SLOT_F)
        assert depth * self.SLOT_B <= self.RING
        assert self.ndma_b * 1024 - 1024 <= 4095 and ns + 1 <= 12 and nu in (1, 2, 3, 4)
        assert (depth - 1) * self.ndma_b <= 63 and (DF - 1) * self.ndma_f <= 63 and 1 <= self.last_lanes <= 64
        # ---- F stash (registers instead of a second HBM read of F), in the layout the forward sweep consumes:
        # lane i < 8 of a 16-lane row keeps columns [0, H) of row i of F_t, lane 8 + i columns [H, ns) - H
        # accumulation registers per timestep, read from the ring slot as pairs (ds_read2_b32) + a single
        self.stash_ok = (64 % nx == 0) and nx <= 8
        self.H = (ns + 1) // 2
        self.stash_pieces = []         # (registers, dword offset inside the half row)
        o = 0
        while self.H - o >= 2:
            self.stash_pieces.append((2, o))
            o += 2
        if self.H - o == 1:
            self.stash_pieces.append((1, o))
        self.stash_regs = self.H
        self.NSTASH = min(256 // self.stash_regs - (1 if 256 % self.stash_regs == 0 else 0), 64)
        self.SPD = 64 // nx                              # timesteps of f per DMA instruction
        self.NFD = (self.NSTASH + 1 + self.SPD - 1) // self.SPD
        self.FAREA = self.NFD * 1024                     # bytes of f per wave: f[tt] at tt * nx * 16

    def flags_fit(self):
        """room for the flag dwords of the masked and MPC forms in the slot padding"""
        return self.SLOT_B - 16 * self.nchunk_b >= 256


class Form(collections.namedtuple("Form", "kind write_k stash expand", defaults=(False,))):
    """Which stream: `kind` and the three switches that combine with it.  write_k: K_t, k_t go to HBM; stash: F stays in
    registers for the rollout instead of a second HBM read (the ring form reads it again); expand: mpc only.

    plain: the solve (lqr/lqr_recursion.py:69-209 of the reference).
    masked: LQR_active (mpc/active_constrained_lqr.py:110-137) - clamped controls get a zero right-hand side, Quu
    is zeroed outside free x free with 1e-8 on the clamped diagonal, so their gain rows come out exactly 0 (and the
    rollout needs no change); the value update keeps the unmasked blocks (:143-145).
    mpc: MPCstep.backward_rec (mpc/mpc_step.py:70-173), backward sweep only - the clamped set of every step is not an
    input but the result of the box QP min 1/2 k'Quu k + qu'k, lower - u <= k <= upper - u, solved IN the stream by the
    projected-Newton iteration of mpc/pnqp.py:37-201 (per-trajectory termination, warm-started from the later step,
    wave-uniform loops as pnqp_solve_rows of pnqp_device.hpp); k_t is its solution, K_t the masked solve with 1e-11 on
    the diagonal (the QP's own last factorisation, :147-157), the value update keeps the unmasked blocks (:165-166).
    u, lower, upper of the wave's four trajectories arrive as 12 nu dwords in the slot padding (the flag DMA of the
    masked variant, one float per lane).
    save (write_k only): the training form of the solve - besides K_t, k_t it leaves Quu_t and Qxu_t of every step in HBM,
    which is all DiffLqr.backward's second solve needs next to F (differentiable_lqr.py:95-134: same C, F, hence the
    same gains; only the affine terms change - the `affine` form below).
    affine (stash, no gains out): the re-solve of an LQR problem whose C and F have been solved before (the saving form
    above) with another c, f = 0 - DiffLqr.backward's second solve (differentiable_lqr.py:108-114: c = [grad_x; grad_u],
    x_init = 0).  The gains K_t and the blocks Quu_t, Qxu_t do not depend on c, so only the affine recursion is redone:
    q = c_t + F_t^T v_{t+1}, k_t = -Quu_t^-1 qu, v_t = qx + Qxu_t k_t (lqr_recursion.py:92,119-120,152 with
    qu + Quu k = 0), then the same rollout.  The slot's C region carries [K_t | Qxu_t | Quu_t] instead of C_t (36
    chunks instead of 100 at (8,2); the other lanes of those groups fetch a resident zero chunk): 504 B per
    timestep-solve instead of 832 B, and ~60 instructions per step instead of ~165.
    ghbm (ring form): the gain rows [K_m | 0 | k_m | pad] of every step go to a caller workspace in HBM ([T,B,nu,KROW] floats)
    instead of LDS and come back to the rollout with F and f, through the forward ring - the horizon is then bounded by
    nothing but the workspace (the LDS form holds T <= 74 at (8,2)).
    adj (the affine form plus): DiffLqr.backward in ONE launch that never reads C (differentiable_lqr.py:78-142).  The reference's
    solve is exact block elimination of the KKT system, so its co-states are the value function's gradients:
    lambda_t = V_t x_t + v_t and d_lambda_t = V_t dx_t + v'_t (v' the affine value term of the second solve) for any, also
    non-symmetric, C (tests/test_saved_gains_identity_cpu.py).  With [V_t | v_t] left in HBM by the saving solve the backward
    sweep is the affine recursion above (v'_t kept in LDS, in the area f would take), and the rollout of d_tau computes
    lambda_{t+1}, d_lambda_{t+1} on the way and writes dC_t, dc_t, dF_t, df_t (:128-134) itself - rows through an LDS
    staging area, whole 16-byte chunks to HBM.  [V_t | v_t | x_t | u_t] come through a four-slot LDS-DMA ring in the idle
    backward ring.
    expand (mpc only): need_expand of MPCstep.forward (mpc_step.py:305-317) inside the sweep - the slot padding also
    takes x_t (4 nx more dwords) and every step starts with c_hat = C [x_t; u_t] + c in the affine column."""
    __slots__ = ()
    KINDS = ("plain", "masked", "mpc", "save", "affine", "adj", "ghbm")

    masked = property(lambda self: self.kind in ("masked", "mpc"))
    mpc = property(lambda self: self.kind == "mpc")
    save = property(lambda self: self.kind == "save")
    affine = property(lambda self: self.kind in ("affine", "adj"))
    adj = property(lambda self: self.kind == "adj")
    ghbm = property(lambda self: self.kind == "ghbm")

    def check(self, L):
        """the combinations that exist, for the shape of layout L"""
        assert self.kind in self.KINDS
        assert not self.stash or L.stash_ok
        assert not self.ghbm or not (self.stash or self.write_k)
        assert not self.mpc or (self.write_k and not self.stash)
        assert not self.expand or (self.mpc and 12 * L.nu + 4 * L.nx <= 64)
        assert not self.save or self.write_k
        assert not self.affine or (self.stash and not self.write_k and L.ns >= 4)

    def struct_name(self, nx, nu):
        tf = lambda b: "true" if b else "false"
        if self.mpc:
            return "MpcAsm<%d, %d, %s>" % (nx, nu, tf(self.expand))
        return "LqrAsm<%d, %d, %s, %s, %s, %s, %s, %s, %s>" % (nx, nu, tf(self.write_k), tf(self.stash), tf(self.masked), tf(self.ghbm),
                                                               tf(self.save), tf(self.affine), tf(self.adj))


def forms_for(nx, nu, knobs):
    """the streams of shape (nx, nu), in the order they stand in the header"""
    L0 = Layout(nx, nu, knobs.ring_depth, knobs.fwd_depth)
    forms = []
    for write_k in (False, True):
        for stash in (False, True):
            if stash and not L0.stash_ok:
                continue
            forms.append(Form("plain", write_k, stash))
            if write_k and nu in (1, 2):
                forms.append(Form("save", write_k, stash))
            if stash and not write_k and nx + nu >= 4 and nu in (1, 2):
                forms.append(Form("affine", write_k, stash))
                forms.append(Form("adj", write_k, stash))
            if not stash and not write_k:
                forms.append(Form("ghbm", write_k, stash))
            if nu not in (1, 2):     # three and four controls: the plain, gains-out and any-horizon forms (the masked, MPC
                continue             # and training forms spell their pivoted solves out for 1 x 1 and 2 x 2)
            if not write_k and L0.flags_fit():
                forms.append(Form("masked", write_k, stash))
            if write_k and not stash and L0.flags_fit():
                forms.append(Form("mpc", True, False))
                if 12 * nu + 4 * nx <= 64:
                    forms.append(Form("mpc", True, False, expand=True))
    return forms


# ---- scalar registers of the stream
S_N, S_TF = "s70", "%[tf]"   # tf: time strides the DMA pointers may still take (an operand: it crosses the two asm blocks)
S_KM, S_SM, S_UM, S_XM, S_HI = "s[72:73]", "s[74:75]", "s[76:77]", "s[88:89]", "s[90:91]"
S_RET, S_STUB, S_JMP, S_TMP = "s[78:79]", "s[80:81]", "s[82:83]", "s84"
S_ROW0 = "s[98:99]"         # save: lane 0 of each 16-lane row
S_GM = "s[98:99]"           # ghbm: lanes 0..ns of each row (a whole gain row)
S_AFF = "s[100:101]"        # mpc: the lanes `aff` (the stash pairs above are the QP's masks there - no stash in that mode)
S_ACT = ["s[92:93]", "s[94:95]"]
QP_REG = "0x2d2febff"       # 1e-11f  (pnqp.py:73)
QP_TOLSQ = "0x322bcc76"     # smallest float32 whose root reaches 1e-4f (pnqp.py:140; pnqp_device.hpp kPnqpDxTolSqBits)
QP_GAMMA = "0x3dcccccd"     # 0.1f: GAMMA (pnqp.py:23) and the step decay (:163)
QP_MAXLS = 10               # pnqp.py:172
BSTUB = 32                  # bytes per backward stub (two LDS reads + s_setpc_b64 = 20)


class LqrStream:
    """One stream: the layout, the register plan, the scalar registers, lane masks and operand names, and the emitter
    `P` that the phases below write into.  emit_backward() leaves the prologue and the backward sweep in P and the
    block that issues the first DMA groups in P_first; the rollout (gen_lqr_rollout.py) and finish() follow."""

    def __init__(self, nx, nu, form, knobs):
        self.nx, self.nu, self.form, self.K = nx, nu, form, knobs
        self.write_k, self.stash, self.expand = form.write_k, form.stash, form.expand
        self.masked, self.mpc, self.save, self.affine, self.adj, self.ghbm = form.masked, form.mpc, form.save, form.affine, form.adj, form.ghbm
        self.D = DB if (self.masked or self.mpc) else knobs.ring_depth      # ring slots (the register sets stay three)
        self.nt = ("plain" if self.ghbm else form.kind) in knobs.nt         # the backward groups carry the nt policy
        self.L = L = Layout(nx, nu, knobs.ring_depth, knobs.fwd_depth, self.D, self.ghbm)
        self.ns = self.aff = L.ns
        form.check(L)
        self.P = Prog(knobs.mfma_use, knobs.mfma_dep)
        self.labels = LabelCounter()       # Ladv / Lqp / Lfrare ... of the sequences emitted more than once
        self.callsites = LabelCounter()    # return labels of the backward stubs' call sites
        self.swaps = LabelCounter()        # Lnoswap of the pivot searches
        self.in_loop = False               # inside a loop body: where the timing knobs drop things
        self.bret = {}                     # body position of the loop (or "first") -> return label number of its call site
        self.plan_operands()
        self.plan_registers()
        self.lane_masks = ((S_KM, list(range(nx)) + [self.aff]), (S_SM, range(self.ns)), (S_UM, range(nx, self.ns)), (S_XM, range(nx)),
                           (S_HI, range(nx, 16)))   # S_HI: the lanes whose row registers take gain rows (lanes < nx take F rows)
        self.PADM = 16 * L.nchunk_b              # masked: the flags of the wave's 4 trajectories land in the slot's padding
        assert not self.masked or L.SLOT_B - self.PADM >= 256
        self.NDB_ALL = L.ndma_b + (1 if self.masked else 0)   # VMEM operations per backward group
        self.n_step_stores = 0      # global stores per backward step (not mpc)
        if self.write_k or self.ghbm:
            self.n_step_stores += nu
        if self.save:
            self.n_step_stores += self.SV_NST
        assert (self.D - 1) * (self.NDB_ALL + self.n_step_stores) <= 63
        self.LC = 3 * self.D // (3 if self.D % 3 == 0 else 1)     # steps per trip of the loop form: lcm(register sets, ring slots)
        assert 8 * len(L.stash_pieces) + 4 <= BSTUB

    # =============================================================== the plan
    def plan_operands(self):
        """operand names (C++ side: struct LqrAsmIn of lqr_asm_gen.hpp, filled by lqr_asm_kernel.hpp)"""
        L, nx, nu = self.L, self.nx, self.nu
        self.ptr = ["%%[ptr%d]" % q for q in range(L.ndma_b)]
        self.str1 = ["%%[str1_%d]" % q for q in range(L.ndma_b)]
        self.strd = ["%%[str%d]" % q for q in range(L.ndma_b)]
        self.aq = ["%%[aq%d]" % i for i in range(self.ns)]
        self.af = ["%%[af%d]" % k for k in range(nx)]
        self.fptr = ["%%[fptr%d]" % q for q in range(2 if self.adj else L.ndma_f)]
        self.fstr = ["%%[fstr%d]" % q for q in range(2 if self.adj else L.ndma_f)]
        self.fp = ["%%[fp%d]" % q for q in range(L.NFD)]
        self.pk = ["%%[pk%d]" % m for m in range(nu)]

    def plan_registers(self):
        L, nx, nu, ns = self.L, self.nx, self.nu, self.ns
        mpc, masked, save, affine, expand = self.mpc, self.masked, self.save, self.affine, self.expand
        R = Regs(VBASE)
        self.mfma = mfma = self.K.use_mfma and ns <= 12 and nx % 4 == 0 and not affine
        self.NQ = NQ = 4 * ((ns + 3) // 4)            # MFMA accumulator tiles are 4 consecutive rows
        # affine: a set is [c | - | Qxu (nu) | Quu (nu*nu) | K rows (nu)] at (nu = 2: 0, 2, 4, 8; nu = 1: 0, 1, 2, 3)
        self.AQX, self.AQU, self.AKR = (2, 4, 8) if nu == 2 else (1, 2, 3)
        self.Q = [R.take(max(ns, self.AKR + nu) if affine else (NQ if mfma else ns), align=4) for _ in range(3)]
        self.F = [R.take(nx) for _ in range(3)]
        self.W = R.take(max(nx, 8 if mpc else 4), align=4)     # DPP path: W = V F~ ; MFMA path: G = V^T F~ (rows = x columns of V); mpc: the QP's temporaries
        self.G10 = R.take(1)[0]                  # MFMA path: row "1" of G^ = F^T v
        self.A = [R.take(nu, align=4 if save and nu == 2 and m_ == 0 else 1) for m_ in range(nu)]   # save: Quu is staged as one b128
        # save: staging area [Vv | Qxu | Quu] of the wave's four trajectories (bytes), its chunks and store instructions
        self.SV_Q, self.SV_U = 16 * nx * (nx + 1), 16 * (nx * (nx + 1) + nx * nu)
        self.SV_N = nx * (nx + 1) + nx * nu + nu * nu
        self.SV_NST = (self.SV_N + 63) // 64
        self.Kt = R.take(nu)
        self.Rr = R.take(nu)
        # tP, tPQ, tL0, tM1, tRA, tRB, tRP, tT, tLL, tD2, tRD, tY1, tT2 of the solves
        self.TMP13 = R.take(13, align=2 if expand else 1)
        self.MINPIV = R.take(1)[0]
        self.QB = R.take(1)[0] if affine else None   # affine: second accumulator of q = c + F^T v
        self.XV0 = R.take(1)[0]                  # x_init (lanes < nx), loaded by the stream itself
        self.SVD = [R.take(4, align=4) for _ in range(self.SV_NST)] if save else None   # save: the staged chunks on their way out
        self.ACT = [R.take(nu) for _ in range(3)] if masked and not mpc else None   # clamped-control flags of the slot in each register set
        self.EPS = R.take(1)[0] if masked and not mpc else None
        self.UC = [R.take(nu) for _ in range(3)] if mpc else None      # mpc: u_t, lower_t, upper_t of the slot in each register set
        self.LB = [R.take(nu) for _ in range(3)] if mpc else None
        self.UB = [R.take(nu) for _ in range(3)] if mpc else None
        self.XK = R.take(nu) if mpc else None                          # QP iterate / k_t (the next step's warm start)
        self.QU = R.take(nu) if mpc else None                          # qu in every lane
        self.NQP = R.take(1)[0] if mpc else None                       # sum over t of the QP passes run          (mpc_step.py:145)
        self.QINFO = R.take(1)[0] if mpc else None                     # 4 once a QP ran into the iteration cap
        self.TAU = R.take(3) if expand else None                       # expand: lane j < ns of set s holds [x_t; u_t][j]
        self.Am = [R.take(nu) for _ in range(nu)] if masked else None   # masked Quu
        self.Rm = R.take(nu) if masked else None                        # masked right-hand side rows
        # forward sweep registers reuse the Q / F sets (the backward sweep is over by then)
        RF = Regs(VBASE)
        self.M = [RF.take(ns, align=4), RF.take(ns, align=4), RF.take(ns, align=4)]
        self.ACC = RF.take(4)
        assert RF.next <= int(self.MINPIV[1:])
        assert R.next - 1 <= 255
        self.n_agpr = L.stash_regs * L.NSTASH if self.stash else 0
        assert self.n_agpr <= 256
        self.TS = R.take(4) if self.K.timing and not mpc else []     # (the mpc streams have no registers left for the stamps)
        self.last_vgpr = R.next - 1

    def stash_regs_of(self, p, j):
        """AGPR numbers of piece p of stash slot j (pairs are 64-bit aligned: all pair regions come first)"""
        L = self.L
        base = 0
        for pp in range(p):
            base += L.stash_pieces[pp][0] * L.NSTASH
        w = L.stash_pieces[p][0]
        return [base + j * w + k for k in range(w)]

    @contextlib.contextmanager
    def emitting(self, p):
        """the phases called inside write into the emitter p instead of the stream's own"""
        keep, self.P = self.P, p
        try:
            yield p
        finally:
            self.P = keep

    def stamp(self, i):
        if self.TS:
            self.P.raw("s_memtime s[86:87]")
            self.P.raw("s_waitcnt lgkmcnt(0)")
            self.P.v("v_mov_b32_e32 %s, s86" % self.TS[i], writes=(self.TS[i],))

    # =============================================================== DMA ring
    def issue_group(self, ptrs, slot, slot_bytes, gap=None):
        """gap: an instruction to emit in the wait state between the M0 write and the first LDS-DMA (else s_nop)"""
        P, L = self.P, self.L
        if self.K.no_dma and self.in_loop:
            if gap:
                P.raw(gap)
            return
        if slot == 0:
            P.raw("s_mov_b32 m0, %[ring]")
        else:
            P.raw("s_add_u32 m0, %%[ring], %d" % (slot * slot_bytes))
        if gap:
            P.raw(gap)
        else:
            P.nop(1)
        for q, p in enumerate(ptrs):
            off = (" offset:%d" % (q * 1024)) if q else ""
            part = ptrs is self.ptr and L.compact and q == len(ptrs) - 1 and L.last_lanes < 64
            if part:     # the rest of this piece would land in the next slot
                P.raw("s_mov_b64 exec, 0x%x" % ((1 << L.last_lanes) - 1))
            P.raw("global_load_lds_dwordx4 %s, off%s%s" % (p, off, " nt" if self.nt and ptrs is self.ptr else ""))
            if part:
                P.exec_all()
        if self.masked and ptrs is self.ptr:   # 4 * nu flag bytes = nu dwords, one per lane (the other lanes repeat dword 0)
            P.raw("global_load_lds_dword %%[pm], off offset:%d" % self.PADM)

    def advance(self, ptrs, strides, by_steps_left=None):
        """move the DMA pointers one timestep back unless they already sit on the first timestep.  In the prologue
        that is counted in tf.  Inside the backward sweep the strides left are a fixed distance from the loop counter
        S_N (step n of the sweep, n = 0 peeled: tf = T-1-D-n, S_N = T-2 for n = 0 and T-1-n after), so the sweep
        tests S_N against by_steps_left (D for the peeled step, D+1 in the loop) and tf is not maintained there."""
        P = self.P
        lab = "Ladv%d_%%=" % self.labels.next()
        if by_steps_left is not None:
            P.raw("s_cmp_ge_i32 %s, %d" % (S_N, by_steps_left))
        else:
            P.raw("s_cmp_gt_i32 %s, 0" % S_TF)
        P.raw("s_cbranch_scc0 " + lab)
        for p, s in zip(ptrs, strides):
            P.v("v_lshl_add_u64 %s, %s, 0, %s" % (p, p, s))
        if self.masked and ptrs is self.ptr:
            P.v("v_lshl_add_u64 %[pm], %[pm], 0, %[dm]")
        if by_steps_left is None:
            P.raw("s_sub_i32 %s, %s, 1" % (S_TF, S_TF))
        P.label(lab, reset=False)   # only pointer registers are written on the fall-through path

    def vmwait(self, n):
        if not ((self.K.no_vmwait or self.K.no_dma) and self.in_loop):
            self.P.raw("s_waitcnt vmcnt(%d)" % n)

    # =============================================================== slot reads
    def read_set(self, s, slot):
        if self.K.no_ldsread and self.in_loop:
            return
        P, nx, nu, ns, Q, F, aq, af = self.P, self.nx, self.nu, self.ns, self.Q, self.F, self.aq, self.af
        AQX, AQU, AKR = self.AQX, self.AQU, self.AKR
        off = slot * self.L.SLOT_B
        P.uses(Q[s][:ns] + F[s])
        if self.affine:
            P.raw("ds_read_b32 %s, %s offset:%d" % (Q[s][0], aq[0], off))                       # c_t, lane j = c[j]
            if nu == 2:
                P.raw("ds_read_b64 %s, %s offset:%d" % (vrange(Q[s][AQX:AQX + 2]), aq[1], off))  # Qxu row of lane i < nx
                P.raw("ds_read_b128 %s, %s offset:%d" % (vrange(Q[s][AQU:AQU + 4]), aq[2], off)) # Quu, the same in every lane
            else:
                P.raw("ds_read_b32 %s, %s offset:%d" % (Q[s][AQX], aq[1], off))
                P.raw("ds_read_b32 %s, %s offset:%d" % (Q[s][AQU], aq[2], off))
            for m in range(nu):                                                                  # K rows, lane j < nx = K[m][j]
                P.raw("ds_read_b32 %s, %s offset:%d" % (Q[s][AKR + m], aq[3], off + m * nx * 4))
        for i in range(0 if self.affine else ns):
            P.raw("ds_read_b32 %s, %s offset:%d" % (Q[s][i], aq[i], off))
        for k in range(nx):
            P.raw("ds_read_b32 %s, %s offset:%d" % (F[s][k], af[k], off))
        if self.mpc:
            UC, LB, UB = self.UC, self.LB, self.UB
            P.uses(UC[s] + LB[s] + UB[s])
            for a_, regs in enumerate((UC[s], LB[s], UB[s])):     # [u | lower | upper], 4 nu floats each
                for m in range(nu):
                    P.raw("ds_read_b32 %s, %%[am] offset:%d" % (regs[m], off + self.PADM + (a_ * 4 * nu + m) * 4))
            if self.expand:
                P.uses([self.TAU[s]])
                P.raw("ds_read_b32 %s, %%[atau] offset:%d" % (self.TAU[s], off + self.PADM))
        elif self.masked:
            for m in range(nu):
                P.raw("ds_read_u8 %s, %%[am] offset:%d" % (self.ACT[s][m], off + self.PADM + m))

    def read_ct(self, slot):
        """expand: row min(lane, ns-1) of C_t of the slot into the temporaries (lane i: C[i][0..ns-1]) - the operand of the
        re-centring C tau at the top of the step that consumes the slot; issued where the temporaries are idle (end of
        the step before), waited for by that step's first s_waitcnt lgkmcnt(0)"""
        P, ns, TMP13 = self.P, self.ns, self.TMP13
        off = slot * self.L.SLOT_B
        if ns % 2 == 0:
            for k in range(0, ns, 2):
                P.raw("ds_read_b64 %s, %%[act] offset:%d" % (vrange(TMP13[k:k + 2]), off + k * 4))
        else:
            for k in range(ns):
                P.raw("ds_read_b32 %s, %%[act] offset:%d" % (TMP13[k], off + k * 4))

    # =============================================================== the solves
    def rcp_newton(self, dst, src, tmp):
        """dst = 1/src, v_rcp_f32 + one Newton step (fast_rcp of colwise.hpp: the QP's tests sit on these quotients)"""
        P = self.P
        P.v("v_rcp_f32_e32 %s, %s" % (dst, src), writes=(dst,), reads=(src,), trans=True)
        P.v("v_fma_f32 %s, -%s, %s, 1.0" % (tmp, src, dst), writes=(tmp,), reads=(src, dst))
        P.v("v_fmac_f32_e32 %s, %s, %s" % (dst, tmp, dst), writes=(dst,), reads=(tmp, dst))

    def neg_solve(self, Au, rhs, out):
        """out = -Au^-1 rhs, nu x nu with partial pivoting in the operation order of lu_factor_rinv / lu_solve_rinv
        (colwise.hpp; LAPACK getf2 / getrs), reciprocal pivots with a Newton step"""
        P, rcp_newton = self.P, self.rcp_newton
        tP, tPQ, tL0, tM1, tRA, tRB, tRP, tT, tLL, tD2, tRD, tY1, tT2 = self.TMP13
        if self.nu == 1:
            rcp_newton(tRP, Au[0][0], tT)
            P.v("v_mul_f32_e64 %s, %s, -%s" % (out[0], rhs[0], tRP), writes=(out[0],), reads=(rhs[0], tRP))
            return
        a00, a01, a10, a11 = Au[0][0], Au[0][1], Au[1][0], Au[1][1]
        P.v("v_cmp_gt_f32_e64 vcc, |%s|, |%s|" % (a10, a00), reads=(a10, a00))
        P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tP, a00, a10), writes=(tP,), reads=(a00, a10))
        P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tL0, a10, a00), writes=(tL0,), reads=(a00, a10))
        P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tPQ, a01, a11), writes=(tPQ,), reads=(a01, a11))
        P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tM1, a11, a01), writes=(tM1,), reads=(a01, a11))
        P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tRA, rhs[0], rhs[1]), writes=(tRA,), reads=(rhs[0], rhs[1]))
        P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tRB, rhs[1], rhs[0]), writes=(tRB,), reads=(rhs[0], rhs[1]))
        rcp_newton(tRP, tP, tT)
        P.v("v_mul_f32_e32 %s, %s, %s" % (tLL, tL0, tRP), writes=(tLL,), reads=(tL0, tRP))
        P.v("v_fma_f32 %s, -%s, %s, %s" % (tD2, tLL, tPQ, tM1), writes=(tD2,), reads=(tLL, tPQ, tM1))
        P.v("v_fma_f32 %s, -%s, %s, %s" % (tY1, tLL, tRA, tRB), writes=(tY1,), reads=(tLL, tRA, tRB))
        rcp_newton(tRD, tD2, tT)
        P.v("v_mul_f32_e64 %s, %s, -%s" % (out[1], tY1, tRD), writes=(out[1],), reads=(tY1, tRD))
        P.v("v_fma_f32 %s, %s, %s, %s" % (tT2, tPQ, out[1], tRA), writes=(tT2,), reads=(tPQ, out[1], tRA))
        P.v("v_mul_f32_e64 %s, %s, -%s" % (out[0], tT2, tRP), writes=(out[0],), reads=(tT2, tRP))

    def masked_hessian(self, reg):
        """Am = Quu on free x free, 0 elsewhere, + `reg` on the diagonal (a register or a literal), from S_ACT"""
        P, nu, A, Am = self.P, self.nu, self.A, self.Am
        if nu == 2:
            P.raw("s_or_b64 s[96:97], s[92:93], s[94:95]")
        for m in range(nu):
            for l in range(nu):
                if m == l:
                    P.v("v_cndmask_b32_e64 %s, %s, 0, %s" % (Am[m][l], A[m][l], S_ACT[m]), writes=(Am[m][l],), reads=(A[m][l],))
                    P.v("v_add_f32_e32 %s, %s, %s" % (Am[m][l], reg, Am[m][l]), writes=(Am[m][l],), reads=(Am[m][l],))
                else:
                    P.v("v_cndmask_b32_e64 %s, %s, 0, s[96:97]" % (Am[m][l], A[m][l]), writes=(Am[m][l],), reads=(A[m][l],))

    def box_qp(self, s, first):
        """PNQP (mpc/pnqp.py:37-201) on H = A (Quu, in every lane), q = QU, bounds LB/UB - UC of register set s; warm
        start XK (first: cold start -H^-1 q, :75-83).  Leaves the solution in XK and the clamped set of the last pass in
        S_ACT.  Every lane of a 16-lane row runs it on its trajectory's data; both loops are wave-uniform (they run
        while any lane needs them) and finished lanes keep their state by construction - see pnqp_solve_rows."""
        P, nu, A, W, UC, XK, QU, NQP, QINFO, rcp_newton = self.P, self.nu, self.A, self.W, self.UC, self.XK, self.QU, self.NQP, self.QINFO, self.rcp_newton
        tP, tPQ, tL0, tM1, tRA, tRB, tRP, tT, tLL, tD2, tRD, tY1, tT2 = self.TMP13
        u_ = self.labels.next()
        LO, HI = self.LB[s], self.UB[s]             # turned into the QP's bounds in place
        Gv, DXv, XH, GD = W[0:nu], W[2:2 + nu], W[4:4 + nu], W[6:6 + nu]   # W is idle between the Q update and the next step
        AL = self.G10
        S_DONE, S_SRCH, S_T0, S_T1, S_T2 = "s[78:79]", "s[80:81]", "s[82:83]", "s[86:87]", "s[98:99]"
        S_I, S_CNT = S_TMP, "s85"
        for m in range(nu):
            P.v("v_sub_f32_e32 %s, %s, %s" % (LO[m], LO[m], UC[s][m]), writes=(LO[m],), reads=(LO[m], UC[s][m]))   # mpc_step.py:136-138
            P.v("v_sub_f32_e32 %s, %s, %s" % (HI[m], HI[m], UC[s][m]), writes=(HI[m],), reads=(HI[m], UC[s][m]))
        if first:
            self.neg_solve(A, QU, XK)
        for m in range(nu):                                                                   # pnqp.py:93
            P.v("v_max_f32_e32 %s, %s, %s" % (XK[m], XK[m], LO[m]), writes=(XK[m],), reads=(XK[m], LO[m]))
            P.v("v_min_f32_e32 %s, %s, %s" % (XK[m], XK[m], HI[m]), writes=(XK[m],), reads=(XK[m], HI[m]))
        P.raw("s_mov_b64 %s, 0" % S_DONE)
        P.raw("s_mov_b32 %s, 0" % S_I)
        P.label("Lqp%d_%%=" % u_, reset=False)   # (the back edge leaves no DPP / transcendental hazard open)
        # grad = Hx + q (:98); clamped = at a bound with the gradient pushing outwards (:110, exact equality)
        for m in range(nu):
            P.v("v_fma_f32 %s, %s, %s, %s" % (Gv[m], A[m][0], XK[0], QU[m]), writes=(Gv[m],), reads=(A[m][0], XK[0], QU[m]))
            for l in range(1, nu):
                P.v("v_fmac_f32_e32 %s, %s, %s" % (Gv[m], A[m][l], XK[l]), writes=(Gv[m],), reads=(A[m][l], XK[l], Gv[m]))
        for m in range(nu):
            if self.K.qp_valu:
                # clamped = (x == lo & g > 0) | (x == hi & g < 0)  <=>  max(x == lo ? g : -1, x == hi ? -g : -1) > 0
                # (a NaN gradient gives "not clamped" either way: v_max returns the other operand, the compare is false)
                P.v("v_cmp_eq_f32_e32 vcc, %s, %s" % (XK[m], LO[m]), reads=(XK[m], LO[m]))
                P.v("v_cndmask_b32_e32 %s, -1.0, %s, vcc" % (tRA, Gv[m]), writes=(tRA,), reads=(Gv[m],))
                P.v("v_cmp_eq_f32_e32 vcc, %s, %s" % (XK[m], HI[m]), reads=(XK[m], HI[m]))
                P.v("v_cndmask_b32_e64 %s, -1.0, -%s, vcc" % (tRB, Gv[m]), writes=(tRB,), reads=(Gv[m],))
                P.v("v_max_f32_e32 %s, %s, %s" % (tRA, tRA, tRB), writes=(tRA,), reads=(tRA, tRB))
                P.v("v_cmp_lt_f32_e64 %s, 0, %s" % (S_ACT[m], tRA), reads=(tRA,))
                continue
            P.v("v_cmp_eq_f32_e64 %s, %s, %s" % (S_T0, XK[m], LO[m]), reads=(XK[m], LO[m]))
            P.v("v_cmp_lt_f32_e64 %s, 0, %s" % (S_T1, Gv[m]), reads=(Gv[m],))
            P.v("v_cmp_eq_f32_e64 %s, %s, %s" % (S_T2, XK[m], HI[m]), reads=(XK[m], HI[m]))
            P.v("v_cmp_gt_f32_e64 vcc, 0, %s" % Gv[m], reads=(Gv[m],))
            P.raw("s_and_b64 %s, %s, %s" % (S_T0, S_T0, S_T1))
            P.raw("s_and_b64 %s, %s, vcc" % (S_T2, S_T2))
            P.raw("s_or_b64 %s, %s, %s" % (S_ACT[m], S_T0, S_T2))
        for m in range(nu):
            P.v("v_cndmask_b32_e64 %s, %s, 0, %s" % (GD[m], Gv[m], S_ACT[m]), writes=(GD[m],), reads=(Gv[m],))
        self.masked_hessian(QP_REG)                                                           # :124-129
        self.neg_solve(self.Am, GD, DXv)                                                      # :134-136
        P.v("v_mul_f32_e32 %s, %s, %s" % (tT, DXv[0], DXv[0]), writes=(tT,), reads=(DXv[0],))
        for m in range(1, nu):
            P.v("v_fmac_f32_e32 %s, %s, %s" % (tT, DXv[m], DXv[m]), writes=(tT,), reads=(DXv[m], tT))
        P.v("v_cmp_le_f32_e32 vcc, %s, %s" % (QP_TOLSQ, tT), reads=(tT,))                     # large = |dx| >= 1e-4 (:139-140)
        # one more pass counted for every lane that had not converged before this one (sum = 1 + it, mpc_step.py:145)
        P.raw("s_not_b64 %s, %s" % (S_T0, S_DONE))
        P.v("v_addc_co_u32_e64 %s, %s, %s, 0, %s" % (NQP, S_T1, NQP, S_T0), writes=(NQP,), reads=(NQP,))
        P.raw("s_orn2_b64 %s, %s, vcc" % (S_DONE, S_DONE))                                    # done |= !large  (:141-144)
        P.raw("s_cmp_eq_u64 %s, -1" % S_DONE)
        P.raw("s_cbranch_scc1 Lqpx%d_%%=" % u_)
        # backtracking line search (:162-190); lhs = 1 + 0.5 d'Hd / g'd as in pnqp_device.hpp
        P.v("v_mov_b32_e32 %s, 1.0" % AL, writes=(AL,))
        P.raw("s_not_b64 %s, %s" % (S_SRCH, S_DONE))
        P.raw("s_mov_b32 %s, 0" % S_CNT)
        P.label("Lls%d_%%=" % u_, reset=False)
        for m in range(nu):
            P.v("v_fma_f32 %s, %s, %s, %s" % (XH[m], AL, DXv[m], XK[m]), writes=(XH[m],), reads=(AL, DXv[m], XK[m]))   # :173
            P.v("v_max_f32_e32 %s, %s, %s" % (XH[m], XH[m], LO[m]), writes=(XH[m],), reads=(XH[m], LO[m]))
            P.v("v_min_f32_e32 %s, %s, %s" % (XH[m], XH[m], HI[m]), writes=(XH[m],), reads=(XH[m], HI[m]))
        for m in range(nu):
            P.v("v_sub_f32_e32 %s, %s, %s" % (GD[m], XH[m], XK[m]), writes=(GD[m],), reads=(XH[m], XK[m]))
        P.v("v_mul_f32_e32 %s, %s, %s" % (tRA, Gv[0], GD[0]), writes=(tRA,), reads=(Gv[0], GD[0]))       # g'd
        for m in range(1, nu):
            P.v("v_fmac_f32_e32 %s, %s, %s" % (tRA, Gv[m], GD[m]), writes=(tRA,), reads=(Gv[m], GD[m], tRA))
        for m in range(nu):                                                                    # d'Hd
            P.v("v_mul_f32_e32 %s, %s, %s" % (tRB, A[m][0], GD[0]), writes=(tRB,), reads=(A[m][0], GD[0]))
            for l in range(1, nu):
                P.v("v_fmac_f32_e32 %s, %s, %s" % (tRB, A[m][l], GD[l]), writes=(tRB,), reads=(A[m][l], GD[l], tRB))
            if m == 0:
                P.v("v_mul_f32_e32 %s, %s, %s" % (tLL, GD[0], tRB), writes=(tLL,), reads=(GD[0], tRB))
            else:
                P.v("v_fmac_f32_e32 %s, %s, %s" % (tLL, GD[m], tRB), writes=(tLL,), reads=(GD[m], tRB, tLL))
        rcp_newton(tRD, tRA, tT)
        P.v("v_mul_f32_e32 %s, 0.5, %s" % (tLL, tLL), writes=(tLL,), reads=(tLL,))
        P.v("v_fma_f32 %s, %s, %s, 1.0" % (tLL, tLL, tRD), writes=(tLL,), reads=(tLL, tRD))              # :175-176
        P.v("v_cmp_ge_f32_e32 vcc, %s, %s" % (QP_GAMMA, tLL), reads=(tLL,))                               # lhs <= GAMMA
        P.raw("s_and_b64 vcc, vcc, %s" % S_SRCH)                                                          # fails
        P.v("v_mul_f32_e32 %s, %s, %s" % (tT, QP_GAMMA, AL), writes=(tT,), reads=(AL,))
        P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (AL, AL, tT), writes=(AL,), reads=(AL, tT))            # :185-186
        P.raw("s_add_u32 %s, %s, 1" % (S_CNT, S_CNT))
        P.raw("s_cmp_lt_u32 %s, %d" % (S_CNT, QP_MAXLS))
        P.raw("s_cselect_b64 %s, vcc, 0" % S_SRCH)                                                        # :172
        P.raw("s_cmp_lg_u64 %s, 0" % S_SRCH)
        P.raw("s_cbranch_scc1 Lls%d_%%=" % u_)
        for m in range(nu):                                                                                # :190
            P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (XK[m], XH[m], XK[m], S_DONE), writes=(XK[m],), reads=(XH[m], XK[m]))
        P.raw("s_add_u32 %s, %s, 1" % (S_I, S_I))
        P.raw("s_cmp_lt_u32 %s, %%[nqp_iter]" % S_I)
        P.raw("s_cbranch_scc1 Lqp%d_%%=" % u_)
        # iteration cap (:192): lanes that never converged
        P.v("v_cndmask_b32_e64 %s, 4, 0, %s" % (tT, S_DONE), writes=(tT,))
        P.v("v_or_b32_e32 %s, %s, %s" % (QINFO, tT, QINFO), writes=(QINFO,), reads=(tT, QINFO))
        P.label("Lqpx%d_%%=" % u_, reset=False)

    def mask_clamped(self, s):
        """masked: the right-hand side rows Rm and Quu Am of the free controls of register set s (flags ACT)"""
        P, nx, nu, A, Am, Rm, ACT, EPS, Qs = self.P, self.nx, self.nu, self.A, self.Am, self.Rm, self.ACT, self.EPS, self.Q[s]
        for m in range(nu):
            P.v("v_cmp_ne_u32_e64 %s, 0, %s" % (S_ACT[m], ACT[s][m]), reads=(ACT[s][m],))
        if nu == 2:
            P.raw("s_or_b64 s[96:97], s[92:93], s[94:95]")
        for m in range(nu):
            P.v("v_cndmask_b32_e64 %s, %s, 0, %s" % (Rm[m], Qs[nx + m], S_ACT[m]), writes=(Rm[m],), reads=(Qs[nx + m],))
            for l in range(nu):
                if m == l:
                    P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (Am[m][l], A[m][l], EPS, S_ACT[m]), writes=(Am[m][l],),
                        reads=(A[m][l], EPS))
                else:
                    P.v("v_cndmask_b32_e64 %s, %s, 0, s[96:97]" % (Am[m][l], A[m][l]), writes=(Am[m][l],), reads=(A[m][l],))

    def gauss_jordan(self, rhs):
        """Three and four controls (round 4): Gauss-Jordan on the rows of [Qux | Quu | qu] where they lie (the HIP kernels'
        gauss_jordan_rows, riccati_blocks.hpp).  Row m is ONE register across the lanes and the multiplier of row i at
        pivot k one lane of it (lane nx + k): a DPP broadcast per multiplier, an FMA per row.  Partial pivoting in
        LAPACK's order: the candidates below the pivot bubble the first largest entry into row k (strict >: the first
        maximum wins; the remaining rows end up permuted differently from getf2's single interchange, which changes
        neither which values the later pivots see nor which register holds which unknown).  Working rows: W (the G
        tiles are dead here); the K registers themselves are written once, under the K mask, as before."""
        P, nx, nu, W, Kt, MINPIV = self.P, self.nx, self.nu, self.W, self.Kt, self.MINPIV
        tP, tPQ, tL0, tM1, tRA, tRB, tRP, tT, tLL, tD2, tRD, tY1, tT2 = self.TMP13
        assert not (self.masked or self.mpc or self.save) and len(W) >= nu and nu <= 4
        Wk = W[:nu]
        LI = [tL0, tM1, tRA, tRB][:nu]
        for m in range(nu):
            P.v("v_mov_b32_e32 %s, %s" % (Wk[m], rhs[m]), writes=(Wk[m],), reads=(rhs[m],))
        for k in range(nu):
            P.mov_dpp(tP, Wk[k], nx + k)
            for i in range(k + 1, nu):
                P.mov_dpp(LI[i], Wk[i], nx + k)
            if k + 1 < nu:
                # the interchange behind a wave-uniform branch: taken only when some trajectory of the wavefront has a
                # larger entry below its pivot (a Quu that is close to diagonally dominant never does)
                cand = [LI[i] for i in range(k + 1, nu)]
                if len(cand) == 3:
                    P.v("v_max3_f32 %s, |%s|, |%s|, |%s|" % (tT, cand[0], cand[1], cand[2]), writes=(tT,), reads=tuple(cand))
                    mx = "%s" % tT
                elif len(cand) == 2:
                    P.v("v_max_f32_e64 %s, |%s|, |%s|" % (tT, cand[0], cand[1]), writes=(tT,), reads=tuple(cand))
                    mx = "%s" % tT
                else:
                    mx = "|%s|" % cand[0]
                P.v("v_cmp_gt_f32_e64 vcc, %s, |%s|" % (mx, tP), reads=(tT, cand[0], tP))
                noswap = "Lnoswap%d_%%=" % self.swaps.next()
                P.raw("s_cbranch_vccz " + noswap)
            for i in range(k + 1, nu):
                P.v("v_cmp_gt_f32_e64 vcc, |%s|, |%s|" % (LI[i], tP), reads=(LI[i], tP))
                P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tT, Wk[k], Wk[i]), writes=(tT,), reads=(Wk[k], Wk[i]))
                P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (Wk[i], Wk[i], Wk[k]), writes=(Wk[i],), reads=(Wk[k], Wk[i]))
                P.v("v_mov_b32_e32 %s, %s" % (Wk[k], tT), writes=(Wk[k],), reads=(tT,))
                P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tT2, tP, LI[i]), writes=(tT2,), reads=(tP, LI[i]))
                P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (LI[i], LI[i], tP), writes=(LI[i],), reads=(tP, LI[i]))
                P.v("v_mov_b32_e32 %s, %s" % (tP, tT2), writes=(tP,), reads=(tT2,))
            if k + 1 < nu:
                P.label(noswap)
            P.v("v_min_f32_e64 %s, |%s|, %s" % (MINPIV, tP, MINPIV), writes=(MINPIV,), reads=(tP, MINPIV))
            self.rcp_newton(tRP, tP, tT)
            P.v("v_mul_f32_e32 %s, %s, %s" % (Wk[k], Wk[k], tRP), writes=(Wk[k],), reads=(Wk[k], tRP))
            for i in range(nu):
                if i == k:
                    continue
                l_ = LI[i]
                if i < k:
                    l_ = tLL
                    P.mov_dpp(tLL, Wk[i], nx + k)
                P.v("v_fma_f32 %s, -%s, %s, %s" % (Wk[i], l_, Wk[k], Wk[i]), writes=(Wk[i],), reads=(l_, Wk[k], Wk[i]))
        P.raw("s_mov_b64 exec, " + S_KM)
        for m in range(nu):
            P.v("v_mul_f32_e32 %s, -1.0, %s" % (Kt[m], Wk[m]), writes=(Kt[m],), reads=(Wk[m],))

    def gains(self, s, first=False):
        """K~ = -Quu^-1 [Qux | Quu | qu] per lane (lqr_recursion.py:112-120); leaves A (Quu), Kt, and MINPIV"""
        P, nx, nu, A, Kt, MINPIV, newton = self.P, self.nx, self.nu, self.A, self.Kt, self.MINPIV, self.K.newton
        tP, tPQ, tL0, tM1, tRA, tRB, tRP, tT, tLL, tD2, tRD, tY1, tT2 = self.TMP13
        Qs = self.Q[s]
        if nu <= 2:      # (three and four controls: nobody needs Quu in every lane - the rows are eliminated where they lie and
            for m in range(nu):      # the value update broadcasts Quu inside its FMAs)
                for l in range(nu):
                    P.mov_dpp(A[m][l], Qs[nx + m], nx + l)
        rhs = [Qs[nx + m] for m in range(nu)]
        Au = A
        if self.mpc:
            for m in range(nu):
                P.mov_dpp(self.QU[m], Qs[nx + m], self.aff)
            self.box_qp(s, first)
            for m in range(nu):      # K_t: rows of clamped controls zero, the QP's last H_f (mpc_step.py:147-157)
                P.v("v_cndmask_b32_e64 %s, %s, 0, %s" % (self.Rm[m], Qs[nx + m], S_ACT[m]), writes=(self.Rm[m],), reads=(Qs[nx + m],))
            # Am still holds that H_f: the QP's last pass built it from the same clamped set (a lane that converged
            # earlier rebuilt the same one from its frozen iterate)
            rhs, Au = self.Rm, self.Am
        elif self.masked:
            self.mask_clamped(s)
            rhs, Au = self.Rm, self.Am
        if nu >= 3:
            self.gauss_jordan(rhs)
        elif nu == 1:
            P.v("v_rcp_f32_e32 %s, %s" % (tRP, Au[0][0]), writes=(tRP,), reads=(Au[0][0],), trans=True)
            P.v("v_min_f32_e64 %s, |%s|, %s" % (MINPIV, Au[0][0], MINPIV), writes=(MINPIV,), reads=(Au[0][0], MINPIV))
            P.nop(1)
            if newton:
                P.v("v_fma_f32 %s, -%s, %s, 1.0" % (tT, Au[0][0], tRP), writes=(tT,), reads=(Au[0][0], tRP))
                P.v("v_fmac_f32_e32 %s, %s, %s" % (tRP, tT, tRP), writes=(tRP,), reads=(tT, tRP))
            P.raw("s_mov_b64 exec, " + S_KM)
            P.v("v_mul_f32_e64 %s, %s, -%s" % (Kt[0], rhs[0], tRP), writes=(Kt[0],), reads=(rhs[0], tRP))
        else:
            a00, a01, a10, a11 = Au[0][0], Au[0][1], Au[1][0], Au[1][1]
            P.v("v_cmp_gt_f32_e64 vcc, |%s|, |%s|" % (a10, a00), reads=(a10, a00))
            P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tP, a00, a10), writes=(tP,), reads=(a00, a10))
            P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tL0, a10, a00), writes=(tL0,), reads=(a00, a10))
            P.v("v_rcp_f32_e32 %s, %s" % (tRP, tP), writes=(tRP,), reads=(tP,), trans=True)
            P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tPQ, a01, a11), writes=(tPQ,), reads=(a01, a11))
            P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tM1, a11, a01), writes=(tM1,), reads=(a01, a11))
            P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tRA, rhs[0], rhs[1]), writes=(tRA,), reads=(rhs[0], rhs[1]))
            P.v("v_cndmask_b32_e32 %s, %s, %s, vcc" % (tRB, rhs[1], rhs[0]), writes=(tRB,), reads=(rhs[0], rhs[1]))
            if newton:
                P.v("v_fma_f32 %s, -%s, %s, 1.0" % (tT, tP, tRP), writes=(tT,), reads=(tP, tRP))
                P.v("v_fmac_f32_e32 %s, %s, %s" % (tRP, tT, tRP), writes=(tRP,), reads=(tT, tRP))
            P.v("v_mul_f32_e32 %s, %s, %s" % (tLL, tL0, tRP), writes=(tLL,), reads=(tL0, tRP))
            P.v("v_fma_f32 %s, -%s, %s, %s" % (tD2, tLL, tPQ, tM1), writes=(tD2,), reads=(tLL, tPQ, tM1))
            P.v("v_rcp_f32_e32 %s, %s" % (tRD, tD2), writes=(tRD,), reads=(tD2,), trans=True)
            P.v("v_fma_f32 %s, -%s, %s, %s" % (tY1, tLL, tRA, tRB), writes=(tY1,), reads=(tLL, tRA, tRB))
            P.v("v_min3_f32 %s, |%s|, |%s|, %s" % (MINPIV, tP, tD2, MINPIV), writes=(MINPIV,), reads=(tP, tD2, MINPIV))
            if newton:
                P.v("v_fma_f32 %s, -%s, %s, 1.0" % (tT, tD2, tRD), writes=(tT,), reads=(tD2, tRD))
                P.v("v_fmac_f32_e32 %s, %s, %s" % (tRD, tT, tRD), writes=(tRD,), reads=(tT, tRD))
            P.raw("s_mov_b64 exec, " + S_KM)
            P.v("v_mul_f32_e64 %s, %s, -%s" % (Kt[1], tY1, tRD), writes=(Kt[1],), reads=(tY1, tRD))
            P.v("v_fma_f32 %s, %s, %s, %s" % (tT2, tPQ, Kt[1], tRA), writes=(tT2,), reads=(tPQ, Kt[1], tRA))
            P.v("v_mul_f32_e64 %s, %s, -%s" % (Kt[0], tT2, tRP), writes=(Kt[0],), reads=(tT2, tRP))
        if self.mpc:   # k_t is the QP's solution (lane aff), not the masked solve's          mpc_step.py:141-146
            for m in range(nu):
                P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (Kt[m], Kt[m], self.XK[m], S_AFF), writes=(Kt[m],), reads=(Kt[m], self.XK[m]))
        self.store_gains(Qs)

    def store_gains(self, Qs):
        """gain rows -> LDS (and HBM when the caller wants Ks/ks), still under the K mask the solve has set; save: Qxu and
        Quu of the step to the staging area"""
        P, nx, nu, A, Kt, pk, mpc, ghbm = self.P, self.nx, self.nu, self.A, self.Kt, self.pk, self.mpc, self.ghbm
        if ghbm:     # ... -> the workspace, whole rows [K_m | 0 | k_m]: lanes nx..ns-1 of K~ are exactly 0, lane aff is column ns
            P.uses(Kt)
            P.raw("s_mov_b64 exec, " + S_GM)
            for m in range(nu):
                P.raw("global_store_dword %%[pgw], %s, off offset:%d" % (Kt[m], m * KROW * 4))
        elif not mpc:
            for m in range(nu):
                off = (" offset:%d" % (m * KROW * 4)) if m else ""
                P.raw("ds_write_b32 %%[ak], %s%s" % (Kt[m], off))
        if self.write_k:
            P.uses(Kt)
            for m in range(nu):
                P.raw("global_store_dword %s, %s, off" % (pk[m], Kt[m]))
        if self.save:
            # The saved blocks leave through an LDS staging area as the contiguous 16-byte chunks they form in HBM (the
            # 8-byte row pieces of Qxu, 36-byte rows of [V | v] cost more as stores than the solve's arithmetic: the saving
            # solve took 68 us with them against 40 us plain).  Qxu_t: rows i < nx of Q~ hold it in lanes nx..ns-1 (the value
            # update below writes over them); Quu_t: every lane has it in A - lane 0 of each row writes the nu * nu floats
            P.uses(Qs[:nx] + [r_ for row_ in A for r_ in row_])
            P.raw("s_mov_b64 exec, " + S_UM)
            for i in range(nx):
                P.raw("ds_write_b32 %%[asq], %s offset:%d" % (Qs[i], self.SV_Q + i * nu * 4))
            P.raw("s_mov_b64 exec, " + S_ROW0)
            quu = [r_ for row_ in A for r_ in row_]
            if nu == 2 and int(quu[0][1:]) % 4 == 0:
                P.raw("ds_write_b128 %%[asu], %s offset:%d" % (vrange(quu), self.SV_U))
            else:
                for j_, r_ in enumerate(quu):
                    P.raw("ds_write_b32 %%[asu], %s offset:%d" % (r_, self.SV_U + 4 * j_))
        P.exec_all()
        if self.write_k:
            for m in range(nu):
                P.v("v_lshl_add_u64 %s, %s, 0, %%[dk]" % (pk[m], pk[m]))
        if ghbm:
            P.v("v_lshl_add_u64 %[pgw], %[pgw], 0, %[dgw]")
        elif not mpc:
            P.v("v_add_u32_e32 %%[ak], %d, %%[ak]" % ((-nu * KROW * 4) & 0xffffffff))

    def gains_affine(self, s, first):
        """One step of the affine recursion.  The step is a chain of dependent instructions on a wavefront that has its
        SIMD to itself, so everything that does not depend on v_{t+1} - the factorisation of Quu_t (pivot choice, both
        reciprocals) - is interleaved with the chain that does, q = c_t + F_t^T v_{t+1} (two accumulators):
            q = c_t + F_t^T v_{t+1}   k_t = -Quu_t^-1 q_u (every lane)   v_t = q_x + Qxu_t k_t (lanes < nx of G10)
        and the gain rows [K_t | 0 | k_t] go to LDS for the rollout."""
        P, nx, nu, W, F, G10, QB, Kt = self.P, self.nx, self.nu, self.W, self.F, self.G10, self.QB, self.Kt
        AQX, AQU, AKR = self.AQX, self.AQU, self.AKR
        tP, tPQ, tL0, tM1, tRA, tRB, tRP, tT, tLL, tD2, tRD, tY1, tT2 = self.TMP13
        Qs = self.Q[s]
        QUa, KK = W[0:nu], W[2:2 + nu]
        Aa = [[Qs[AQU + m * nu + l] for l in range(nu)] for m in range(nu)]
        S_PIV = "s[86:87]"
        fact, qch = [], []
        if nu == 1:
            fact.append(lambda: P.v("v_rcp_f32_e32 %s, %s" % (tRP, Aa[0][0]), writes=(tRP,), reads=(Aa[0][0],), trans=True))
            fact.append(lambda: P.v("v_fma_f32 %s, -%s, %s, 1.0" % (tT, Aa[0][0], tRP), writes=(tT,), reads=(Aa[0][0], tRP)))
            fact.append(lambda: P.v("v_fmac_f32_e32 %s, %s, %s" % (tRP, tT, tRP), writes=(tRP,), reads=(tT, tRP)))
        else:
            a00, a01, a10, a11 = Aa[0][0], Aa[0][1], Aa[1][0], Aa[1][1]
            fact.append(lambda: P.v("v_cmp_gt_f32_e64 %s, |%s|, |%s|" % (S_PIV, a10, a00), reads=(a10, a00)))
            fact.append(lambda: P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (tP, a00, a10, S_PIV), writes=(tP,), reads=(a00, a10)))
            fact.append(lambda: P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (tL0, a10, a00, S_PIV), writes=(tL0,), reads=(a00, a10)))
            fact.append(lambda: P.v("v_rcp_f32_e32 %s, %s" % (tRP, tP), writes=(tRP,), reads=(tP,), trans=True))
            fact.append(lambda: P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (tPQ, a01, a11, S_PIV), writes=(tPQ,), reads=(a01, a11)))
            fact.append(lambda: P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (tM1, a11, a01, S_PIV), writes=(tM1,), reads=(a01, a11)))
            fact.append(lambda: P.v("v_fma_f32 %s, -%s, %s, 1.0" % (tT, tP, tRP), writes=(tT,), reads=(tP, tRP)))
            fact.append(lambda: P.v("v_fmac_f32_e32 %s, %s, %s" % (tRP, tT, tRP), writes=(tRP,), reads=(tT, tRP)))
            fact.append(lambda: P.v("v_mul_f32_e32 %s, %s, %s" % (tLL, tL0, tRP), writes=(tLL,), reads=(tL0, tRP)))
            fact.append(lambda: P.v("v_fma_f32 %s, -%s, %s, %s" % (tD2, tLL, tPQ, tM1), writes=(tD2,), reads=(tLL, tPQ, tM1)))
            fact.append(lambda: P.v("v_rcp_f32_e32 %s, %s" % (tRD, tD2), writes=(tRD,), reads=(tD2,), trans=True))
            fact.append(lambda: P.v("v_fma_f32 %s, -%s, %s, 1.0" % (tT2, tD2, tRD), writes=(tT2,), reads=(tD2, tRD)))
            fact.append(lambda: P.v("v_fmac_f32_e32 %s, %s, %s" % (tRD, tT2, tRD), writes=(tRD,), reads=(tT2, tRD)))
        if not first:       # q = c_t + F_t^T v_{t+1}: lane j takes column j of F_t, v_{t+1}[k] broadcast from lane k  (:92)
            for k in range(nx):
                if k == 1:
                    qch.append(lambda k=k: P.mul_dpp(QB, G10, F[s][k], k))
                elif k % 2 == 1:
                    qch.append(lambda k=k: P.fmac_dpp(QB, G10, F[s][k], k))
                else:
                    qch.append(lambda k=k: P.fmac_dpp(Qs[0], G10, F[s][k], k))
        while fact or qch:
            if qch:
                qch.pop(0)()
            if fact:
                fact.pop(0)()
        if not first and nx > 1:
            P.v("v_add_f32_e32 %s, %s, %s" % (Qs[0], QB, Qs[0]), writes=(Qs[0],), reads=(QB, Qs[0]))
        for m in range(nu):
            P.mov_dpp(QUa[m], Qs[0], nx + m)
        if nu == 1:
            P.v("v_mul_f32_e64 %s, %s, -%s" % (KK[0], QUa[0], tRP), writes=(KK[0],), reads=(QUa[0], tRP))
        else:                # the back half of neg_solve (LAPACK getrs order)
            P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (tRA, QUa[0], QUa[1], S_PIV), writes=(tRA,), reads=(QUa[0], QUa[1]))
            P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (tRB, QUa[1], QUa[0], S_PIV), writes=(tRB,), reads=(QUa[0], QUa[1]))
            P.v("v_fma_f32 %s, -%s, %s, %s" % (tY1, tLL, tRA, tRB), writes=(tY1,), reads=(tLL, tRA, tRB))
            P.v("v_mul_f32_e64 %s, %s, -%s" % (KK[1], tY1, tRD), writes=(KK[1],), reads=(tY1, tRD))
            P.v("v_fma_f32 %s, %s, %s, %s" % (tT2, tPQ, KK[1], tRA), writes=(tT2,), reads=(tPQ, KK[1], tRA))
            P.v("v_mul_f32_e64 %s, %s, -%s" % (KK[0], tT2, tRP), writes=(KK[0],), reads=(tT2, tRP))
        P.v("v_fma_f32 %s, %s, %s, %s" % (G10, Qs[AQX], KK[0], Qs[0]), writes=(G10,), reads=(Qs[AQX], KK[0], Qs[0]))
        for m in range(1, nu):
            P.v("v_fmac_f32_e32 %s, %s, %s" % (G10, Qs[AQX + m], KK[m]), writes=(G10,), reads=(Qs[AQX + m], KK[m], G10))
        for m in range(nu):
            P.v("v_cndmask_b32_e64 %s, %s, %s, %s" % (Kt[m], Qs[AKR + m], KK[m], S_AFF), writes=(Kt[m],),
                reads=(Qs[AKR + m], KK[m]))
        P.raw("s_mov_b64 exec, " + S_KM)
        for m in range(nu):
            off = (" offset:%d" % (m * KROW * 4)) if m else ""
            P.raw("ds_write_b32 %%[ak], %s%s" % (Kt[m], off))
        if self.adj:      # v'_t (lanes < nx of G10) goes where f_t would be: the rollout's d_lambda_t = V_t dx_t + v'_t reads it
            P.raw("s_mov_b64 exec, " + S_XM)
            P.raw("ds_write_b32 %%[avp], %s" % G10)
        P.exec_all()
        P.v("v_add_u32_e32 %%[ak], %d, %%[ak]" % ((-nu * KROW * 4) & 0xffffffff))
        if self.adj:
            P.v("v_add_u32_e32 %%[avp], %d, %%[avp]" % ((-nx * 16) & 0xffffffff))

    # =============================================================== value update
    def vupdate(self, s):
        """V~ = Q~x. + Qxu K~ + K~^T (Q~u. + Quu K~) in place in Q[s][0..nx-1]   (lqr_recursion.py:151-152)"""
        P, nx, nu, A, Kt, Rr = self.P, self.nx, self.nu, self.A, self.Kt, self.Rr
        Qs = self.Q[s]
        if nu >= 3:      # R = Q~u. + Quu K~ with Quu[m][l] broadcast from lane nx + l of row m inside the FMA
            for m in range(nu):
                P.v("v_mov_b32_e32 %s, %s" % (Rr[m], Qs[nx + m]), writes=(Rr[m],), reads=(Qs[nx + m],))
            for l in range(nu):
                for m in range(nu):
                    P.fmac_dpp(Rr[m], Qs[nx + m], Kt[l], nx + l)
        for m in range(nu if nu <= 2 else 0):
            P.v("v_fma_f32 %s, %s, %s, %s" % (Rr[m], A[m][0], Kt[0], Qs[nx + m]), writes=(Rr[m],),
                reads=(A[m][0], Kt[0], Qs[nx + m]))
            for l in range(1, nu):
                P.v("v_fmac_f32_e32 %s, %s, %s" % (Rr[m], A[m][l], Kt[l]), writes=(Rr[m],), reads=(A[m][l], Kt[l]))
        for m in range(nu):
            for i in range(nx):
                P.fmac_dpp(Qs[i], Qs[i], Kt[m], nx + m)
        if self.mfma:      # V~ += K^T R: the A^T B shape again (A = K~ row m, block i/4)
            for m in range(nu):
                for I in range(nx // 4):
                    P.mfma(Qs[4 * I:4 * I + 4], Kt[m], Rr[m], Qs[4 * I:4 * I + 4], I)
        else:
            for m in range(nu):
                for i in range(nx):
                    P.fmac_dpp(Qs[i], Kt[m], Rr[m], i)

    # =============================================================== one backward step
    def recentre(self, s):
        """expand: c_hat = c + C tau: lane i holds row i of C_t (read_ct), tau_k comes from lane k of TAU by a DPP broadcast -
        two accumulators; then entry i of the sum goes to the affine lane of row i of Q~ (one DPP FMA against e_aff).
        (Until round 2's last day the rows of Q~ - columns per lane - were multiplied by tau and summed across the
        lanes by four rotations each: 61 instructions instead of 2 ns + 2 and ns / 2 LDS reads.)"""
        P, ns, TMP13, TAU = self.P, self.ns, self.TMP13, self.TAU
        assert ns + 2 <= len(TMP13)
        ACCA, ACCB = TMP13[ns], TMP13[ns + 1]
        P.mul_dpp(ACCA, TAU[s], TMP13[0], 0)
        if ns > 1:
            P.mul_dpp(ACCB, TAU[s], TMP13[1], 1)
        for k in range(2, ns):
            P.fmac_dpp(ACCA if k % 2 == 0 else ACCB, TAU[s], TMP13[k], k)
        if ns > 1:
            P.v("v_add_f32_e32 %s, %s, %s" % (ACCA, ACCB, ACCA), writes=(ACCA,), reads=(ACCA, ACCB))
        for i in range(ns):
            P.fmac_dpp(self.Q[s][i], ACCA, "%[eaff]", i)

    def save_value(self, s):
        """save: the value function of the step, [V_t | v_t] (row i of Q~ now: V_t[i][:] in lanes < nx, v_t[i] in lane aff), as
        rows of nx + 1 floats: what the one-pass gradient reads instead of C (lambda_t = V_t x_t + v_t, the `adj` form);
        then [Vv | Qxu | Quu] of the wave's four trajectories go out as whole chunks"""
        P, nx, Q, SVD = self.P, self.nx, self.Q, self.SVD
        P.uses(Q[s][:nx])
        with P.under_exec(S_KM):
            for i in range(nx):
                P.raw("ds_write_b32 %%[asv], %s offset:%d" % (Q[s][i], i * (nx + 1) * 4))
        for q in range(self.SV_NST):
            P.raw("ds_read_b128 %s, %%[ach] offset:%d" % (vrange(SVD[q]), q * 1024))
        P.raw("s_waitcnt lgkmcnt(0)")
        for q in range(self.SV_NST):
            P.store_part(self.SV_N - 64 * q, "global_store_dwordx4 %%[pso%d], %s, off" % (q, vrange(SVD[q])))
        for q in range(self.SV_NST):
            P.v("v_lshl_add_u64 %%[pso%d], %%[pso%d], 0, %%[sso%d]" % (q, q, q))

    def bstep(self, step, first, extra_outstanding=0):
        """step `step` of the sweep (0 is the peeled first step; the loop form passes its body position, the step modulo
        the loop length): register set step % 3, ring slot step % D"""
        P, L, D, nx, ns, aff, Q, F, W, G10, mfma = self.P, self.L, self.D, self.nx, self.ns, self.aff, self.Q, self.F, self.W, self.G10, self.mfma
        s, slot, nslot = step % 3, step % D, (step + 1) % D
        p, n = (s + 2) % 3, (s + 1) % 3
        V = Q[p]
        self.issue_group(self.ptr, slot, L.SLOT_B, gap="s_waitcnt lgkmcnt(0)")   # the slot's last reads are in before it is refilled
        self.advance(self.ptr, self.strd, by_steps_left=D if first else D + 1)
        if self.expand:
            self.recentre(s)
        if self.affine:
            pass    # (all of the step's arithmetic comes after the reads of the next step have been issued: gains_affine)
        elif not first and mfma:
            # Q~ += F~^T V^ F^ as (V^^T F^)^T F^ - both products have the A^T B shape that an outer-product MFMA
            # computes from column-per-lane registers (A operand = 4 lanes of a register = 4 rows of A^T):
            #   G[b][j]  = sum_a V[a][b] F~[a][j]      rows b = x columns: tiles of 4, A = V[a] block b/4, B = F~[a]
            #   g1[j]    = sum_a v[a] F~[a][j]         the row of the homogeneous coordinate (8 DPP FMAs)
            # This is the reference's own association, (F^T V) F  (lqr_recursion.py:89,96).
            if not self.K.g10_mix:
                P.mul_dpp(G10, V[0], F[s][0], aff)
                for a_ in range(1, nx):
                    P.fmac_dpp(G10, V[a_], F[s][a_], aff)
            for a_ in range(nx):
                for I in range(nx // 4):
                    Gt = W[4 * I:4 * I + 4]
                    P.mfma(Gt, V[a_], F[s][a_], Gt if a_ else None, I)
                if self.K.g10_mix:     # the g1 FMAs sit between dependent accumulations of the same tile
                    if a_ == 0:
                        P.mul_dpp(G10, V[0], F[s][0], aff)
                    else:
                        P.fmac_dpp(G10, V[a_], F[s][a_], aff)
        elif not first:
            # W~ = V~ F~  (+ v in column aff):  W[i] = sum_k bcast<k>(V[i]) F[k] + bcast<aff>(V[i]) e_aff
            for i in range(nx):
                P.mul_dpp(W[i], V[i], F[s][0], 0)
            for k in range(1, nx):
                for i in range(nx):
                    P.fmac_dpp(W[i], V[i], F[s][k], k)
            for i in range(nx):
                P.fmac_dpp(W[i], V[i], "%[eaff]", aff)
        # The stores of a step (gains, the saved blocks) are younger than its DMA group and retire in order with it
        # (one counter, gfx9): between the group this step needs and now lie D-1 younger groups AND the stores of the
        # D-1 steps since - allowing for them keeps D-1 groups in flight (without, eleven stores per step would leave
        # one).  Body positions j < D-1 also run step j of the sweep, where only j steps' stores and the prologue's
        # extra loads lie in between: the smaller of the two counts.
        st_allow = 0
        if not first and not self.mpc and self.n_step_stores:
            st_allow = (D - 1) * self.n_step_stores
            if step <= D - 2:
                st_allow = step * self.n_step_stores + min(self.n_extra, (D - 1 - step) * self.n_step_stores)
        self.vmwait((D - 1) * self.NDB_ALL + extra_outstanding + st_allow)
        self.read_set(n, nslot)
        if self.stash:
            # F of the NEXT step goes from its ring slot into this step's stash registers: the register numbers
            # differ per step, so the two reads live in a table of stubs (one per step) that is called here
            lo = sgpr_lo(S_STUB)
            if self.K.ret_direct:
                site = self.callsites.next()
                P.raw("s_setpc_b64 " + S_STUB)
                P.align(6)
                P.label("Lret%d_%%=" % site, reset=False)
                self.bret["first" if first else step] = site
            else:
                P.raw("s_swappc_b64 %s, %s" % (S_RET, S_STUB))
            P.raw("s_add_u32 s%d, s%d, %d" % (lo, lo, BSTUB))
            P.raw("s_addc_u32 s%d, s%d, 0" % (lo + 1, lo + 1))
        if self.affine:
            self.gains_affine(s, first)
            return
        if not first and mfma:
            #   Q~[i][j] += sum_b G[b][i] F~[b][j] + g1[i] e_aff[j]    tiles of 4 rows i: A = G[b] block i/4, B = F~[b]
            for b_ in range(nx):
                for I in range(self.NQ // 4):
                    Qt = Q[s][4 * I:4 * I + 4]
                    P.mfma(Qt, W[b_], F[s][b_], Qt, I)
            for I in range(self.NQ // 4):
                Qt = Q[s][4 * I:4 * I + 4]
                P.mfma(Qt, G10, "%[eaff]", Qt, I)
        elif not first:
            # Q~ += F~^T W~ ; the u-rows first in the last pass so that the Quu broadcasts need no wait states
            for k in range(nx):
                order = list(range(ns)) if k < nx - 1 else list(range(nx, ns)) + list(range(nx))
                for i in order:
                    P.fmac_dpp(Q[s][i], F[s][k], W[k], i)
        self.gains(s, first)
        if self.expand:
            self.read_ct(nslot)   # (the last step reads a slot nobody consumes)
        self.vupdate(s)
        if self.save:
            self.save_value(s)

    # =============================================================== prologue, issue_first, the backward loop
    def issue_first(self):
        """The first D groups are issued by a SEPARATE asm block (issue_first) that the C++ side runs as soon as the
        DMA pointers exist - the rest of the operand set-up then overlaps their flight."""
        with self.emitting(self.P.fresh()) as p:
            p.raw("s_sub_i32 %s, %%[T], 1" % S_TF)
            self.issue_group(self.ptr, 0, self.L.SLOT_B)
            self.advance(self.ptr, self.str1)
            for j in range(1, self.D):
                self.issue_group(self.ptr, j, self.L.SLOT_B)
                self.advance(self.ptr, self.strd)
        return p

    def prologue(self):
        """masks and constants, the loads behind the first groups (all of f, x_init), the zero fill of the gain rows, the
        first slot into register set 0; leaves n_extra: the loads younger than the first groups"""
        P, L, nx, nu, ns, aff, W, mpc, stash = self.P, self.L, self.nx, self.nu, self.ns, self.aff, self.W, self.mpc, self.stash
        P.comment("---- prologue (the first DMA groups are already in flight)")
        P.raw("s_waitcnt lgkmcnt(0)")
        self.stamp(0)
        for pair, lanes in self.lane_masks:
            P.load_mask(pair, lanes)
        for m in range(nu):
            P.v("v_mov_b32_e32 %s, 0" % self.Kt[m], writes=(self.Kt[m],))
        P.v("v_mov_b32_e32 %s, 0x7f7fffff" % self.MINPIV, writes=(self.MINPIV,))
        if self.ghbm:
            P.load_mask(S_GM, range(ns + 1))
        if self.save:
            P.load_mask(S_ROW0, [0])
        if self.affine:
            P.load_mask(S_AFF, [aff])
        if mpc:
            for r_ in self.XK + [self.NQP, self.QINFO]:
                P.v("v_mov_b32_e32 %s, 0" % r_, writes=(r_,))
            P.load_mask(S_AFF, [aff])
        elif self.masked:
            P.v("v_mov_b32_e32 %s, 0x322bcc77" % self.EPS, writes=(self.EPS,))   # 1e-8f (active_constrained_lqr.py:121-122)
        if stash:
            lo = sgpr_lo(S_STUB)
            P.raw("s_getpc_b64 " + S_STUB)
            P.label("Lpcb_%=", reset=False)
            P.raw("s_add_u32 s%d, s%d, Lbstub_%%=-Lpcb_%%=" % (lo, lo))
            P.raw("s_addc_u32 s%d, s%d, 0" % (lo + 1, lo + 1))
        self.n_extra = 0
        if stash and not self.adj:
            # all of f (the forward sweep's only input from memory) goes to LDS now, BEHIND the first groups: the
            # backward sweep's first two waits allow for these NFD younger operations, later ones are merely conservative
            self.n_extra = L.NFD
            for q in range(L.NFD):
                if q == 0:
                    P.raw("s_mov_b32 m0, %[farea]")
                else:
                    P.raw("s_add_u32 m0, %%[farea], %d" % (q * 1024))
                P.nop(1)
                P.raw("global_load_lds_dwordx4 %s, off" % self.fp[q])
        P.raw("global_load_dword %s, %%[pxi], off" % self.XV0)
        self.n_extra += 1
        # zero this wave's gain rows while the first slots are in flight (columns nx..ns-1 and the pad of every row
        # are never written afterwards; the region is padded to whole 1 KB pieces by lqr_asm_kernel.hpp)
        if not mpc and not self.ghbm:
            for i in range(4):
                P.v("v_mov_b32_e32 %s, 0" % W[i], writes=(W[i],))
            P.raw("s_mov_b32 %s, %%[nz]" % S_TMP)
            P.label("Lzero_%=", reset=False)
            P.raw("ds_write_b128 %%[gz], %s" % vrange(W[0:4]))
            P.v("v_add_u32_e32 %[gz], 0x400, %[gz]")
            P.raw("s_sub_u32 %s, %s, 1" % (S_TMP, S_TMP))
            P.raw("s_cmp_lg_u32 %s, 0" % S_TMP)
            P.raw("s_cbranch_scc1 Lzero_%=")
        if stash and self.K.warm_stubs and not self.K.ret_direct:
            P.raw("s_mov_b64 s[82:83], %s" % S_STUB)
            P.raw("s_mov_b32 %s, %d" % (S_TMP, L.NSTASH))
            P.label("Lwarm_%=", reset=False)
            P.raw("s_swappc_b64 %s, s[82:83]" % S_RET)
            P.raw("s_add_u32 s82, s82, %d" % BSTUB)
            P.raw("s_addc_u32 s83, s83, 0")
            P.raw("s_sub_u32 %s, %s, 1" % (S_TMP, S_TMP))
            P.raw("s_cmp_lg_u32 %s, 0" % S_TMP)
            P.raw("s_cbranch_scc1 Lwarm_%=")
        P.raw("s_waitcnt vmcnt(%d)" % ((self.D - 1) * self.NDB_ALL + self.n_extra))
        self.read_set(0, 0)
        if self.expand:
            self.read_ct(0)
        P.raw("s_sub_i32 %s, %%[T], 2" % S_N)      # steps left after the first, minus one

    def backward_loop(self):
        """the peeled step t = T-1, then one form of the sweep: the loop over lcm(register sets, ring slots) steps"""
        P, LC = self.P, self.LC
        P.comment("---- t = T-1")
        self.stamp(1)
        self.bstep(0, True, self.n_extra)
        if self.K.skip_bwd:
            P.raw("s_branch Lbwd_done_%=")
        self.in_loop = True
        P.label("Lbwd_%=")
        for k in range(1, LC + 1):       # steps k, k + LC, k + 2 LC, ... of the sweep
            P.comment("---- backward step, register set %d, ring slot %d" % (k % 3, k % self.D))
            self.bstep(k, False)
            P.raw("s_sub_u32 %s, %s, 1" % (S_N, S_N))       # SCC = borrow: that was the last step
            if k != LC:
                P.raw("s_cbranch_scc1 Lbwd_done_%=")
            else:
                P.raw("s_cbranch_scc0 Lbwd_%=")
        P.label("Lbwd_done_%=")
        self.in_loop = False
        self.n_bwd = P.n_instr
        if self.mpc:      # backward sweep only
            P.v("v_mov_b32_e32 %[xvout], 0")
            P.v("v_mov_b32_e32 %%[nqp], %s" % self.NQP)
            P.v("v_mov_b32_e32 %%[qpinfo], %s" % self.QINFO)
            P.raw("s_branch Ldone_%=")

    def emit_backward(self):
        self.P_first = self.issue_first()
        self.prologue()
        self.backward_loop()

    def finish(self):
        P = self.P
        P.label("Ldone_%=")
        P.v("v_mov_b32_e32 %%[minpiv], %s" % self.MINPIV)
        P.raw("s_waitcnt vmcnt(0) lgkmcnt(0)")
        self.stamp(3)
        for i in range(len(self.TS)):
            P.v("v_mov_b32_e32 %%[ts%d], %s" % (i, self.TS[i]))
