#!/usr/bin/env python
"""Emit lqr_asm_gen.hpp: the fused LQR solve (Riccati backward sweep + rollout) of the 16-lane row layout as ONE
hand-scheduled gfx950 instruction stream per shape and form (gen_lqr_stream.py: Form says what each form computes).

Why a generator and why whole-kernel asm.  B = 4096 trajectories at four per wavefront is exactly one wavefront
per SIMD, and a lone wavefront issues one instruction every ~4.5 cycles whatever its type
(profiles/r01/microbench_valu_issue.txt: v_fmac 4.45, DPP 5.4, s_nop 4.45).  The kernel's time is therefore its
instruction count.  The HIP version (lqr_dma_kernel.hpp) spends 554 instructions per timestep of which only ~230
are arithmetic; the rest is exec-mask branching around partial DMA chunks, scalar address arithmetic, copies and
s_nops that hipcc puts around asm statements.  Here every instruction is chosen:

  * inputs of one timestep (C, c, F, f of the wave's four trajectories, 3168 B at (8,2)) arrive by FOUR full-width
    LDS-DMA instructions: each lane carries its own 64-bit source pointer (one 16-byte chunk of whichever array
    its position in the slot belongs to) which advances by that array's time stride - no partial chunks, no
    exec masks, no scalar pointer bookkeeping; M0 is written once per group and the instruction offset moves
    both the global and the LDS address;
  * three rotating register sets: the value function V of step t is accumulated IN PLACE in the x-rows of Q_t
    (no copies), while set t-1 is being filled by ds_read_b32 from the ring slot that the DMA of three steps ago
    has completed (counted vmcnt);
  * W = V [F|f] + [0|v] starts with v_mul_f32_dpp (no zero-init) and takes v from lane `aff` with one more DPP
    FMA against a constant unit vector; the 2x2 / 1x1 pivoted solve is spelled out (LAPACK getf2/getrs order,
    reciprocal pivots, one Newton step on v_rcp_f32); gain rows are written to LDS as [K_m | 0 | k_m | pad]
    under an exec mask that also keeps lanes nx..ns-1 of K~ at exactly 0 - which is what makes the in-place value
    update and the forward sweep's in-place control FMAs legal;
  * forward sweep: lane i < nx owns row i of [F_t | f_t] (ring slot), lane nx+m owns gain row m (same shape), so
    one stream of ds_read2_b64 + nx + nu DPP FMAs yields [x_{t+1} | u_t] in one register, stored by ONE
    global_store_dword through per-lane pointers.

The pieces: gen_asm_emit.py (emitter with the hazard tracker), gen_lqr_stream.py (knobs, layout, forms, the register
plan and the backward sweep), gen_lqr_rollout.py (the three rollouts), this file (operand lists and the C++ text).

    python chainer_differentiable_mpc_amd/csrc/gen_lqr_asm.py [--out PATH]    # rewrites lqr_asm_gen.hpp
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_asm_emit import VBASE   # noqa: E402
from gen_lqr_rollout import emit_rollout   # noqa: E402
from gen_lqr_stream import KROW, SHAPES, Form, Knobs, LqrStream, forms_for   # noqa: E402,F401

OUT = os.path.join(HERE, "lqr_asm_gen.hpp")


def operands(st):
    """output, read-write and input operands and the clobber list of the stream's main block"""
    L, nx, nu, ns = st.L, st.nx, st.nu, st.ns
    outs = [("xvout", '"=&v"(xvout)'), ("minpiv", '"=&v"(minpiv)')]
    if st.mpc:
        outs += [("nqp", '"=&v"(nqp)'), ("qpinfo", '"=&v"(qpinfo)')]
    if st.TS:
        outs += [("ts%d" % i, '"=&v"(in.ts[%d])' % i) for i in range(4)]
    rw = []
    for q in range(L.ndma_b):
        rw.append(("ptr%d" % q, '"+v"(in.ptr[%d])' % q))
    NDA, NST = adj_counts(st)
    if not st.stash or st.adj:
        for q in range(NDA if st.adj else L.ndma_f):
            rw.append(("fptr%d" % q, '"+v"(in.fptr[%d])' % q))
    if st.adj:
        rw.append(("avp", '"+v"(in.avp)'))
        for q in range(NST):
            rw.append(("pso%d" % q, '"+v"(in.pso[%d])' % q))
    rw += [("tf", '"+s"(in.tf)'), ("gz", '"+v"(in.gz)'), ("ak", '"+v"(in.ak)'), ("arow", '"+v"(in.arow)'), ("aaff", '"+v"(in.aaff)'), ("pst", '"+v"(in.pst)')]
    if st.write_k:
        for m in range(nu):
            rw.append(("pk%d" % m, '"+v"(in.pk[%d])' % m))
    if st.ghbm:
        rw.append(("pgw", '"+v"(in.pgw)'))
    if st.masked:
        rw.append(("pm", '"+v"(in.pm)'))
    if st.save:
        for q in range(st.SV_NST):
            rw.append(("pso%d" % q, '"+v"(in.pso[%d])' % q))
    ins = []
    for q in range(L.ndma_b):
        ins.append(("str1_%d" % q, '"v"(in.str1[%d])' % q))
        ins.append(("str%d" % q, '"v"(in.str[%d])' % q))
    for i in range(4 if st.affine else ns):
        ins.append(("aq%d" % i, '"v"(in.aq[%d])' % i))
    for k in range(nx):
        ins.append(("af%d" % k, '"v"(in.af[%d])' % k))
    ins += [("eaff", '"v"(in.eaff)'), ("dst", '"v"(in.dst)'), ("pxi", '"v"(in.pxi)'), ("px0", '"v"(in.px0)')]
    if st.stash:
        for q in range(L.NFD):
            ins.append(("fp%d" % q, '"v"(in.fp[%d])' % q))
        for q in range(st.D):
            ins.append(("sr%d" % q, '"v"(in.sr[%d])' % q))
        ins += [("drowo", '"v"(in.drow)'), ("daff", '"v"(in.daff)'),
                ("farea", '"s"(in.farea)')]
    else:
        for q in range(L.ndma_f):
            ins.append(("fstr%d" % q, '"v"(in.fstr[%d])' % q))
        ins += [("drow", '"v"(in.drow)'), ("drow2", '"v"(in.drow2)'), ("daff", '"v"(in.daff)'), ("daff2", '"v"(in.daff2)')]
    if st.adj:
        for q in range(NDA):
            ins.append(("fstr%d" % q, '"v"(in.fstr[%d])' % q))
        for q in range(NST):
            ins.append(("sso%d" % q, '"v"(in.sso[%d])' % q))
        for q in range(4):
            ins.append(("avr%d" % q, '"v"(in.avr[%d])' % q))
        ins += [("atx", '"v"(in.atx)'), ("awc", '"v"(in.awc)'), ("awe", '"v"(in.awe)'), ("awf", '"v"(in.awf)'),
                ("awd", '"v"(in.awd)'), ("ach", '"v"(in.ach)'), ("wa", '"v"(in.wa)'), ("wb", '"v"(in.wb)'),
                ("dfshift", '"v"(in.dfshift)')]
    if st.write_k:
        ins.append(("dk", '"v"(in.dk)'))
    if st.ghbm:
        ins.append(("dgw", '"v"(in.dgw)'))
        for q in range(L.ndma_f):
            ins.append(("fstrl%d" % q, '"v"(in.fstrl[%d])' % q))
    if st.save:
        for q in range(st.SV_NST):
            ins.append(("sso%d" % q, '"v"(in.sso[%d])' % q))
        ins += [("asv", '"v"(in.asv)'), ("asq", '"v"(in.asq)'), ("asu", '"v"(in.asu)'), ("ach", '"v"(in.ach)')]
    if st.masked:
        ins += [("dm", '"v"(in.dm)'), ("am", '"v"(in.am)')]
    ins += [("ring", '"s"(in.ring)'), ("T", '"s"(in.T)'), ("nz", '"s"(in.nz)'), ("bwd_only", '"v"(in.bwd_only)')]
    if st.mpc:
        ins.append(("nqp_iter", '"s"(in.n_qp_iter)'))
    if st.expand:
        ins += [("atau", '"v"(in.atau)'), ("act", '"v"(in.act)')]
    clob = ['"v%d"' % i for i in range(VBASE, (255 if st.adj else st.last_vgpr) + 1)] + ['"a%d"' % i for i in range(st.n_agpr)] + \
        ['"s%d"' % i for i in ([70] + list(range(72, 102 if (st.mpc or st.affine) else (100 if (st.save or st.ghbm) else 98))))] + ['"vcc"', '"scc"', '"memory"']
    return outs, rw, ins, clob


def adj_counts(st):
    NDA = (st.nx * (st.nx + 1) + st.ns + 63) // 64     # adj: DMAs per group of [Vv | x | u]
    NST = (st.L.nchunk_b + 63) // 64                   # adj: store instructions per step
    assert NDA <= 2
    return NDA, NST


def first_operands(st):
    """read-write and input operands of block 1: the first D groups"""
    rw1 = [("ptr%d" % q, '"+v"(in.ptr[%d])' % q) for q in range(st.L.ndma_b)] + [("tf", '"+s"(in.tf)')]
    if st.masked:
        rw1.append(("pm", '"+v"(in.pm)'))
    ins1 = []
    for q in range(st.L.ndma_b):
        ins1.append(("str1_%d" % q, '"v"(in.str1[%d])' % q))
        ins1.append(("str%d" % q, '"v"(in.str[%d])' % q))
    if st.masked:
        ins1.append(("dm", '"v"(in.dm)'))
    ins1 += [("ring", '"s"(in.ring)'), ("T", '"s"(in.T)')]
    return rw1, ins1


def asm_block(o, lines, operand_lists, clobbers):
    o.append("    asm volatile(\n")
    for ln in lines:
        o.append('        "%s\\n\\t"\n' % ln)
    for ops in operand_lists:
        o.append("        : " + ", ".join("[%s] %s" % x for x in ops) + "\n")
    o.append("        : " + clobbers + ");\n")
    o.append("  }\n")


def struct_text(st):
    """the C++ specialisation around an emitted stream"""
    L, nx, nu = st.L, st.nx, st.nu
    outs, rw, ins, clob = operands(st)
    o = []
    o.append("// (%d,%d) write_k=%d stash=%d masked=%d: %d instructions in prologue + 4 backward steps, %d in %d unrolled forward steps\n"
             % (nx, nu, st.write_k, st.stash, st.masked, st.n_bwd, st.n_fwd, st.n_fwd_steps))
    o.append("template <>\nstruct %s {\n" % st.form.struct_name(nx, nu))
    o.append("  static constexpr bool kAvailable = true;\n")
    o.append("  static constexpr int NDB = %d, NDF = %d, SLOT_B = %d, SLOT_F = %d, RING_BYTES = %d, KROW = %d, DEPTH_F = %d, DEPTH_B = %d;\n"
             % (L.ndma_b, L.ndma_f, L.SLOT_B, L.SLOT_F, L.RING, KROW, L.DF, st.D))
    o.append("  static constexpr int OFF_C = %d, OFF_c = %d, OFF_F = %d, OFF_f = %d, FOFF_f = %d, FOFF_G = %d;\n"
             % (L.OFF_C, L.OFF_c, L.OFF_F, L.OFF_f, L.FOFF_f, L.FOFF_G))
    o.append("  static constexpr int NSTASH = %d, NFD = %d, FAREA_BYTES = %d, HROW = %d, SPD = %d, PADM = %d;\n"
             % (L.NSTASH, L.NFD, L.FAREA, L.H, L.SPD, 16 * L.nchunk_b))
    if st.adj:
        NDA, NST = adj_counts(st)
        o.append("  static constexpr int ADJ_NDA = %d, ADJ_SLOT = %d, ADJ_NST = %d;\n" % (NDA, NDA * 1024, NST))
    if st.save:
        o.append("  static constexpr int SAVE_STAGE_BYTES = %d, SAVE_NST = %d;\n" % (16 * st.SV_N, st.SV_NST))
    o.append("  static __device__ __forceinline__ void issue_first(LqrAsmIn<%d, %d> &in) {\n" % (nx, nu))
    asm_block(o, st.P_first.text(), first_operands(st), '"scc", "memory"')
    o.append("  static __device__ __forceinline__ void run(LqrAsmIn<%d, %d> &in, float &xvout, float &minpiv%s) {\n"
             % (nx, nu, ", int &nqp, int &qpinfo" if st.mpc else ""))
    asm_block(o, st.P.text(), (outs + rw, ins), ", ".join(clob))
    o.append("};\n\n")
    return "".join(o)


def gen_kernel(nx, nu, form, knobs):
    """the specialisation of shape (nx, nu) and `form`: backward sweep, rollout, the C++ text around them"""
    st = LqrStream(nx, nu, form, knobs)
    st.emit_backward()
    emit_rollout(st)
    st.finish()
    return struct_text(st)


HEADER = """// lqr_asm_gen.hpp - GENERATED by gen_lqr_asm.py; do not edit.
// Whole-kernel gfx950 instruction streams of the fused LQR solve (lqr/lqr_recursion.py:69-209 of the reference),
// 16-lane row layout, one per (nx, nu, write_k, stash).  The C++ side that prepares the per-lane operands is
// lqr_asm_kernel.hpp.
#pragma once
#include <cstdint>

namespace dmpc {

// per-lane operands of the instruction stream (see lqr_asm_kernel.hpp for how they are filled)
template <int NX, int NU>
struct LqrAsmIn {
  static constexpr int NS = NX + NU;
  // backward sweep
  uint64_t ptr[4], str1[4], str[4];  // LDS-DMA source of this lane's chunk (t = T-1), first / later time strides
  unsigned aq[NS], af[NX];           // LDS byte addresses (ring slot 0) of this lane's [C|c] rows and [F|f] rows
  unsigned ak;                       // LDS byte address of gain row (T-1, 0), this lane's column
  unsigned gz;                       // LDS byte address of this wave's gain rows + lane64 * 16 (zero fill)
  int nz;                            // wave-uniform: 1 KB pieces of the gain rows of one wave
  int tf;                            // wave-uniform: time strides the DMA pointers may still take (set by issue_first)
  int bwd_only;                      // 1 = stop after the backward sweep (LqrRecursion.backward()); same in every lane
  float eaff;                        // 1 in lane `aff`, else 0
  uint64_t pk[NU], dk;               // Ks/ks store pointers (t = T-1) and their time stride (write_k)
  uint64_t pgw, dgw;                 // ghbm: store pointer of column min(lane, ns) of gain row (T-1, 0) in the workspace, time stride
  // save: [Vv | Qxu | Quu] leave through a staging area (LDS byte addresses of: column min(lane, nx) of row 0 of this
  // trajectory's [V | v] - lane ns is column nx -, column lane - nx of row 0 of Qxu, Quu) as 16-byte chunks: pso / sso / ach
  unsigned asv, asq, asu;
  uint64_t pm, dm;                   // masked: DMA source of this lane's dword of clamped-control flags, time stride
  unsigned am;                       // masked: LDS byte address (ring slot 0, without the padding offset) of this row's flags
  int n_qp_iter;                     // mpc (wave-uniform): iteration cap of the box QP
  unsigned act;                      // mpc, expand: LDS byte address (ring slot 0) of row min(lane, ns-1) of this trajectory's C_t
  unsigned atau;                     // mpc, expand: LDS byte address (ring slot 0, without the padding offset) of [x_t; u_t][lane]
  // forward sweep
  uint64_t fptr[2], fstr[2];         // ring variant: DMA source of this lane's [F|f] chunk (t = 0) and time stride
  uint64_t fstrl[2];                 // ghbm: stride of the LAST step (T-2 -> T-1): that of the gain lanes, 0 for F / f
  uint64_t fp[8];                    // stash variant: DMA sources of all of f (issued in the prologue)
  unsigned sr[6];                    // stash variant: LDS byte address of this lane's half row of F in ring slot q < DEPTH_B
  unsigned farea;                    // stash variant (wave-uniform): LDS byte address of this wave's f area
  unsigned arow, aaff, drow, drow2, daff, daff2;
  uint64_t pst, dst;                 // [x_{t+1} | u_t] store pointer and time stride
  uint64_t pxi, px0;                 // &x_init[b][lane] (every lane valid), &x[0][b][lane] (lanes < nx store)
  // wave-uniform
  unsigned ring;                     // LDS byte address of this wave's ring
  int T;
  unsigned ts[4];                    // GEN_TIMING builds only: s_memtime at the phase boundaries
  // adj (the one-pass gradient; fptr / fstr carry the DMA sources of [Vv | x | u], walking forward in time)
  unsigned avp;                      // LDS byte address of v'_{T-1}[lane] in the f area (lanes < nx), moves back per step
  unsigned avr[4];                   // LDS byte address of row min(lane, nx-1) of this trajectory's [V | v] in ring slot q
  unsigned atx;                      // ... of [x; u][min(lane, ns-1)] in ring slot 0
  unsigned awc, awe, awf, awd;       // staging area (without its ring offset): column `lane` of row 0 of dC / dc / dF, df[lane]
  unsigned ach;                      // staging area + lane64 * 16: this lane's chunk (adj: without the area's ring offset)
  uint64_t pso[4], sso[4];           // store pointer of this lane's chunk (adj: of [dC | dc | dF | df] at t = 0), time stride
  float wa, wb;                      // dC = wa dtau (x) tau + wb tau (x) dtau
  int dfshift;                       // 0: df[t] = d_lambda[t] (the reference), 1: d_lambda[t+1]
};

// GHBM (ring form, no gains out): the gain rows pass through a caller workspace in HBM instead of LDS - any horizon
// SAVE (with WRITE_K): Quu_t and Qxu_t of every step go to HBM as well (DiffLqr's training form)
// AFFINE (STASH, no gains out): the re-solve with saved K_t, Quu_t, Qxu_t and another c (DiffLqr.backward's second solve)
// ADJ (with AFFINE): DiffLqr.backward in one launch - the affine re-solve whose rollout writes dC, dc, dF, df, dx_init from
// [V_t | v_t] of the saving solve instead of C (see gen_kernel)
template <int NX, int NU, bool WRITE_K, bool STASH, bool MASKED = false, bool GHBM = false, bool SAVE = false, bool AFFINE = false,
          bool ADJ = false>
struct LqrAsm {
  static constexpr bool kAvailable = false;
};

// MPCstep.backward_rec: backward sweep with the box QP in the stream (gains to HBM, no rollout); EXPAND: with the
// Taylor re-centring of c (need_expand) in the sweep
template <int NX, int NU, bool EXPAND>
struct MpcAsm {
  static constexpr bool kAvailable = false;
};

"""


def header_text(knobs):
    """the whole of lqr_asm_gen.hpp under `knobs`"""
    out = [HEADER.replace("#pragma once\n", "#pragma once\n#define DMPC_ASM_TIMING_GEN 1\n") if knobs.timing else HEADER]
    for nx, nu in SHAPES:
        for form in forms_for(nx, nu, knobs):
            out.append(gen_kernel(nx, nu, form, knobs))
    out.append("}  // namespace dmpc\n")
    return "".join(out)


def main(argv):
    out = argv[2] if len(argv) > 2 and argv[1] == "--out" else OUT
    with open(out, "w") as fh:
        fh.write(header_text(Knobs.from_env(os.environ)))
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv)
