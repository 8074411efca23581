// line_search.hpp - what the kernels of MPCstep.forward_rec (mpc/mpc_step.py:175-286: the clamped rollout and its backtracking
// search) have in common, written once: their arguments, the clamp onto the box, the terms a row of the cost adds, the
// sequential search's state and decision, and the epilogue (cap hit, flags, the per-trajectory stores).  The kernels:
// mpc_forward_rec_kernel, the pendulum's two speculative searches (mpc_kernels.hpp), mpc_forward_asm_body
// (mpc_fwd_asm_kernel.hpp; its generated stream emits a clamp of its own), mpc_wide_forward_kernel, mpc_generic_forward_kernel
// and mpc_staged_forward_kernel (mpc_generic.hpp), mpc_tiled_forward_kernel, mpc_forward_rec_mlp_kernel.
// A kernel keeps what is its own: where a timestep's inputs come from, how its lanes share the rows, the order of its sums.
#pragma once
#include <cstdint>
#include "../../include/dmpc.h"   // DMPC_INFO_*
#include "colwise.hpp"            // is_finite

namespace dmpc {

struct MpcFwdArgs {
  int T, B;
  const float *Ks, *ks;                  // gains from backward_rec
  const float *controls, *states;        // current iterate  [T,B,nu], [T,B,nx]
  const float *lower, *upper;            // absolute control bounds [T,B,nu]
  const float *C, *c, *F, *f;            // TRUE QuadCost / LinDx (f may be nullptr)
  float ls_decay;
  int max_ls_iter;                       // only guards the first pass in the reference (:196), kept for the record
  int ls_cap;                            // safety cap on line-search passes (the reference loop is unbounded)
  float *x, *u;                          // new trajectory
  float *u_first;                        // controls of the first (alpha = 1) pass, or nullptr      (:260-263)
  float *costs, *old_costs, *alphas;     // [B]
  float *objs;                           // [T,B] per-step cost of the accepted pass, or nullptr
  int32_t *n_ls;                         // [B] passes run
  int32_t *info;
  // TRUE dynamics other than LinDx, evaluated inside the line search (mpc_step.py:237-240 calls a Python callable):
  //   0 LinDx (F, f above)   1 the pendulum of env_dx/pendulum.py:65-102, simple model (nx = 3, nu = 1)
  int dyn_kind;
  float pend_g, pend_m, pend_l, pend_dt, pend_max_torque;
  int pend_clamp_closed;                 // derivative of the torque clamp at its limits (PendulumModel::clamp_grad)
  const int32_t *done;                   // device flag of the BoxDDP loop: non-zero -> no-op
  // The accepted trajectory IS the next iLQR iteration's nominal one (BoxDDP re-rolls it with get_traj and linearises
  // it, mpc/box_ddp.py:123-136): the speculative pendulum search can write that model while it writes the
  // trajectory - F_next [T-1,B,3,4], f_next [T-1,B,3], c_next [T,B,4] = C tau + c (mpc_step.py:305-317); nullptr = no.
  float *F_next, *f_next, *c_next;
  // speculative search: every candidate keeps its trajectory in LDS (T * 4 floats per lane, T * 4 KB per workgroup)
  // and the accepted one is copied out instead of being rolled out a second time; 0 = no such buffer was given
  int traj_in_lds;
  const int32_t *info_in;                // [B] flags to merge into info (the backward sweep's, when it ran ahead of `done`)
  int nx_log = 0, nu_log = 0;            // container launches (PAD): the problem's own dimensions
  int info_store = 0;                    // != 0: info[b] = this search's flags (plain store; pendulum spec4 search only)
};

// ---- the clamp                                                                                          mpc_step.py:221
// "Sits on its bound": the reference tests |u - bound| <= 1e-8 in float64 (mpc_step.py:363-364), where a
// clamped control differs from its bound by at most an ulp (1e-16).  In float32 an ulp at |bound| ~ 1 is
// 6e-8, so the same test needs a tolerance of a few float32 ulps; controls that close are also snapped
// onto the bound by the rollout so that `u == bound` holds exactly for callers.
__device__ __forceinline__ float bound_tol(float bound) { return 1e-8f + 4.0f * 1.1920929e-07f * fmaxf(1.0f, fabsf(bound)); }

__device__ __forceinline__ bool on_bound(float u, float bound) { return fabsf(u - bound) <= bound_tol(bound); }   // :363-364

__device__ __forceinline__ float box_clamp(float v, float lb, float ub) {
  v = fminf(fmaxf(v, lb), ub);                                                                             // :221
  v = (v - lb <= bound_tol(lb)) ? lb : v;
  return (ub - v <= bound_tol(ub)) ? ub : v;
}

// ---- what row i of the cost 1/2 tau'C tau + c'tau adds (:246-251, util.py:162-198), with q = (C v)[i] for the v named.
// The test `current_cost > OLD_COST` (:196,266) is NOT taken on the two rounded totals: near a fixed point their
// difference is far below float32's resolution of the totals (the reference decides it in float64).  Per timestep
//     obj(tau') - obj(tau) = 1/2 d'(C tau') + 1/2 tau'(C d) + c'd ,   d = tau' - tau
// is exact algebra for any (also non-symmetric) C and has no cancellation: its rounding error scales with |d|, not
// with the cost.  A candidate that has collapsed onto the nominal trajectory gives d = 0, hence exactly 0.
// ... to the cost of v (the candidate; the iterate too, in the kernels that form C tau0 as a product of its own: generic,
// staged, tiled, mlp)
__device__ __forceinline__ float cost_row(float v_i, float q_i, float c_i) { return v_i * fmaf(0.5f, q_i, c_i); }
// ... to the cost of the iterate tau0 from C tau0 = C tau' - C d (row, wide, spec4: no third product)              :191
__device__ __forceinline__ float cost_row_iterate(float tau0_i, float q_i, float qd_i, float c_i) {
  return tau0_i * fmaf(0.5f, q_i - qd_i, c_i);
}
// ... to obj(tau') - obj(tau0): d_i = tau'_i - tau0_i, q_i = (C tau')[i], qd_i = (C d)[i]
__device__ __forceinline__ float cost_row_diff(float d_i, float q_i, float c_i, float tau0_i, float qd_i) {
  return fmaf(d_i, fmaf(0.5f, q_i, c_i), 0.5f * tau0_i * qd_i);
}

// ---- the sequential search: one pass per step size, alpha = ls_decay^p, until a pass is not worse           :196-268
struct LineSearch {
  float alpha = 1.0f;
  int n_pass = 0;
  bool worse = true;    // the last pass cost more than the iterate (before the first: search)
  // another pass?  Also the start condition (no pass at all under a cap of 0).                                :196
  __device__ __forceinline__ bool searching(int cap) const { return worse && n_pass < cap; }
  // a pass has ended with delta = current_cost - OLD_COST
  __device__ __forceinline__ void advance(float delta, float decay) {
    ++n_pass;
    worse = delta > 0.f;                 // :266  current_cost > OLD_COST
    if (worse) alpha *= decay;           // :268
  }
};

// ---- the epilogue.  Cap hit: the reference would still be looping; its last pass is the result, at the step size that
// pass ran with - as the reference forms it, decayed (:268) and divided again (:274), which need not round back.  By what
// the kernel holds at that point:
// ... the sequential kernels and the stream's wrapper: alpha already decayed once more after the last pass
__device__ __forceinline__ float cap_alpha_sequential(float alpha_next, float decay) { return alpha_next / decay; }
// ... the two speculative kernels: the last candidate's own alpha
__device__ __forceinline__ float cap_alpha_speculative(float alpha_last, float decay) { return (alpha_last * decay) / decay; }

__device__ __forceinline__ int search_flags(bool cap_hit, float cost) {
  int bits = 0;
  if (cap_hit) bits |= DMPC_INFO_LS_ITERCAP;
  if (!is_finite(cost)) bits |= DMPC_INFO_NONFINITE;
  return bits;
}

// The results of trajectory b, by the one lane that holds them.  MERGE_IN: a.info_in[b] joins the flags.  PLAIN_STORE:
// a.info_store is honoured (info[b] = flags, zero included) - otherwise the flags are or-ed into info[b].
template <bool MERGE_IN, bool PLAIN_STORE>
__device__ __forceinline__ void search_store(const MpcFwdArgs &a, int b, float cost, float old_cost, float alpha, int n_pass,
                                             int flags) {
  if constexpr (MERGE_IN) {
    if (a.info_in != nullptr) flags |= a.info_in[b];
  }
  a.costs[b] = cost;
  if (a.old_costs != nullptr) a.old_costs[b] = old_cost;
  a.alphas[b] = alpha;
  a.n_ls[b] = n_pass;
  if constexpr (PLAIN_STORE) {
    if (a.info != nullptr) {
      if (a.info_store) a.info[b] = flags;
      else if (flags != 0) atomicOr(&a.info[b], flags);
    }
  } else {
    if (a.info != nullptr && flags != 0) atomicOr(&a.info[b], flags);
  }
}

}  // namespace dmpc
