// costate_common.hpp - what the co-state kernels (costate_kernels.hpp, costate_dma_kernel.hpp, costate_wide_kernel.hpp,
// costate_staged_kernel.hpp) have in common, written once: the dC weights, the per-step scalar stores, a lane's inputs of a
// step, and the slot layout of the two LDS-DMA ring kernels that give a wavefront four trajectories.
// Follows DiffLqr.backward, lqr/differentiable_lqr.py:85-134, and MPCstep.backward, mpc/mpc_step.py:383-446.
#pragma once
#include "costate_args.hpp"
#include "dma_gather.hpp"

namespace dmpc {

// dC_t = out_sign * (wa dtau (x) tau + wb tau (x) dtau)                     differentiable_lqr.py:128 / mpc_step.py (symmetric)
constexpr float kCostateWa = 0.5f;
__device__ __forceinline__ float costate_wb(int dC_mode) { return dC_mode == 0 ? 1.0f : 0.5f; }

// The per-step stores of element i of the co-state rows, by the lane (or loop iteration) that holds it; `on`: it is a live
// state row.  lam_out / dlam_out take the recursion's own values, df takes them times out_sign.
// ... before the update: lam, dlam are lambda_{t+1}, d_lambda_{t+1}
__device__ __forceinline__ void costate_store_before(const CostateArgs &a, int t, size_t tb, int nx, int i, bool on,
                                                     float /*lam*/, float dlam) {
  if (a.df != nullptr && a.df_shift == 1 && t < a.T - 1 && on) a.df[tb * nx + i] = a.out_sign * dlam;
}
// ... after it: lambda_t, d_lambda_t
__device__ __forceinline__ void costate_store_after(const CostateArgs &a, int t, size_t tb, int nx, int i, bool on, float lam,
                                                    float dlam) {
  if (a.df != nullptr && a.df_shift == 0 && t < a.T - 1 && on) a.df[tb * nx + i] = a.out_sign * dlam;
  if (a.lam_out != nullptr && on) a.lam_out[tb * nx + i] = lam;
  if (a.dlam_out != nullptr && on) a.dlam_out[tb * nx + i] = dlam;
}

// Inputs of one timestep as a lane of a group holds them: its element of tau and dtau, and (lanes < NX) row `lane` of C_t,
// c_t[lane], r_t[lane], column `lane` of F_t[:, :NX].
template <int NX, int NS>
struct CostateSlot {
  float tau, dtau, ci, ri;
  float Crow[NS], Fcol[NX];
};

// ---- The LDS-DMA ring of costate_dma_kernel and costate_wide_kernel: a wavefront owns four consecutive trajectories, so
// C, c, r, F, x, u, dx, du of one timestep are eight contiguous runs of HBM, which per-lane gather DMA (dma_gather.hpp) moves
// into a ring of DB slots.  (Each kernel builds its own gather table over this map: a shared builder cost them registers.)
// 16-byte chunks of one wave-step: [C | c | r | F | x | u | dx | du], each region at the size of the instance.  C_ROWS: the
// rows of C_t a trajectory brings - only the state rows enter the recursions (differentiable_lqr.py:92,102,115,124:
// C[:nx, :]), so NX where a trajectory's nx * ns floats are whole chunks, else NS.  SCR_: floats of output staging per wave.
template <int NX, int NU, int DB, int C_ROWS, int SCR_>
struct CostateRingLayout {
  static constexpr int NS = NX + NU, kNX = NX, kNU = NU, kCRows = C_ROWS;
  static_assert(C_ROWS == NS || (C_ROWS == NX && (NX * NS) % 4 == 0), "a trajectory's rows of C are whole 16-byte chunks");
  static constexpr int nC = C_ROWS * NS, nc = NS, nF = NX * NS;
  static constexpr int CH_C = 0, CH_c = CH_C + nC, CH_r = CH_c + nc, CH_F = CH_r + nc, CH_x = CH_F + nF;
  static constexpr int CH_u = CH_x + NX, CH_dx = CH_u + NU, CH_du = CH_dx + NX, CH_END = CH_du + NU;
  static constexpr int OFF_C = CH_C * 4, OFF_c = CH_c * 4, OFF_r = CH_r * 4, OFF_F = CH_F * 4, OFF_x = CH_x * 4;
  static constexpr int OFF_u = CH_u * 4, OFF_dx = CH_dx * 4, OFF_du = CH_du * 4;   // in floats
  static constexpr int kDma = (CH_END + 63) / 64;   // gather DMAs per step; padding lanes repeat chunk 0 of C
  static constexpr int SLOT = kDma * 256;           // floats per wave and timestep (whole 1 KB pieces)
  static constexpr int SCR = SCR_;
  static_assert((DB - 1) * kDma <= 63, "ring too deep for vmcnt");
};

}  // namespace dmpc
