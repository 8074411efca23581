// episode_kernels.hpp - the step between two solves of a closed-loop (receding-horizon) MPC episode, dmpc_mpc_episode of
// include/dmpc_episode.h: after a box-DDP solve from x_k ONE launch applies the plan's first control to the plant, logs the
// step and hands the next solve its state and its warm start -
//
//     u_k = u_best[0]        x_{k+1} = plant(x_k, u_k)       stage_cost[k] = 1/2 tau^T C[0] tau + c[0]^T tau,  tau = [x_k; u_k]
//     x_log[k+1] = x_cur = x_{k+1}    u_log[k] = u_k    state_log[k] = the solve's loop state    info |= the solve's flags
//     u_warm[t] = u_best[t+1] (t < T-1),  u_warm[T-1] = u_best[T-1]                    the plan shifted by one, its last control held
//
// The plant (PLANT) is evaluated by the step function of the kernel that rolls that kind of dynamics out, so a step here has
// the bits of that kernel's T = 2 rollout:
//     0  linear, time-invariant: lin_step_row (box_ddp_kernels.hpp), row i in lane i
//     1  the simple pendulum: pendulum_model / pendulum_next (mpc_kernels.hpp), every lane on the same four scalars
//     2  an MlpDx: MlpNet<DEPTH>::next<ACT> on weights staged by MlpNet::stage (mlp_dx_kernels.hpp) - no Jacobian, no slice
//
// Layout: mlp_rollout_linearize_kernel's - ONE wavefront per trajectory, four per workgroup, element i of tau in lane i
// (nx + nu <= 64).  The stage cost is the t = 0 term of the line search's cost: lane j forms row j of C tau in ascending
// order, cost_row, one wave_sum64.  No atomics (the lane that owns trajectory b owns info[b]), plain stores, no barrier behind
// the staging one; a wavefront without a trajectory returns behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// The kernel headers define the non-template kernels of mpc_api.hip's and mlp_dx_api.hip's translation units; here, as in
// mlp_dx_kernels.hpp, their functions get internal linkage: nothing is defined a second time, and what is not launched from
// this translation unit is not emitted.
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "mlp_dx_kernels.hpp"
#include "box_ddp_kernels.hpp"
#pragma clang attribute pop

namespace dmpc {

constexpr int kEpisodeMaxNs = 64;    // element i of tau lives in lane i

struct EpisodeAdvanceArgs {
  int T, B, nx, nu;
  int first;                           // step 0: info is written, not OR-ed into
  // the solve's results (the episode's workspace) and its stage cost at t = 0
  const float *x_k;                    // [B,nx] the state the solve started from
  const float *u_best;                 // [T,B,nu]
  const float *C, *c;                  // [T,B,ns,ns], [T,B,ns]: block t = 0 is read
  const int32_t *state, *info_step;    // [8], [B]
  // the plant
  const float *plant_F, *plant_f;      // PLANT 0: [B,nx,ns], [B,nx] or nullptr
  float pend_g, pend_m, pend_l, pend_dt, pend_max_torque;   // PLANT 1
  MlpModel m;                          // PLANT 2
  // what the step leaves
  float *x_first;                      // x_log[0] at step 0 (receives x_k), else nullptr
  float *x_next, *u_now, *stage_cost;  // x_log[k+1] [B,nx], u_log[k] [B,nu], stage_cost[k] [B]
  int32_t *state_now;                  // state_log[k] [8]
  int32_t *info;                       // [B] or nullptr
  float *x_cur, *u_warm;               // [B,nx], [T,B,nu]: the next solve's x_init and u_init
  const float *x_best;                 // [T,B,nx]
  float *x_plan, *u_plan;              // the last step: copies of x_best, u_best (each or nullptr)
};

template <int PLANT, int ACT, int DEPTH>
__global__ __launch_bounds__(64 * kMlpWaves) void episode_advance_kernel(const EpisodeAdvanceArgs a) {
  static_assert(PLANT >= 0 && PLANT <= 2, "plant kind");
  extern __shared__ float lds[];
  typename MlpNet<DEPTH>::Lds L;
  if constexpr (PLANT == 2) L = MlpNet<DEPTH>::stage(a.m, lds);     // (every thread of the workgroup; the only barrier)
  const int lane = threadIdx.x % 64;
  const int b = blockIdx.x * kMlpWaves + threadIdx.x / 64;
  if (b >= a.B) return;
  const int nx = a.nx, nu = a.nu, ns = nx + nu, T = a.T;
  const size_t B = (size_t)a.B;
  const bool is_x = lane < nx, is_u = lane >= nx && lane < ns;
  const float *xk = a.x_k + (size_t)b * nx, *uk = a.u_best + (size_t)b * nu;
  const float tau = is_x ? xk[lane] : (is_u ? uk[lane - nx] : 0.f);

  // stage cost: the t = 0 term of get_cost, as the searches form a timestep's cost
  {
    const int lt = lane < ns ? lane : 0;
    const float *Cr = a.C + ((size_t)b * ns + lt) * ns;
    float qi = 0.f;
    for (int j = 0; j < ns; ++j) qi = fmaf(Cr[j], lane_value(tau, j), qi);
    const float part = lane < ns ? cost_row(tau, qi, a.c[(size_t)b * ns + lt]) : 0.f;
    const float obj = wave_sum64(part);
    if (lane == 0) a.stage_cost[b] = obj;
  }

  // x_{k+1}: element `lane` (0 in lanes >= nx)
  float xn = 0.f;
  if constexpr (PLANT == 0) {
    const int i = is_x ? lane : 0;
    const float acc = lin_step_row(a.plant_F + (size_t)b * nx * ns, i, xk, uk, nx, nu,
                                   a.plant_f != nullptr ? a.plant_f[(size_t)b * nx + i] : 0.f);
    xn = is_x ? acc : 0.f;
  } else if constexpr (PLANT == 1) {
    const PendulumModel pm = pendulum_model(a.pend_g, a.pend_m, a.pend_l, a.pend_dt, a.pend_max_torque, 0);
    float cn, sn, nw, nth;
    pendulum_next(pm, xk[0], xk[1], xk[2], uk[0], cn, sn, nw, nth);
    xn = lane == 0 ? cn : (lane == 1 ? sn : (lane == 2 ? nw : 0.f));
  } else {
    MlpNet<DEPTH> net;
    xn = net.template next<ACT>(a.m, L, lane, tau);
  }

  if (is_x) {
    if (a.x_first != nullptr) a.x_first[(size_t)b * nx + lane] = tau;
    a.x_next[(size_t)b * nx + lane] = xn;
    a.x_cur[(size_t)b * nx + lane] = xn;
  }
  if (is_u) a.u_now[(size_t)b * nu + (lane - nx)] = tau;
  if (lane == 0 && a.info != nullptr) a.info[b] = (a.first ? 0 : a.info[b]) | a.info_step[b];
  if (b == 0 && lane == 0)
    for (int i = 0; i < 8; ++i) a.state_now[i] = a.state[i];

  // the plan shifted by one step, its last control held; the last step also hands the plan out
  for (int e = lane; e < T * nu; e += 64) {
    const int t = e / nu, m = e % nu;
    const int ts = t + 1 < T ? t + 1 : T - 1;
    const float v = a.u_best[((size_t)t * B + b) * nu + m];
    a.u_warm[((size_t)t * B + b) * nu + m] = a.u_best[((size_t)ts * B + b) * nu + m];
    if (a.u_plan != nullptr) a.u_plan[((size_t)t * B + b) * nu + m] = v;
  }
  if (a.x_plan != nullptr)
    for (int e = lane; e < T * nx; e += 64) {
      const size_t at = ((size_t)(e / nx) * B + b) * nx + e % nx;
      a.x_plan[at] = a.x_best[at];
    }
}

}  // namespace dmpc
