/*
 * dmpc_episode.h - a closed-loop (receding-horizon) MPC episode as ONE chain of launches, in the same libdmpc_hip.so as
 * include/dmpc.h.  The conventions of dmpc.h hold: device pointers to contiguous float32, the caller owns every buffer, inputs
 * are read-only, work is enqueued on `stream` and not synchronised, 0 ok / > 0 a hipError_t / < 0 DMPC_E_*.  Adding these
 * symbols does not move DMPC_VERSION.
 *
 * dmpc_mpc_episode: n_steps times
 *     solve     dmpc_box_ddp from x_k, warm-started with u_warm (step 0: from x_init with u_init), as that entry point is
 *     advance   ONE launch (episode_advance_kernel, a wavefront per trajectory):
 *                   u_k = u_best[0]                       x_{k+1} = plant(x_k, u_k)
 *                   x_log[k+1] = x_{k+1}                  u_log[k] = u_k            (x_log[0] = x_init, by the first advance)
 *                   stage_cost[k] = 1/2 tau^T C[0] tau + c[0]^T tau,  tau = [x_k; u_k]         (the t = 0 term of the cost)
 *                   state_log[k]  = the solve's `state` words (dmpc_box_ddp)
 *                   info         |= the solve's info       (written by step 0, OR-ed into by the later ones)
 *                   u_warm[t]     = u_best[t+1] for t < T-1,  u_warm[T-1] = u_best[T-1]        (the last control is held)
 *               the last one also copies the last solve's best trajectory to x_plan, u_plan (each may be NULL).
 * C, c, u_lower, u_upper are the same arrays at every step: a time-invariant stage cost over a sliding horizon.
 *
 * The controller's model (F, f, dyn_kind, dyn_params) and the scalars are dmpc_box_ddp's, argument for argument; batch_coupled
 * is not offered.  The plant:
 *     plant_kind 0  linear, time-invariant: x+ = plant_F[b] [x;u] + plant_f[b]; plant_F [B,nx,ns], plant_f [B,nx] or NULL; the
 *                   summation order of dmpc_lin_rollout, so a step has the bits of that entry point at T = 2
 *     plant_kind 1  the simple pendulum, (nx, nu) = (3, 1): plant_params = HOST array {g, m, l, dt, max_torque, (ignored)} as
 *                   dmpc_box_ddp's dyn_kind 1; the bits of dmpc_pendulum_rollout_linearize at T = 2
 *     plant_kind 2  an MlpDx: plant_F = the packed weights as dyn_kind 2 takes them, plant_f = NULL, plant_params = HOST array
 *                   {n_hidden code, act, residual}; the bits of dmpc_mlp_rollout_linearize at T = 2
 * The model's packed weights and the plant's are read by every launch: nothing is cached.  nx + nu <= 64.
 *
 * Workspace (dmpc_mpc_episode_workspace_bytes; 0 for a non-positive size): dmpc_box_ddp's own, then x_cur [B,nx], u_warm
 * [T,B,nu] and the solve's outputs x_best, u_best, three [B] vectors, state [8], info [B] - each part 16-byte aligned, u_warm
 * and u_best apart.  `ws` must be 16-byte aligned.
 *
 * Checks, all before the first HIP call:
 *   DMPC_E_BADARG       n_steps < 1, T < 2, a non-positive B, nx, nu, max_iter or n_qp_iter_max; x_init, C, c, u_init, u_lower,
 *                       u_upper, x_log, u_log, stage_cost, state_log or ws NULL; plant_kind 0 or 2 with plant_F NULL; plant_kind
 *                       1 or 2 with plant_params NULL; plant_kind 2 with plant_f not NULL, with a non-integral or negative code
 *                       or a residual that is neither 0 nor 1; ws not 16-byte aligned; and what dmpc_box_ddp reports so
 *   DMPC_E_UNSUPPORTED  plant_kind outside 0..2; plant_kind 1 at another shape than (3, 1); a plant network that
 *                       dmpc_mlp_dx_supported refuses; nx + nu > 64; and what dmpc_box_ddp refuses for the model
 *   DMPC_E_WORKSPACE    ws_bytes below the query
 * No allocation, no host synchronisation, nothing is read back: the call can be captured into a hipGraph.
 */
#ifndef DMPC_EPISODE_H_
#define DMPC_EPISODE_H_

#include "dmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t dmpc_mpc_episode_workspace_bytes(int T, int B, int nx, int nu);
int dmpc_mpc_episode(int n_steps, int T, int B, int nx, int nu, const float *x_init, const float *C, const float *c,
                     const float *F, const float *f, int dyn_kind, const float *dyn_params, const float *plant_F,
                     const float *plant_f, int plant_kind, const float *plant_params, const float *u_init,
                     const float *u_lower, const float *u_upper, float eps, int not_improved_lim, float ls_decay,
                     int max_ls_iter, float best_cost_eps, int max_iter, int n_qp_iter_max, int scrambled_norm,
                     float *x_log, float *u_log, float *stage_cost, float *x_plan, float *u_plan, int32_t *state_log,
                     void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DMPC_EPISODE_H_ */
