/*
 * dmpc_mlp_cost.h - a learned, stationary, non-quadratic stage cost (MlpCost of the Python layer), in the same libdmpc_hip.so as
 * include/dmpc.h.  The conventions of dmpc.h hold: device pointers to contiguous float32, the caller owns every buffer, inputs
 * are read-only, work is enqueued on `stream` and not synchronised, 0 ok / > 0 a hipError_t / < 0 DMPC_E_*.  Adding these symbols
 * does not move DMPC_VERSION.
 *
 *     c(tau) = 1/2 tau' Q tau + p' tau + w2' act(W1 tau + b1)
 *     tau = [x;u] (ns = nx + nu)   Q [ns,ns] (used as given, not symmetrised)   p [ns]   W1 [H,ns]   b1 [H]   w2 [H]
 *
 * `n_hidden` = H, `act` the code of dmpc.h's MlpDx section (0 tanh, 2 relu, 3 silu, 4 softplus).  Limits: nx <= 16, nu <= 8,
 * 1 <= H <= 256.  Checks common to every entry point, all before the first HIP call: a non-positive size or a NULL pointer that
 * is not named optional below: DMPC_E_BADARG; a size beyond the limits or another `act`: DMPC_E_UNSUPPORTED.  No entry point
 * allocates or synchronises with the host: each can be captured in a hipGraph.
 *
 * dmpc_mlp_cost_supported: 1 when the kernels serve (nx, nu, n_hidden, act), else 0.  Nothing is launched.
 *
 * dmpc_mlp_cost_approx: the second-order Taylor model at every (t, b) of x [T,B,nx], u [T,B,nu] (mpc/approximate.py:18-54), one
 *   launch.  With z = W1 tau + b1, Qs = (Q + Q')/2:
 *       H_out [T,B,ns,ns] = Qs + W1' diag(w2 * act''(z)) W1          (symmetric to the bit)
 *       g_out [T,B,ns]    = grad c(tau) - H tau = p + W1' (w2 * (act'(z) - act''(z) * (W1 tau)))
 *       costs_out [T,B]   = c(tau)
 *   H_out and g_out may both be NULL (values only), costs_out may be NULL; H_out without g_out, g_out without H_out, or all three
 *   NULL: DMPC_E_BADARG.  The costs of a values-only call are bit-equal to those of a full call.  T B ns^2 >= 2^31:
 *   DMPC_E_UNSUPPORTED.
 *
 * dmpc_mpc_forward_rec_mlp_cost: dmpc_mpc_forward_rec (dmpc.h) with this cost in place of C_true, c_true: the clamped closed-loop
 *   rollout under the dense LinDx F_true [T-1,B,nx,ns], f_true [T-1,B,nx] or NULL, and the per-trajectory backtracking search.
 *   The search's decision is taken on the cost difference formed per timestep - the quadratic part without cancellation, the
 *   network part as sum_h w2_h (act(z'_h) - act(z0_h)) - so a candidate equal to the nominal trajectory gives exactly 0.  The
 *   bound snap, the cap of 64 passes, the outputs and the info flags are dmpc_mpc_forward_rec's; old_costs, objs, u_first and
 *   info may be NULL.  T = 1 is served (no dynamics step: F_true and f_true are not read and may be NULL).
 *
 * dmpc_mlp_cost_param_grad: the gradient of a loss L(g_out, costs_out) with respect to the five parameters, with tau, H and H tau
 *   held constant (the Hessian is a constant of the graph, mpc/approximate.py:75).  grad_g [T,B,ns] = dL/dg_out, grad_costs [T,B]
 *   = dL/dcosts_out; either may be NULL, not both (DMPC_E_BADARG).  With v = grad_g, r = grad_costs at a point, q = W1 v,
 *   a = act(z), d1 = act'(z), d2 = act''(z), summed over t and b:
 *       dQ  = 1/2 (v tau' + tau v') + 1/2 r tau tau'        dp  = v + r tau
 *       dW1 = (w2*d1) v' + (w2*d2*q) tau' + r (w2*d1) tau'  db1 = w2*d2*q + r w2*d1        dw2 = d1*q + r a
 *   The outputs are WRITTEN (not added to).  Two launches.  mlp_cost_param_grad_kernel<act>: wavefront g of
 *   G = min(T B, 256) walks the points g, g + G, ... and stores one partial [dQ | dp | dW1 | db1 | dw2] into ws;
 *   mlp_cost_param_grad_reduce_kernel adds the G partials per element in ascending order.  No atomics: the result is bit-equal
 *   from call to call and depends on (T B, nx, nu, H) and the data alone.  ws NULL or shorter than
 *   dmpc_mlp_cost_param_grad_workspace_bytes (0 for a size the kernels refuse): DMPC_E_WORKSPACE.
 *
 * dmpc_box_ddp_mlp_cost: dmpc_box_ddp (dmpc.h) with this cost in place of a QuadCost's C, c, under a dense LinDx F [T-1,B,nx,ns],
 *   f [T-1,B,nx] or NULL: the whole iLQR loop as one chain of launches with its stop tests on the device.  No allocation, no host
 *   synchronisation, no read-back; `state`, `info` and the five outputs mean exactly what they mean in dmpc_box_ddp.
 *   cost_packed is ONE device array of contiguous float32, 16-byte aligned:
 *       [Q (ns*ns) | p (ns) | W1 (H*ns) | b1 (H) | w2 (H)]
 *   Every launch reads it and nothing is cached: an optimiser step in place is seen by the next call and by a replayed hipGraph.
 *   Launches of an iteration (after the stop they are no-ops through the device flag; the chain's first launch clears the
 *   chain's words):
 *     search_approximates = 0, five: lin_rollout_kernel; mlp_cost_approx_kernel<act> into the workspace's C_hat, c_hat; the
 *       backward sweep of dmpc_box_ddp's dyn_kind 0 on C_hat, c_hat, F (it re-centres c itself); mpc_forward_rec_mlp_cost_kernel<act>;
 *       the bookkeeping (box_ddp_select_kernel, and box_ddp_keep_kernel for the larger problems).
 *     search_approximates = 1: the first iteration as above; the search also stores the Taylor model of the trajectory it
 *       accepts - the next iteration's nominal one - through the function mlp_cost_approx_kernel forms it with, and the states
 *       it leaves are lin_rollout_kernel's to the bit (the same sums in the same order).  Every later iteration is three
 *       launches: sweep, search, bookkeeping; the nominal states alternate between two state buffers.  Every output and `state`
 *       is bit for bit that of search_approximates = 0.
 *   Then box_ddp_summary_kernel.  The workspace is dmpc_box_ddp's, then C_hat [T,B,ns,ns] and c_hat [T,B,ns]
 *   (dmpc_box_ddp_mlp_cost_workspace_bytes; 0 for a non-positive size).
 *   DMPC_E_BADARG: what dmpc_box_ddp reports so; cost_packed NULL or not 16-byte aligned; search_approximates other than 0 or 1;
 *   F NULL.  DMPC_E_UNSUPPORTED: dyn_kind != 0 - the codes 1 (the pendulum) and 2 (MlpDx) are reserved: with this cost either
 *   needs a search kernel that evaluates both models, which does not exist; batch_coupled != 0; a size or `act` that
 *   dmpc_mlp_cost_supported refuses; T B ns^2 >= 2^31.  DMPC_E_WORKSPACE: ws shorter than the query.  dyn_params is not read.
 */
#ifndef DMPC_MLP_COST_H_
#define DMPC_MLP_COST_H_

#include "dmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

int dmpc_mlp_cost_supported(int nx, int nu, int n_hidden, int act);
int dmpc_mlp_cost_approx(int T, int B, int nx, int nu, int n_hidden, int act, const float *Q, const float *p, const float *W1,
                         const float *b1, const float *w2, const float *x, const float *u, float *H_out, float *g_out,
                         float *costs_out, dmpc_stream_t stream);
int dmpc_mpc_forward_rec_mlp_cost(int T, int B, int nx, int nu, int n_hidden, int act, const float *Q, const float *p,
                                  const float *W1, const float *b1, const float *w2, const float *Ks, const float *ks,
                                  const float *controls, const float *states, const float *u_lower, const float *u_upper,
                                  const float *F_true, const float *f_true, float ls_decay, int max_ls_iter, float *x_out,
                                  float *u_out, float *costs, float *old_costs, float *alphas, float *objs, float *u_first,
                                  int32_t *n_ls_iter, int32_t *info, dmpc_stream_t stream);
size_t dmpc_mlp_cost_param_grad_workspace_bytes(int T, int B, int nx, int nu, int n_hidden);
int dmpc_mlp_cost_param_grad(int T, int B, int nx, int nu, int n_hidden, int act, const float *W1, const float *b1,
                             const float *w2, const float *x, const float *u, const float *grad_g, const float *grad_costs,
                             float *dQ, float *dp, float *dW1, float *db1, float *dw2, void *ws, size_t ws_bytes,
                             dmpc_stream_t stream);
size_t dmpc_box_ddp_mlp_cost_workspace_bytes(int T, int B, int nx, int nu);
int dmpc_box_ddp_mlp_cost(int T, int B, int nx, int nu, const float *x_init, const float *cost_packed, int n_hidden, int act,
                          int search_approximates, const float *F, const float *f, int dyn_kind, const float *dyn_params,
                          const float *u_init, const float *u_lower, const float *u_upper, float eps, int not_improved_lim,
                          float ls_decay, int max_ls_iter, float best_cost_eps, int max_iter, int n_qp_iter_max,
                          int scrambled_norm, int batch_coupled, float *x_best, float *u_best, float *costs_best,
                          float *du_norm_best, float *du_norm_last, int32_t *state, void *ws, size_t ws_bytes, int32_t *info,
                          dmpc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DMPC_MLP_COST_H_ */
