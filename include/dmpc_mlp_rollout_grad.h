/*
 * dmpc_mlp_rollout_grad.h - the vector-Jacobian product of the device rollout of a learned dynamics model (MlpDx.rollout of the
 * Python layer with param_grad="device"), in the same libdmpc_hip.so as include/dmpc.h.  The conventions of dmpc.h hold: device
 * pointers to contiguous float32, the caller owns every buffer, inputs are read-only, work is enqueued on `stream` and not
 * synchronised, 0 ok / > 0 a hipError_t / < 0 DMPC_E_*.  Adding these symbols does not move DMPC_VERSION.
 *
 * The model is the one of dmpc.h's MlpDx section: `n_hidden` a one-layer width H or DMPC_MLP_HIDDEN2(H1, H2), `act` that
 * section's code, the weights as the other entry points take them -
 *     one hidden layer:   W1 [H,ns], b1 [H], W2 [nx,H], b2 [nx]
 *     two hidden layers:  W1 [H1,ns], b1 [H1], W2 = [W2 (H2*H1) | W3 (nx*H2)], b2 = [b2 (H2) | b3 (nx)]
 * and the gradients go out in the same packed form.
 *
 * dmpc_mlp_rollout_grad: for x_0 = x_init, x_{t+1} = next(x_t, u_t) as dmpc_mlp_rollout_linearize rolls it, and any loss L of
 *   the rolled states with grad_x [T,B,nx] = dL/dx, the gradient of L with respect to every weight, x_init and u.  x [T,B,nx]
 *   are the states that launch stored, u [T,B,nu] its controls (row T-1 is not read).  Per trajectory, one hidden layer, with
 *   tau = [x_t;u_t], z = W1 tau + b1, a = act(z), d = act'(z):
 *       lam = grad_x[T-1]
 *       for t = T-2 .. 0:    r = lam
 *           dW2 += r a^T          db2 += r
 *           delta = d * (W2^T r)  dW1 += delta tau^T    db1 += delta
 *           d_u[t] = W1[:, nx:]^T delta
 *           lam    = grad_x[t] + W1[:, :nx]^T delta (+ r when residual)
 *       d_x_init = lam ;  d_u[T-1] = 0
 *   Two hidden layers: dW3 += r a2^T, db3 += r, e2 = d2 * (W3^T r), dW2 += e2 a1^T, db2 += e2, e1 = d1 * (W2^T e2),
 *   dW1 += e1 tau^T, db1 += e1, and d_u[t], lam are formed from e1.  The weight gradients are summed over t and b; every output
 *   is WRITTEN (not added to).  d_x_init [B,nx] and d_u [T,B,nu] may each be NULL.
 *   Two launches.  mlp_rollout_grad_kernel<act> or mlp2_rollout_grad_kernel<act>: one wavefront per trajectory, four per
 *   workgroup, the steps of a trajectory one dependent chain; G = dmpc_mlp_rollout_grad_partials(B, n_hidden) partials go into
 *   ws - min(B, 512) wavefronts' with one hidden layer, min(ceil(B / 4), 256) workgroups' with two, in the layouts of
 *   dmpc_mlp_param_grad and dmpc_mlp2_param_grad - and that entry point's reduction kernel adds them per element in ascending
 *   order.  No atomics: the result is bit-equal from call to call, d_x_init[b] and d_u[:, b] depend on trajectory b and the
 *   weights alone, and the weight gradients on (T, B, nx, nu, n_hidden) and the data alone.
 *   Checks, all before the first HIP call: a non-positive T, B, nx, nu or a NULL pointer (d_x_init, d_u, and ws when T = 1, may
 *   be NULL): DMPC_E_BADARG; a size or an `act` that dmpc_mlp_dx_supported refuses, T B nx ns >= 2^31: DMPC_E_UNSUPPORTED; ws NULL
 *   or shorter than dmpc_mlp_rollout_grad_workspace_bytes (0 for a size the kernels refuse) when T > 1: DMPC_E_WORKSPACE.
 *   T = 1: no sweep and no workspace; the weight gradients and d_u are zeros, d_x_init = grad_x[0].  No allocation, no host
 *   synchronisation; the call can be captured into a hipGraph.
 */
#ifndef DMPC_MLP_ROLLOUT_GRAD_H_
#define DMPC_MLP_ROLLOUT_GRAD_H_

#include "dmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

int dmpc_mlp_rollout_grad_partials(int B, int n_hidden);
size_t dmpc_mlp_rollout_grad_workspace_bytes(int B, int nx, int nu, int n_hidden);
int dmpc_mlp_rollout_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                          const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                          const float *grad_x, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                          void *ws, size_t ws_bytes, dmpc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DMPC_MLP_ROLLOUT_GRAD_H_ */
