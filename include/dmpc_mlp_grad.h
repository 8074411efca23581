/*
 * dmpc_mlp_grad.h - the weight gradient of a learned dynamics model with TWO hidden layers (MlpDx of the Python layer with
 * n_hidden = (H1, H2) and param_grad="device"), in the same libdmpc_hip.so as include/dmpc.h.  The conventions of dmpc.h hold:
 * device pointers to contiguous float32, the caller owns every buffer, inputs are read-only, work is enqueued on `stream` and
 * not synchronised, 0 ok / > 0 a hipError_t / < 0 DMPC_E_*.  Adding these symbols does not move DMPC_VERSION.
 *
 * The model is the one of dmpc.h's MlpDx section, `n_hidden` = DMPC_MLP_HIDDEN2(H1, H2), `act` that section's code, the weights
 * as the other two-layer entry points take them:
 *     W1 [H1,ns], b1 [H1], W2 = [W2 (H2*H1) | W3 (nx*H2)], b2 = [b2 (H2) | b3 (nx)]
 * and the gradients go out in the same packed form: dW1 [H1,ns], db1 [H1], dW2 = [dW2 | dW3], db2 = [db2 | db3].
 *
 * dmpc_mlp2_param_grad: the gradient of a loss L(f) of dmpc_mlp_rollout_linearize's f with respect to the six weights, F_t held
 *   constant at the value of the live Jacobian (mpc/approximate.py:77-119).  x [T,B,nx] are the states that launch stored,
 *   grad_f [T-1,B,nx] = dL/df (may be NULL when T = 1).  With tau = [x_t;u_t], r = grad_f_t,
 *       z1 = W1 tau + b1, a1 = act(z1), d1 = act'(z1);   z2 = W2 a1 + b2, a2 = act(z2), d2 = act'(z2)
 *       dW3 += r a2^T          db3 += r
 *       e2   = d2 * (W3^T r)   dW2 += e2 a1^T    db2 += e2
 *       e1   = d1 * (W2^T e2)  dW1 += e1 tau^T   db1 += e1
 *   summed over t and b; the outputs are WRITTEN (not added to).  d_x_init [B,nx] and d_u [T,B,nu], each or NULL, are written
 *   too: they are exact zeros, because the derivative of next through [x_t;u_t] and F_t's cancel at every step.
 *   Two launches.  mlp2_param_grad_kernel<act>: one wavefront per trajectory, four per workgroup; workgroup g of
 *   G = dmpc_mlp2_param_grad_partials(B) = min(ceil(B / 4), 256) walks the trajectory groups g, g + G, ... and stores one partial
 *   [dW1 | db1 | dW2 | dW3 | db2 | db3] into ws.  mlp2_param_grad_reduce_kernel adds the G partials per element in ascending
 *   order.  No atomics: the result is bit-equal from call to call and depends on (T, B, nx, nu, H1, H2) and the data alone.
 *   Checks, all before the first HIP call: a non-positive T, B, nx, nu or a NULL pointer (grad_f: only when T > 1; d_x_init, d_u,
 *   and ws when T = 1, may be NULL): DMPC_E_BADARG; a size or an `act` that dmpc_mlp_dx_supported refuses, a one-layer `n_hidden`
 *   (H2 = 0: that is dmpc_mlp_param_grad's), T B nx ns >= 2^31: DMPC_E_UNSUPPORTED; ws NULL or shorter than
 *   dmpc_mlp2_param_grad_workspace_bytes (0 for a size the kernels refuse and for a one-layer code) when T > 1: DMPC_E_WORKSPACE.
 *   T = 1 launches no sweep and writes zeros.  No allocation, no host synchronisation.
 */
#ifndef DMPC_MLP_GRAD_H_
#define DMPC_MLP_GRAD_H_

#include "dmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

int dmpc_mlp2_param_grad_partials(int B);
size_t dmpc_mlp2_param_grad_workspace_bytes(int B, int nx, int nu, int n_hidden);
int dmpc_mlp2_param_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                         const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                         const float *grad_f, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                         void *ws, size_t ws_bytes, dmpc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DMPC_MLP_GRAD_H_ */
