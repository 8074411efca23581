// Host-side sanitizer run of the C-ABI's argument checking and dispatch logic (SURVEY.md section 5's hook).
// Built by scripts/asan/run_asan_host.sh with -fsanitize=address,undefined on the HOST side of every *_api.hip and run on the
// CPU (no GPU needed, none used): workspace queries, dispatch tables, every entry point with NULL / inconsistent arguments
// (must return DMPC_E_BADARG or DMPC_E_WORKSPACE without touching memory), and the full host path of the solves with fake
// non-null device pointers for a sweep of shapes - the launch itself fails with "no device", the code before it has run.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "dmpc.h"
#include "dmpc_mlp_grad.h"
#include "dmpc_episode.h"
#include "dmpc_mlp_rollout_grad.h"
#include "dmpc_mlp_cost.h"

static int checks = 0, bad = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    ++checks;                                                          \
    if (!(cond)) { ++bad; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

int main() {
  float *p = reinterpret_cast<float *>(0x1000);       // a 16-byte aligned "device pointer" the host never dereferences
  double *pd = reinterpret_cast<double *>(0x1000);
  int32_t *pi = reinterpret_cast<int32_t *>(0x2000);
  uint8_t *pm = reinterpret_cast<uint8_t *>(0x3000);
  void *ws = reinterpret_cast<void *>(0x4000);
  EXPECT(dmpc_version() == DMPC_VERSION);
  EXPECT(dmpc_mpc_step_status(0, pi, pi, p, pi, nullptr) == DMPC_E_BADARG);      // (argument checks return before any launch)
  EXPECT(dmpc_mpc_step_status(16, pi, pi, p, nullptr, nullptr) == DMPC_E_BADARG);
  const int shapes[][2] = {{1, 1}, {3, 1}, {8, 2}, {4, 4}, {8, 4}, {12, 3}, {6, 3}, {5, 5}, {3, 8}, {16, 4}, {20, 6}, {32, 8}, {16, 8},
                           {40, 4}, {10, 12}, {64, 16}, {100, 1}, {70, 3}, {300, 40}};
  for (auto &s : shapes) {
    const int nx = s[0], nu = s[1];
    for (int T : {1, 2, 20, 50, 51, 52, 75, 100, 400})
      for (int B : {1, 3, 4, 17, 4096}) {
        const int fam = dmpc_lqr_kernel_family(nx, nu);
        EXPECT(fam >= 1 && fam <= 5);
        const size_t wsb = dmpc_lqr_workspace_bytes(T, B, nx, nu);
        EXPECT(wsb >= (size_t)T * B * nu * (nx + 1) * 4);
        (void)dmpc_lqr_solve_path(T, B, nx, nu);
        (void)dmpc_lqr_saving_available(T, B, nx, nu);
        EXPECT(dmpc_lqr_kkt_workspace_bytes(T, B, nx, nu) >= wsb);
        EXPECT(dmpc_mpc_step_workspace_bytes(T, B, nx, nu) >= wsb);
        EXPECT(dmpc_lqr_f64_workspace_bytes(T, B, nx, nu) > 0);
        (void)dmpc_box_ddp_workspace_bytes(T, B, nx, nu);
        (void)dmpc_mpc_backward_rec_workspace_bytes(T, B, nx, nu, 20, 0);
        (void)dmpc_mpc_backward_rec_workspace_bytes(T, B, nx, nu, 20, 1);
        // the whole host path: dispatch, layout arithmetic, launch attempt (fails: no device) - must not crash or overrun
        (void)dmpc_lqr_solve(T, B, nx, nu, p, p, T > 1 ? p : nullptr, p, p, nullptr, nullptr, nullptr, p, p, ws, wsb, pi, nullptr);
        (void)dmpc_lqr_solve(T, B, nx, nu, p, p, T > 1 ? p : nullptr, nullptr, p, pm, p, p, p, p, ws, wsb, pi, nullptr);
        (void)dmpc_lqr_backward_sweep_ws(T, B, nx, nu, p, p, p, p, nullptr, p, p, ws, wsb, pi, nullptr);
        (void)dmpc_lqr_forward_sweep(T, B, nx, nu, p, p, p, p, p, nullptr, p, p, pi, nullptr);
        if (T > 1) {
          (void)dmpc_lqr_kkt_grad(T, B, nx, nu, p, p, p, p, p, p, p, 0, p, p, p, p, p, ws, dmpc_lqr_kkt_workspace_bytes(T, B, nx, nu), pi, nullptr);
          (void)dmpc_mpc_step_forward(T, B, nx, nu, p, p, p, p, p, p, p, p, p, p, p, p, 1, 0.2f, 5, 20, 0, p, p, p, p, p, p, p, p, p, pi, pi,
                                      ws, dmpc_mpc_step_workspace_bytes(T, B, nx, nu), pi, nullptr);
          (void)dmpc_lqr_solve_f64(T, B, nx, nu, pd, pd, pd, pd, pd, nullptr, nullptr, nullptr, pd, pd, ws,
                                   dmpc_lqr_f64_workspace_bytes(T, B, nx, nu), pi, nullptr);
          // the MPC step family's routes and launchers (csrc/mpc_api.hip): the halves of the step on their own, the box QP, the
          // device-driven BoxDDP loop; `controls` aligned and four bytes off, per-trajectory and batch-coupled
          float *p4 = reinterpret_cast<float *>(0x1004);
          (void)dmpc_mpc_step_forward(T, B, nx, nu, p, p, p, p, p4, p, p, p, p, p, p, p, 0, 0.2f, 5, 20, 1, p, p, p, p, p, p, p, p, p, pi, pi,
                                      ws, dmpc_mpc_step_workspace_bytes(T, B, nx, nu), pi, nullptr);
          for (int coupled : {0, 1}) {
            const size_t bwb = dmpc_mpc_backward_rec_workspace_bytes(T, B, nx, nu, 20, coupled);
            for (float *u : {p, p4}) {
              (void)dmpc_mpc_backward_rec(T, B, nx, nu, p, p, p, p, u, p, p, 20, coupled, p, p, pi, ws, bwb, pi, nullptr);
              (void)dmpc_mpc_backward_rec(T, B, nx, nu, p, p, p, nullptr, u, p, p, 20, coupled, p, p, pi, ws, bwb, pi, nullptr);
            }
            if (bwb > 0)
              EXPECT(dmpc_mpc_backward_rec(T, B, nx, nu, p, p, p, p, p, p, p, 20, coupled, p, p, pi, ws, bwb - 1, pi, nullptr) == DMPC_E_WORKSPACE);
            (void)dmpc_pnqp(B, nu, p, p, p, p, nullptr, 20, coupled, p, p, pi, p, pi, ws, dmpc_pnqp_workspace_bytes(B, nu, 20, coupled), pi,
                            nullptr);
            const float pendulum[6] = {10.f, 1.f, 1.f, 0.05f, 2.f, 0.f};
            const size_t dwb = dmpc_box_ddp_workspace_bytes(T, B, nx, nu);
            for (float *u : {p, p4}) {
              (void)dmpc_box_ddp(T, B, nx, nu, p, p, p, p, p, 0, nullptr, u, p, p, 1e-3f, 5, 0.2f, 10, 1e-3f, 3, 20, 0, coupled, p, p, p, p, p,
                                 pi, ws, dwb, pi, nullptr);
              const int rd = dmpc_box_ddp(T, B, nx, nu, p, p, p, nullptr, nullptr, 1, pendulum, u, p, p, 1e-3f, 5, 0.2f, 10, 1e-3f, 3, 20, 0,
                                          coupled, p, p, p, p, p, pi, ws, dwb, pi, nullptr);
              if (nx != 3 || nu != 1) EXPECT(rd == DMPC_E_BADARG);
              // the MlpDx network inside the chain (dyn_kind 2): F = the packed weights, host floats {n_hidden, act, residual, search_linearizes}
              for (float lin : {0.f, 1.f}) {
                const float mlp[4] = {64.f, 2.f, 1.f, lin};
                const int rm = dmpc_box_ddp(T, B, nx, nu, p, p, p, p, nullptr, 2, mlp, u, p, p, 1e-3f, 5, 0.2f, 10, 1e-3f, 3, 20, 0, coupled,
                                            p, p, p, p, p, pi, ws, dwb, pi, nullptr);
                if (coupled || nx > 16 || nu > 8) EXPECT(rm == DMPC_E_UNSUPPORTED);
                EXPECT(dmpc_box_ddp(T, B, nx, nu, p, p, p, p, p, 2, mlp, u, p, p, 1e-3f, 5, 0.2f, 10, 1e-3f, 3, 20, 0, coupled, p, p, p, p, p,
                                    pi, ws, dwb, pi, nullptr) == DMPC_E_BADARG);      // (f given)
              }
            }
          }
          for (float *u : {p, p4})
            (void)dmpc_mpc_forward_rec(T, B, nx, nu, p, p, u, p, p, p, p, p, p, p, 0.2f, 5, p, p, p, p, p, p, p, pi, pi, nullptr);
          if (nx == 3 && nu == 1)
            for (float *u : {p, p4})
              (void)dmpc_mpc_forward_rec_pendulum(T, B, p, p, u, p, p, p, p, p, 10.f, 1.f, 1.f, 0.05f, 2.f, 0.2f, 5, p, p, p, p, p, p, p, pi,
                                                  pi, nullptr);
        }
        // inconsistent arguments are refused before anything else happens
        EXPECT(dmpc_lqr_solve(T, B, nx, nu, nullptr, p, p, p, p, nullptr, nullptr, nullptr, p, p, ws, wsb, pi, nullptr) == DMPC_E_BADARG);
        EXPECT(dmpc_lqr_solve(T, B, nx, nu, p, p, p, p, p, nullptr, p, nullptr, p, p, ws, wsb, pi, nullptr) == DMPC_E_BADARG);
        EXPECT(dmpc_lqr_solve(T, B, nx, nu, p + 1, p, p, p, p, nullptr, nullptr, nullptr, p, p, ws, wsb, pi, nullptr) == DMPC_E_BADARG);
        if (wsb > 0) EXPECT(dmpc_lqr_solve(T, B, nx, nu, p, p, p, p, p, nullptr, nullptr, nullptr, p, p, ws, wsb - 1, pi, nullptr) == DMPC_E_WORKSPACE);
      }
  }
  // batch-shared C and F: workspace queries, every layout, argument and workspace checks, the host path of both launches
  for (int nx : {1, 3, 8, 17, 32, 33})
    for (int nu : {1, 2, 5, 8, 9})
      for (int T : {1, 2, 50})
        for (int B : {1, 65, 4096}) {
          const size_t wsb = dmpc_lqr_shared_workspace_bytes(T, B, nx, nu);
          const size_t gwb = dmpc_lqr_shared_grad_workspace_bytes(T, B, nx, nu);
          const bool ok = nx <= 32 && nu <= 8;
          EXPECT(ok == (wsb > 0) && ok == (gwb > 0));
          {   // the MPC step's parameter-shaped gradient over the same reduction: workspace query, layouts, argument checks, host path
            const size_t mwb = dmpc_mpc_step_shared_grad_workspace_bytes(T, B, nx, nu);
            EXPECT((ok && T > 1) == (mwb > 0));
            for (uint32_t layout = 0; layout < 64; ++layout) {
              const int rm = dmpc_mpc_step_backward_shared(T, B, nx, nu, layout, p, p, p, p, p, p, p, p, p, p, layout & 1 ? p : nullptr,
                                                           layout & 4 ? p : nullptr, p, layout & 16 ? p : nullptr, p, pi, 1e-5f, ws,
                                                           mwb, pi, nullptr);
              if (T <= 1 || (layout & (DMPC_SHARED_CVEC_BATCH | DMPC_SHARED_FVEC_BATCH))) EXPECT(rm == DMPC_E_BADARG);
              else if (!ok) EXPECT(rm == DMPC_E_UNSUPPORTED);
            }
            if (mwb > 0) {
              EXPECT(mwb >= (size_t)T * B * (4 * nx + 2 * nu) * 4 + dmpc_lqr_workspace_bytes(T, B, nx, nu));
              EXPECT(dmpc_mpc_step_backward_shared(T, B, nx, nu, 0, p, p, nullptr, p, p, p, p, p, p, p, nullptr, nullptr, p, nullptr,
                                                   nullptr, nullptr, 0.f, ws, mwb, pi, nullptr) == DMPC_E_BADARG);
              EXPECT(dmpc_mpc_step_backward_shared(T, B, nx, nu, 0, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, p, nullptr,
                                                   nullptr, nullptr, 0.f, ws, mwb - 1, pi, nullptr) == DMPC_E_WORKSPACE);
            }
          }
          if (!ok) {
            EXPECT(dmpc_lqr_shared_solve(T, B, nx, nu, 0, p, p, p, nullptr, p, p, p, ws, 1 << 30, pi, nullptr) == DMPC_E_UNSUPPORTED);
            continue;
          }
          EXPECT(wsb > dmpc_lqr_shared_saved_bytes(T, nx, nu) && wsb >= (size_t)T * B * nu * 4);
          EXPECT(gwb >= (size_t)T * B * (3 * nx + nu) * 4);
          for (uint32_t layout = 0; layout < 64; ++layout) {
            const bool good = !((layout & DMPC_SHARED_CVEC_BATCH) && !(layout & DMPC_SHARED_CVEC_TIME)) &&
                              !((layout & DMPC_SHARED_FVEC_BATCH) && !(layout & DMPC_SHARED_FVEC_TIME));
            const int rs = dmpc_lqr_shared_solve(T, B, nx, nu, layout, p, p, p, p, p, p, p, ws, wsb, pi, nullptr);
            const int rg = dmpc_lqr_shared_kkt_grad(T, B, nx, nu, layout, p, p, p, p, p, ws, p, p, layout & 1, p, p, p, p, p, ws,
                                                    gwb, pi, nullptr);
            if (!good) EXPECT(rs == DMPC_E_BADARG && rg == DMPC_E_BADARG);
          }
          EXPECT(dmpc_lqr_shared_solve(T, B, nx, nu, 64, p, p, p, p, p, p, p, ws, wsb, pi, nullptr) == DMPC_E_BADARG);
          EXPECT(dmpc_lqr_shared_solve(T, B, nx, nu, 0, nullptr, p, p, p, p, p, p, ws, wsb, pi, nullptr) == DMPC_E_BADARG);
          EXPECT(dmpc_lqr_shared_solve(T, B, nx, nu, 0, p + 1, p, p, p, p, p, p, ws, wsb, pi, nullptr) == DMPC_E_BADARG);
          EXPECT(dmpc_lqr_shared_solve(T, B, nx, nu, 0, p, p, p, p, p, p, p, ws, wsb - 1, pi, nullptr) == DMPC_E_WORKSPACE);
          EXPECT(dmpc_lqr_shared_kkt_grad(T, B, nx, nu, 0, p, p, p, p, p, ws, p, p, 0, p, p, nullptr, p, p, ws, gwb, pi, nullptr) ==
                 DMPC_E_BADARG);
          EXPECT(dmpc_lqr_shared_kkt_grad(T, B, nx, nu, 0, p, p, p, p, p, ws, p, p, 0, p, p, p, p, p, ws, gwb - 1, pi, nullptr) ==
                 DMPC_E_WORKSPACE);
        }
  {   // MPCstep.backward's tiled-cost sums come from the LDS-DMA co-state kernel alone, which moves x and u in 16-byte chunks:
      // a view of x four bytes off is refused before anything is launched; the aligned call goes on to its launches (no device)
    float *x4 = reinterpret_cast<float *>(0x1004);
    const size_t mwb = dmpc_mpc_step_workspace_bytes(20, 4, 8, 2);
    EXPECT(dmpc_mpc_step_backward(20, 4, 8, 2, p, p, p, x4, p, p, p, p, p, p, nullptr, nullptr, nullptr, nullptr, p, p, nullptr,
                                  nullptr, 0.f, ws, mwb, pi, nullptr) == DMPC_E_UNSUPPORTED);
    EXPECT(dmpc_mpc_step_backward(20, 4, 8, 2, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, nullptr, p, p, nullptr,
                                  nullptr, 0.f, ws, mwb, pi, nullptr) != DMPC_E_UNSUPPORTED);
  }
  // the learned dynamics model: size and argument checks come before any HIP call; the supported sizes go on to the launch
  for (int nx : {0, 1, 3, 16, 17})
    for (int nu : {0, 1, 8, 9})
      for (int H : {0, 1, 5, 64, 256, 257})
        for (int act : {0, 1, 2, 4, 5})
          for (int T : {0, 1, 2, 20}) {
            const bool act_ok = act == 0 || act == 2 || act == 3 || act == 4;
            const bool sized = nx > 0 && nu > 0, ok = sized && act_ok && nx <= 16 && nu <= 8 && H >= 1 && H <= 256;
            EXPECT(dmpc_mlp_dx_supported(nx, nu, H, act) == (ok ? 1 : 0));
            const int rr = dmpc_mlp_rollout_linearize(T, 5, nx, nu, H, act, 1, p, p, p, p, p, p, p, p, p, nullptr);
            const int rs = dmpc_mpc_forward_rec_mlp(T, 5, nx, nu, H, act, 1, p, p, p, p, p, p, p, p, p, p, p, p, 0.2f, 10, p, p, p, p,
                                                    p, p, p, pi, pi, nullptr);
            if (!sized || T <= 0) EXPECT(rr == DMPC_E_BADARG && rs == DMPC_E_BADARG);
            else if (!ok) EXPECT(rr == DMPC_E_UNSUPPORTED && (T == 1 ? rs == DMPC_E_BADARG : rs == DMPC_E_UNSUPPORTED));
            else EXPECT(rr >= 0 && (T == 1 ? rs == DMPC_E_BADARG : rs >= 0));
            if (ok && T > 1) {
              EXPECT(dmpc_mlp_rollout_linearize(T, 5, nx, nu, H, 0, 1, nullptr, p, p, p, p, p, p, p, p, nullptr) == DMPC_E_BADARG);
              EXPECT(dmpc_mlp_rollout_linearize(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, p, nullptr, p, nullptr) == DMPC_E_BADARG);
              EXPECT(dmpc_mpc_forward_rec_mlp(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, p, nullptr, p, p, p, p, 0.2f, 10, p, p, p, p,
                                              p, p, p, pi, pi, nullptr) == DMPC_E_BADARG);
            }
            // its weight gradient: the same order of checks, then the workspace
            const size_t gwb = dmpc_mlp_param_grad_workspace_bytes(5, nx, nu, H);
            EXPECT((gwb > 0) == (sized && nx <= 16 && nu <= 8 && H >= 1 && H <= 256));
            EXPECT(gwb == (size_t)dmpc_mlp_param_grad_partials(5) * (size_t)(gwb ? H * (nx + nu) + H + nx * H + nx : 0) * sizeof(float));
            const int rg = dmpc_mlp_param_grad(T, 5, nx, nu, H, act, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, gwb, nullptr);
            if (!sized || T <= 0) EXPECT(rg == DMPC_E_BADARG);
            else if (!ok) EXPECT(rg == DMPC_E_UNSUPPORTED);
            else EXPECT(rg >= 0);
            if (ok && T > 1) {
              EXPECT(dmpc_mlp_param_grad(T, 5, nx, nu, H, 0, 1, nullptr, p, p, p, p, p, p, p, p, p, p, p, p, ws, gwb, nullptr) ==
                     DMPC_E_BADARG);
              EXPECT(dmpc_mlp_param_grad(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, p, p, p, nullptr, p, p, p, ws, gwb, nullptr) ==
                     DMPC_E_BADARG);
              EXPECT(dmpc_mlp_param_grad(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, ws, gwb - 1,
                                         nullptr) == DMPC_E_WORKSPACE);
              EXPECT(dmpc_mlp_param_grad(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, gwb, nullptr) ==
                     DMPC_E_WORKSPACE);
            }
            // the rollout's vector-Jacobian product (include/dmpc_mlp_rollout_grad.h): the same checks, the same workspace
            EXPECT(dmpc_mlp_rollout_grad_workspace_bytes(5, nx, nu, H) == gwb);
            EXPECT(dmpc_mlp_rollout_grad_partials(5, H) == (H >= 1 ? dmpc_mlp_param_grad_partials(5) : 0));
            const int rv = dmpc_mlp_rollout_grad(T, 5, nx, nu, H, act, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, gwb, nullptr);
            if (!sized || T <= 0) EXPECT(rv == DMPC_E_BADARG);
            else if (!ok) EXPECT(rv == DMPC_E_UNSUPPORTED);
            else EXPECT(rv >= 0);
            if (ok && T > 0)      // grad_x is read at every T: d_x_init = grad_x[0] when T = 1
              EXPECT(dmpc_mlp_rollout_grad(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, nullptr, p, p, p, p, p, p, ws, gwb, nullptr) ==
                     DMPC_E_BADARG);
            if (ok && T > 1) {
              EXPECT(dmpc_mlp_rollout_grad(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, ws, gwb - 1,
                                           nullptr) == DMPC_E_WORKSPACE);
              EXPECT(dmpc_mlp_rollout_grad(T, 5, nx, nu, H, 0, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, gwb, nullptr) ==
                     DMPC_E_WORKSPACE);
            }
          }
  // two hidden layers: n_hidden = DMPC_MLP_HIDDEN2(H1, H2); the rollout and the search take it, the weight gradient refuses it
  for (int H1 : {0, 1, 5, 128, 129})
    for (int H2 : {1, 7, 128, 129})
      for (int T : {1, 2, 20}) {
        const int H = DMPC_MLP_HIDDEN2(H1, H2);
        const bool ok = H1 >= 1 && H1 <= 128 && H2 <= 128;
        EXPECT(dmpc_mlp_dx_supported(16, 8, H, 3) == (ok ? 1 : 0));
        const int rr = dmpc_mlp_rollout_linearize(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, nullptr);
        const int rs = dmpc_mpc_forward_rec_mlp(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, p, 0.2f, 10, p, p, p, p, p, p,
                                                p, pi, pi, nullptr);
        if (!ok) EXPECT(rr == DMPC_E_UNSUPPORTED && (T == 1 ? rs == DMPC_E_BADARG : rs == DMPC_E_UNSUPPORTED));
        else EXPECT(rr >= 0 && (T == 1 ? rs == DMPC_E_BADARG : rs >= 0));
        EXPECT(dmpc_mlp_rollout_linearize(T, 5, 16, 8, H, 3, 1, p, p, nullptr, p, p, p, p, p, p, nullptr) == DMPC_E_BADARG);
        EXPECT(dmpc_mlp_param_grad_workspace_bytes(5, 16, 8, H) == 0);
        EXPECT(dmpc_mlp_param_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, 1 << 20, nullptr) ==
               DMPC_E_UNSUPPORTED);
        // ... and dmpc_mlp2_param_grad (include/dmpc_mlp_grad.h) takes it, and refuses the one-layer code in turn
        const size_t g2 = dmpc_mlp2_param_grad_workspace_bytes(5, 16, 8, H);
        EXPECT(g2 == (ok ? (size_t)dmpc_mlp2_param_grad_partials(5) * (size_t)(H1 * 24 + H1 + H2 * H1 + 16 * H2 + H2 + 16) * sizeof(float) : 0));
        const int rg2 = dmpc_mlp2_param_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, g2, nullptr);
        EXPECT(ok ? rg2 >= 0 : rg2 == DMPC_E_UNSUPPORTED);
        if (ok) {
          EXPECT(dmpc_mlp2_param_grad(T, 5, 16, 8, H, 3, 1, p, p, nullptr, p, p, p, p, p, p, p, p, p, p, ws, g2, nullptr) == DMPC_E_BADARG);
          EXPECT(dmpc_mlp2_param_grad(T, 5, 16, 8, H1, 3, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, g2, nullptr) == DMPC_E_UNSUPPORTED);
          if (T > 1) {
            EXPECT(dmpc_mlp2_param_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, nullptr, p, p, p, p, p, p, ws, g2, nullptr) == DMPC_E_BADARG);
            EXPECT(dmpc_mlp2_param_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, ws, g2 - 1, nullptr) ==
                   DMPC_E_WORKSPACE);
            EXPECT(dmpc_mlp2_param_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, g2, nullptr) == DMPC_E_WORKSPACE);
          }
        }
        // ... and dmpc_mlp_rollout_grad takes both codes
        EXPECT(dmpc_mlp_rollout_grad_workspace_bytes(5, 16, 8, H) == g2);
        const int rv2 = dmpc_mlp_rollout_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, g2, nullptr);
        EXPECT(ok ? rv2 >= 0 : rv2 == DMPC_E_UNSUPPORTED);
        if (ok && T > 1) {
          EXPECT(dmpc_mlp_rollout_grad_partials(5, H) == dmpc_mlp2_param_grad_partials(5));
          EXPECT(dmpc_mlp_rollout_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, ws, g2 - 1, nullptr) ==
                 DMPC_E_WORKSPACE);
          EXPECT(dmpc_mlp_rollout_grad(T, 5, 16, 8, H, 3, 1, p, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, g2, nullptr) == DMPC_E_WORKSPACE);
        }
        const float mlp2[4] = {(float)H, 3.f, 1.f, 0.f};
        if (T > 1) {
          const int rm = dmpc_box_ddp(T, 4, 16, 8, p, p, p, p, nullptr, 2, mlp2, p, p, p, 1e-3f, 5, 0.2f, 10, 1e-3f, 3, 20, 0, 0, p, p, p,
                                      p, p, pi, ws, dmpc_box_ddp_workspace_bytes(T, 4, 16, 8), nullptr, nullptr);
          EXPECT(ok ? rm >= 0 : rm == DMPC_E_UNSUPPORTED);
        }
      }
  // the closed-loop episode (include/dmpc_episode.h): its own checks first, then dmpc_box_ddp's; the workspace arithmetic
  {
    const float pend[6] = {10.f, 1.f, 1.f, 0.05f, 2.f, 1.f};
    auto episode = [&](int n_steps, int T, int B, int nx, int nu, const float *F, int dyn_kind, const float *dyn_params, const float *plant_F,
                       const float *plant_f, int plant_kind, const float *plant_params, void *w, size_t short_by) {
      return dmpc_mpc_episode(n_steps, T, B, nx, nu, p, p, p, F, nullptr, dyn_kind, dyn_params, plant_F, plant_f, plant_kind, plant_params,
                              p, p, p, 1e-3f, 5, 0.2f, 10, 1e-4f, 3, 20, 1, p, p, p, nullptr, nullptr, pi, w,
                              dmpc_mpc_episode_workspace_bytes(T, B, nx, nu) - short_by, nullptr, nullptr);
    };
    EXPECT(dmpc_mpc_episode_workspace_bytes(0, 4, 3, 1) == 0 && dmpc_mpc_episode_workspace_bytes(4, 4, 3, 0) == 0);
    for (auto &s : shapes)
      for (int T : {2, 20, 400})
        for (int B : {1, 3, 4, 17, 4096}) {
          const int nx = s[0], nu = s[1];
          const size_t eb = dmpc_mpc_episode_workspace_bytes(T, B, nx, nu);
          EXPECT(eb >= dmpc_box_ddp_workspace_bytes(T, B, nx, nu) + sizeof(float) * ((size_t)B * nx + (size_t)T * B * (nx + 2 * nu) + 4 * (size_t)B + 8));
          EXPECT(eb % 16 == 0);
          const int r = episode(2, T, B, nx, nu, p, 0, nullptr, p, p, 0, nullptr, ws, 0);
          EXPECT(nx + nu > 64 ? r == DMPC_E_UNSUPPORTED : (r >= 0 || r == DMPC_E_UNSUPPORTED));   // (launches fail: no device)
          EXPECT(episode(2, T, B, nx, nu, p, 0, nullptr, p, p, 0, nullptr, ws, 1) == (nx + nu > 64 ? DMPC_E_UNSUPPORTED : DMPC_E_WORKSPACE));
          const int rp = episode(2, T, B, nx, nu, p, 0, nullptr, nullptr, nullptr, 1, pend, ws, 0);
          EXPECT(nx == 3 && nu == 1 ? rp >= 0 : rp == DMPC_E_UNSUPPORTED);
        }
    EXPECT(episode(0, 4, 2, 3, 1, p, 0, nullptr, p, nullptr, 0, nullptr, ws, 0) == DMPC_E_BADARG);
    EXPECT(episode(2, 1, 2, 3, 1, p, 0, nullptr, p, nullptr, 0, nullptr, ws, 0) == DMPC_E_BADARG);
    EXPECT(episode(2, 4, 0, 3, 1, p, 0, nullptr, p, nullptr, 0, nullptr, ws, 0) == DMPC_E_BADARG);
    EXPECT(episode(2, 4, 2, 3, 1, p, 0, nullptr, nullptr, nullptr, 0, nullptr, ws, 0) == DMPC_E_BADARG);
    EXPECT(episode(2, 4, 2, 3, 1, p, 0, nullptr, p, nullptr, 0, nullptr, nullptr, 0) == DMPC_E_BADARG);
    EXPECT(episode(2, 4, 2, 3, 1, p, 0, nullptr, p, nullptr, 3, nullptr, ws, 0) == DMPC_E_UNSUPPORTED);
    EXPECT(episode(2, 4, 2, 3, 1, p, 0, nullptr, nullptr, nullptr, 1, nullptr, ws, 0) == DMPC_E_BADARG);
    EXPECT(episode(2, 4, 2, 3, 1, nullptr, 0, nullptr, p, nullptr, 0, nullptr, ws, 0) == DMPC_E_BADARG);        // (dmpc_box_ddp's)
    EXPECT(episode(2, 4, 2, 3, 1, p, 3, nullptr, p, nullptr, 0, nullptr, ws, 0) == DMPC_E_UNSUPPORTED);         // (dmpc_box_ddp's)
    EXPECT(episode(2, 4, 2, 3, 1, nullptr, 1, pend, nullptr, nullptr, 1, pend, ws, 0) >= 0);
    for (int H1 : {0, 1, 5, 128, 129, 256, 257})
      for (int H2 : {0, 7, 128, 129}) {
        const float net[4] = {(float)DMPC_MLP_HIDDEN2(H1, H2), 3.f, 1.f, 0.f};
        const bool ok = dmpc_mlp_dx_supported(16, 8, DMPC_MLP_HIDDEN2(H1, H2), 3) == 1;
        const int rn = episode(2, 5, 3, 16, 8, p, 2, net, p, nullptr, 2, net, ws, 0);      // the network as model and as plant
        EXPECT(ok ? rn >= 0 : rn == DMPC_E_UNSUPPORTED);
        EXPECT(episode(2, 5, 3, 16, 8, p, 0, nullptr, p, p, 2, net, ws, 0) == DMPC_E_BADARG);                   // plant_f with a network
        if (ok) EXPECT(episode(2, 5, 3, 16, 8, p, 2, net, p, nullptr, 2, net, ws, 1) == DMPC_E_WORKSPACE);
      }
    const float frac[3] = {5.5f, 0.f, 1.f}, neg[3] = {5.f, -1.f, 1.f}, res[3] = {5.f, 0.f, 0.5f};
    for (const float *bad_params : {frac, neg, res})
      EXPECT(episode(2, 4, 2, 3, 1, p, 0, nullptr, p, nullptr, 2, bad_params, ws, 0) == DMPC_E_BADARG);
  }
  // the learned stage cost (include/dmpc_mlp_cost.h): the limits, every argument check, the workspace arithmetic, the host path
  for (auto &s : shapes)
    for (int H : {0, 1, 7, 64, 65, 256, 257})
      for (int act : {0, 1, 2, 3, 4, 5}) {
        const int nx = s[0], nu = s[1], ns = nx + nu;
        const bool ok = nx <= 16 && nu <= 8 && H >= 1 && H <= 256 && act != 1 && act != 5;
        const int refused = H < 1 ? DMPC_E_BADARG : DMPC_E_UNSUPPORTED;
        EXPECT(dmpc_mlp_cost_supported(nx, nu, H, act) == (ok ? 1 : 0));
        for (int T : {1, 2, 20})
          for (int B : {1, 5, 4096}) {
            const size_t gb = dmpc_mlp_cost_param_grad_workspace_bytes(T, B, nx, nu, H);
            const long long pts = (long long)T * B;
            if (nx <= 16 && nu <= 8 && H >= 1 && H <= 256)
              EXPECT(gb == (size_t)(pts < 256 ? pts : 256) * (ns * ns + ns + H * ns + 2 * H) * sizeof(float));
            else
              EXPECT(gb == 0);
            const int ra = dmpc_mlp_cost_approx(T, B, nx, nu, H, act, p, p, p, p, p, p, p, p, p, p, nullptr);
            const int rv = dmpc_mlp_cost_approx(T, B, nx, nu, H, act, p, p, p, p, p, p, p, nullptr, nullptr, p, nullptr);
            const int rs = dmpc_mpc_forward_rec_mlp_cost(T, B, nx, nu, H, act, p, p, p, p, p, p, p, p, p, p, p, T > 1 ? p : nullptr, nullptr,
                                                         0.2f, 10, p, p, p, nullptr, p, nullptr, nullptr, pi, nullptr, nullptr);
            const int rg = dmpc_mlp_cost_param_grad(T, B, nx, nu, H, act, p, p, p, p, p, p, nullptr, p, p, p, p, p, ws, gb, nullptr);
            for (int r : {ra, rv, rs, rg}) EXPECT(ok ? r >= 0 : r == refused);      // (launches fail: no device)
            if (ok) {
              EXPECT(dmpc_mlp_cost_param_grad(T, B, nx, nu, H, act, p, p, p, p, p, p, p, p, p, p, p, p, ws, gb - 1, nullptr) == DMPC_E_WORKSPACE);
              EXPECT(dmpc_mlp_cost_param_grad(T, B, nx, nu, H, act, p, p, p, p, p, p, p, p, p, p, p, p, nullptr, gb, nullptr) == DMPC_E_WORKSPACE);
              EXPECT(dmpc_mlp_cost_param_grad(T, B, nx, nu, H, act, p, p, p, p, p, nullptr, nullptr, p, p, p, p, p, ws, gb, nullptr) == DMPC_E_BADARG);
              EXPECT(dmpc_mlp_cost_approx(T, B, nx, nu, H, act, p, p, p, p, p, p, p, p, nullptr, p, nullptr) == DMPC_E_BADARG);
              EXPECT(dmpc_mlp_cost_approx(T, B, nx, nu, H, act, p, p, p, p, p, p, p, nullptr, nullptr, nullptr, nullptr) == DMPC_E_BADARG);
              if (T > 1)
                EXPECT(dmpc_mpc_forward_rec_mlp_cost(T, B, nx, nu, H, act, p, p, p, p, p, p, p, p, p, p, p, nullptr, nullptr, 0.2f, 10, p, p, p,
                                                     nullptr, p, nullptr, nullptr, pi, nullptr, nullptr) == DMPC_E_BADARG);
            }
          }
      }
  EXPECT(dmpc_mlp_cost_approx(1 << 12, 1 << 12, 16, 8, 256, 4, p, p, p, p, p, p, p, p, p, p, nullptr) == DMPC_E_UNSUPPORTED);   // T B ns^2 >= 2^31
  EXPECT(dmpc_mlp_cost_param_grad_workspace_bytes(0, 4, 3, 1, 5) == 0 && dmpc_mlp_cost_param_grad_workspace_bytes(4, 0, 3, 1, 5) == 0);
  EXPECT(dmpc_mlp_param_grad_partials(0) == 0 && dmpc_mlp_param_grad_partials(1 << 30) == dmpc_mlp_param_grad_partials(1 << 20));
  EXPECT(dmpc_lqr_shared_workspace_bytes(0, 1, 1, 1) == 0 && dmpc_lqr_shared_saved_bytes(0, 1, 1) == 0);
  EXPECT(dmpc_lqr_kernel_family(0, 3) == DMPC_E_UNSUPPORTED);
  EXPECT(dmpc_lqr_workspace_bytes(0, 1, 1, 1) == 0);
  EXPECT(dmpc_lqr_solve(0, 1, 1, 1, p, p, p, p, p, nullptr, nullptr, nullptr, p, p, nullptr, 0, nullptr, nullptr) == DMPC_E_BADARG);
  EXPECT(dmpc_pnqp(0, 2, p, p, p, p, nullptr, 20, 0, p, p, pi, p, pi, nullptr, 0, pi, nullptr) == DMPC_E_BADARG);
  EXPECT(dmpc_pnqp(4, 2, p, p, p, p, nullptr, 20, 1, p, p, pi, p, pi, nullptr, 0, pi, nullptr) == DMPC_E_WORKSPACE);
  // batch-coupled workspaces (round 5: the fixed-grid form's rows behind the decision slots)
  EXPECT(dmpc_pnqp_workspace_bytes(4, 2, 20, 0) == 0);
  EXPECT(dmpc_pnqp_workspace_bytes(0, 2, 20, 1) == 0);
  for (int n : {1, 2, 8, 9, 40})
    for (int B : {1, 256, 16384})
      EXPECT(dmpc_pnqp_workspace_bytes(B, n, 20, 1) >= dmpc_coupled_workspace_bytes(1, 20) + (size_t)B * 12 * n * sizeof(float));
  for (int nx : {3, 8, 60})
    for (int nu : {1, 2, 9})
      EXPECT(dmpc_mpc_backward_rec_workspace_bytes(10, 64, nx, nu, 20, 1) >
             dmpc_coupled_workspace_bytes(10, 20) + (size_t)64 * (nx + nu) * (nx + nu + 1) * sizeof(float));
  EXPECT(dmpc_mpc_backward_rec(10, 64, 8, 2, p, p, p, p, p, p, p, 20, 1, p, p, pi, p, dmpc_coupled_workspace_bytes(10, 20), pi, nullptr) ==
         DMPC_E_WORKSPACE);
  EXPECT(dmpc_batch_lu_factor(0, 2, p, p, pi, nullptr, nullptr) == DMPC_E_BADARG);
  char name[64];
  (void)dmpc_last_kernel_name(name, sizeof(name));
  (void)dmpc_last_kernel_name(name, 1);
  std::printf("asan_host_driver: %d checks, %d failed\n", checks, bad);
  return bad ? 1 : 0;
}
