// lqr_shared_api.hip - C-ABI of the LQR with batch-shared C and F (include/dmpc.h, dmpc_lqr_shared_*; lqr_shared.hpp).
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "api_util.hpp"
#include "lqr_shared.hpp"

using namespace dmpc;

namespace {

constexpr uint32_t kLayoutBits = DMPC_SHARED_C_TIME | DMPC_SHARED_F_TIME | DMPC_SHARED_CVEC_TIME | DMPC_SHARED_CVEC_BATCH |
                                 DMPC_SHARED_FVEC_TIME | DMPC_SHARED_FVEC_BATCH;

bool shape_ok(int T, int B, int nx, int nu) { return T > 0 && B > 0 && nx > 0 && nu > 0; }
bool shape_supported(int T, int nx, int nu) { return nx <= kSharedMaxNx && nu <= kSharedMaxNu && T <= 65535; }

bool layout_ok(uint32_t layout) {
  if (layout & ~kLayoutBits) return false;
  if ((layout & DMPC_SHARED_CVEC_BATCH) && !(layout & DMPC_SHARED_CVEC_TIME)) return false;
  if ((layout & DMPC_SHARED_FVEC_BATCH) && !(layout & DMPC_SHARED_FVEC_TIME)) return false;
  return true;
}

int n_chunks(int B) { return (B + kSharedChunk - 1) / kSharedChunk; }

size_t kbuf_bytes(int T, int B, int nu) { return round_up((size_t)T * shared_pad_nu(nu) * B * sizeof(float), 256); }

// gradient workspace: k' [T][U][B] | d_tau [T][B][ns] | lambda, d_lambda [T][B][nx] | partials [T][chunk][G][part]
struct GradWs {
  size_t kbuf, dtau, lam, dlam, part, total;
};
GradWs grad_ws(int T, int B, int nx, int nu) {
  GradWs g{};
  const size_t tb = (size_t)T * B;
  g.kbuf = 0;
  g.dtau = g.kbuf + kbuf_bytes(T, B, nu);
  g.lam = g.dtau + round_up(tb * (nx + nu) * sizeof(float), 256);
  g.dlam = g.lam + round_up(tb * nx * sizeof(float), 256);
  g.part = g.dlam + round_up(tb * nx * sizeof(float), 256);
  g.total = g.part + shared_reduce_part_bytes(T, B, nx, nu);
  return g;
}

template <int P, int U>
void launch_affine(int T, int B, int nx, int nu, uint32_t layout, const float *c, const float *f, const float *x_init,
                   const float *ws, float *kbuf, float *x_out, float *u_out, int32_t *info, hipStream_t stream) {
  DMPC_LAUNCH_GGL((lqr_shared_affine_kernel<P, U>), dim3((B + kSharedLaneThreads - 1) / kSharedLaneThreads),
                  dim3(kSharedLaneThreads), 0, stream, T, B, nx, nu, layout, c, f, x_init, ws, kbuf, x_out, u_out, info);
}

template <int P, int U>
void launch_grad_lane(int T, int B, int nx, int nu, uint32_t layout, int strict, const float *c, const float *x,
                      const float *u, const float *gx, const float *gu, const float *ws_saved, float *kbuf, float *dtau,
                      float *lam, float *dlam, float *dx0, float *df, int32_t *info, hipStream_t stream) {
  DMPC_LAUNCH_GGL((lqr_shared_grad_lane_kernel<P, U>), dim3((B + kSharedLaneThreads - 1) / kSharedLaneThreads),
                  dim3(kSharedLaneThreads), 0, stream, T, B, nx, nu, layout, strict, c, x, u, gx, gu, ws_saved, kbuf, dtau,
                  lam, dlam, dx0, df, info);
}

// the padded (P, U) instantiation of a runtime (nx, nu): P in {4, 8, 16, 32}, U in {1, 2, 4, 8}
template <template <int, int> class L, class... A>
void by_size(int nx, int nu, A... a) {
  const int P = shared_pad_nx(nx), U = shared_pad_nu(nu);
#define DMPC_SHARED_CASE(p, u) \
  if (P == p && U == u) return L<p, u>::run(a...);
#define DMPC_SHARED_ROW(p) \
  DMPC_SHARED_CASE(p, 1) DMPC_SHARED_CASE(p, 2) DMPC_SHARED_CASE(p, 4) DMPC_SHARED_CASE(p, 8)
  DMPC_SHARED_ROW(4) DMPC_SHARED_ROW(8) DMPC_SHARED_ROW(16) DMPC_SHARED_ROW(32)
#undef DMPC_SHARED_ROW
#undef DMPC_SHARED_CASE
}

template <int P, int U>
struct Affine {
  template <class... A>
  static void run(A... a) { launch_affine<P, U>(a...); }
};
template <int P, int U>
struct GradLane {
  template <class... A>
  static void run(A... a) { launch_grad_lane<P, U>(a...); }
};

}  // namespace

namespace dmpc {

bool shared_reduce_supported(int T, int nx, int nu) { return shape_supported(T, nx, nu); }

size_t shared_reduce_part_bytes(int T, int B, int nx, int nu) {
  return (size_t)T * n_chunks(B) * shared_red_groups(nx, nu) * shared_part_floats(nx, nu) * sizeof(float);
}

// partial sums per (step, chunk, thread group), then the fixed-order sum of the partials: out_sign * (the reduce kernel's forms)
int shared_grad_reduce(int T, int B, int nx, int nu, uint32_t layout, int strict_math, float out_sign, const float *x,
                       const float *u, const float *dtx, const float *dtu, int dtx_stride, int dtu_stride, const float *lam,
                       const float *dlam, float *part, float *dC, float *dc, float *dF, float *df, hipStream_t stream) {
  const int nchunk = n_chunks(B), G = shared_red_groups(nx, nu);
  DMPC_LAUNCH_GGL(lqr_shared_reduce_kernel, dim3(nchunk, T), dim3(kSharedRedThreads), 0, stream, T, B, nx, nu, strict_math, x,
                  u, dtx, dtu, dtx_stride, dtu_stride, lam, dlam, part);
  const long long outs = (long long)(nx + nu) * (nx + nu) * T + (long long)nx * (nx + nu) * T + (long long)(nx + nu) * T +
                         (long long)nx * T;
  const int grid = (int)(outs < 65536 ? outs : 65536);
  DMPC_LAUNCH_GGL(lqr_shared_finalize_kernel, dim3(grid), dim3(kSharedFinThreads), 0, stream, T, nx, nu, layout, nchunk, G,
                  out_sign, (const float *)part, dC, dc, dF, df);
  return (int)hipGetLastError();
}

}  // namespace dmpc

extern "C" {

size_t dmpc_lqr_shared_saved_bytes(int T, int nx, int nu) {
  if (T <= 0 || nx <= 0 || nu <= 0 || !shape_supported(T, nx, nu)) return 0;
  return round_up(shared_saved_floats(T, nx, nu) * sizeof(float), 256);
}

size_t dmpc_lqr_shared_workspace_bytes(int T, int B, int nx, int nu) {
  if (!shape_ok(T, B, nx, nu) || !shape_supported(T, nx, nu)) return 0;
  return dmpc_lqr_shared_saved_bytes(T, nx, nu) + kbuf_bytes(T, B, nu);
}

size_t dmpc_lqr_shared_grad_workspace_bytes(int T, int B, int nx, int nu) {
  if (!shape_ok(T, B, nx, nu) || !shape_supported(T, nx, nu)) return 0;
  return grad_ws(T, B, nx, nu).total;
}

int dmpc_lqr_shared_solve(int T, int B, int nx, int nu, uint32_t layout, const float *C, const float *c, const float *F,
                          const float *f, const float *x_init, float *x_out, float *u_out, void *ws, size_t ws_bytes,
                          int32_t *info, dmpc_stream_t stream_) {
  if (!shape_ok(T, B, nx, nu) || !layout_ok(layout) || !C || !c || (T > 1 && !F) || !x_init || !x_out || !u_out || !ws)
    return DMPC_E_BADARG;
  if ((layout & DMPC_SHARED_FVEC_BATCH) && !f) return DMPC_E_BADARG;
  for (const void *p : {(const void *)C, (const void *)c, (const void *)F, (const void *)f, (const void *)x_init,
                        (const void *)x_out, (const void *)u_out, (const void *)ws})
    if (!aligned16(p)) return DMPC_E_BADARG;
  if (!shape_supported(T, nx, nu)) return DMPC_E_UNSUPPORTED;
  if (ws_bytes < dmpc_lqr_shared_workspace_bytes(T, B, nx, nu)) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float *wsf = static_cast<float *>(ws);
  float *kbuf = reinterpret_cast<float *>(static_cast<char *>(ws) + dmpc_lqr_shared_saved_bytes(T, nx, nu));
  DMPC_LAUNCH_GGL(lqr_shared_sweep_kernel, dim3(1), dim3(kSharedSweepThreads), 0, stream, T, nx, nu, layout, C, c, F, f,
                  wsf);
  by_size<Affine>(nx, nu, T, B, nx, nu, layout, c, f, x_init, (const float *)wsf, kbuf, x_out, u_out, info, stream);
  return (int)hipGetLastError();
}

int dmpc_lqr_shared_kkt_grad(int T, int B, int nx, int nu, uint32_t layout, const float *C, const float *c, const float *F,
                             const float *x, const float *u, const void *ws_saved, const float *grad_x,
                             const float *grad_u, int strict_math, float *d_x_init, float *dC, float *dc, float *dF,
                             float *df, void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream_) {
  if (!shape_ok(T, B, nx, nu) || !layout_ok(layout) || !C || !c || (T > 1 && !F) || !x || !u || !ws_saved || !grad_x ||
      !grad_u || !d_x_init || !dc || !ws)
    return DMPC_E_BADARG;
  for (const void *p : {(const void *)C, (const void *)c, (const void *)F, (const void *)x, (const void *)u, ws_saved,
                        (const void *)grad_x, (const void *)grad_u, (const void *)d_x_init, (const void *)dC,
                        (const void *)dc, (const void *)dF, (const void *)df, (const void *)ws})
    if (!aligned16(p)) return DMPC_E_BADARG;
  if (!shape_supported(T, nx, nu)) return DMPC_E_UNSUPPORTED;
  if (ws_bytes < dmpc_lqr_shared_grad_workspace_bytes(T, B, nx, nu)) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const GradWs g = grad_ws(T, B, nx, nu);
  char *w = static_cast<char *>(ws);
  const bool cB = layout & DMPC_SHARED_CVEC_BATCH, fB = layout & DMPC_SHARED_FVEC_BATCH;
  // c per trajectory: its gradient IS d_tau, which the lane kernel then writes straight into dc
  float *dtau = cB ? dc : reinterpret_cast<float *>(w + g.dtau);
  float *lam = reinterpret_cast<float *>(w + g.lam), *dlam = reinterpret_cast<float *>(w + g.dlam);
  float *part = reinterpret_cast<float *>(w + g.part);
  by_size<GradLane>(nx, nu, T, B, nx, nu, layout, strict_math ? 1 : 0, c, x, u, grad_x, grad_u,
                    static_cast<const float *>(ws_saved), reinterpret_cast<float *>(w + g.kbuf), dtau, lam, dlam, d_x_init,
                    fB ? df : nullptr, info, stream);
  float *dc_red = cB ? nullptr : dc, *df_red = fB ? nullptr : df;
  return shared_grad_reduce(T, B, nx, nu, layout, strict_math ? 1 : 0, 1.0f, x, u, dtau, dtau + nx, nx + nu, nx + nu, lam, dlam,
                            part, dC, dc_red, dF, df_red, stream);
}

}  // extern "C"
