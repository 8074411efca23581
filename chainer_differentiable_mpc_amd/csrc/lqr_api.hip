// lqr_api.hip - C-ABI entry points of the LQR solve family (include/dmpc.h section A).
// Replaces LqrRecursion.backward/forward/solve_recursion (lqr/lqr_recursion.py:69-209) and
// LQR_active (mpc/active_constrained_lqr.py:67-202) of the reference.
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "api_util.hpp"
#include "knobs.hpp"
#include "lqr_asm_kernel.hpp"
#include "lqr_dma_kernel.hpp"
#include "lqr_generic.hpp"
#include "lqr_tiled.hpp"
#include "lqr_kernels.hpp"
#include "lqr_wave_api.hpp"
#include "lqr_wide_kernel.hpp"

namespace dmpc {

// LDS a 256-thread workgroup may spend on gains before we spill them to HBM.
constexpr size_t kGainLdsBudget = 156 * 1024;   // (round 4: was 64 KB - (8,4) and (12,3) at T = 50 sent their gains through HBM)
// LDS-DMA path: ring depths (timesteps in flight per wave) and the LDS it may use (one workgroup per CU).
#ifndef DMPC_DMA_DEPTH_B
#define DMPC_DMA_DEPTH_B 4
#define DMPC_DMA_DEPTH_F 8
#endif
constexpr int kDmaDepthB = DMPC_DMA_DEPTH_B, kDmaDepthF = DMPC_DMA_DEPTH_F;
constexpr size_t kDmaLdsBudget = 156 * 1024;
constexpr size_t kAsmLdsBudget = 160 * 1024;

// ---- One launcher per kernel template.  A launcher reads from the call only what is an argument form of its kernel (f absent,
// gains wanted, the mask); which kernel takes a call is lqr_route's business alone.

// the generated instruction stream (lqr_asm_kernel.hpp) in one of its forms
template <int NX, int NU, bool STASH, bool MASKED = false, bool GHBM = false, bool SAVE = false, bool AFFINE = false,
          bool ADJ = false>
static int launch_asm(const LqrArgs &a, hipStream_t stream) {
  return with_bools([&](auto has_f, auto write_k) {
    constexpr bool HAS_F = decltype(has_f)::value, WRITE_K = decltype(write_k)::value;
    if constexpr (LqrAsm<NX, NU, WRITE_K, STASH, MASKED, GHBM, SAVE, AFFINE, ADJ>::kAvailable && !(AFFINE && HAS_F))
      return launch_kernel(lqr_asm_kernel<NX, NU, HAS_F, WRITE_K, STASH, MASKED, GHBM, SAVE, AFFINE, ADJ>, four_traj_per_wave_grid(a.B),
                           dim3(256), lqr_asm_lds_bytes<NX, NU, STASH, SAVE, GHBM>(a.T), stream, a);
    else
      return (int)DMPC_E_UNSUPPORTED;   // (no such stream: the route does not send the call here)
  }, a.f != nullptr, a.Ks != nullptr);
}
// ... with the F stash where the route asks for it and the form has one; nullptr: the shape has no stream of this form
template <int NX, int NU, bool STASH, bool MASKED, bool GHBM, bool SAVE, bool AFFINE, bool ADJ>
constexpr bool kAsmForm = LqrAsm<NX, NU, false, STASH, MASKED, GHBM, SAVE, AFFINE, ADJ>::kAvailable ||
                          LqrAsm<NX, NU, true, STASH, MASKED, GHBM, SAVE, AFFINE, ADJ>::kAvailable;   // (with or without gains out)
template <int NX, int NU, bool MASKED = false, bool GHBM = false, bool SAVE = false, bool AFFINE = false, bool ADJ = false>
static LqrLauncher asm_launcher(bool stash) {
  if constexpr (kAsmForm<NX, NU, true, MASKED, GHBM, SAVE, AFFINE, ADJ>) {
    if (stash) return launch_asm<NX, NU, true, MASKED, GHBM, SAVE, AFFINE, ADJ>;
  }
  if constexpr (kAsmForm<NX, NU, false, MASKED, GHBM, SAVE, AFFINE, ADJ>)
    return launch_asm<NX, NU, false, MASKED, GHBM, SAVE, AFFINE, ADJ>;
  return nullptr;
}

// the LDS-DMA ring kernel (lqr_dma_kernel.hpp); KHBM: its gain rows through the workspace
template <int NX, int NU, bool KHBM>
static int launch_dma(const LqrArgs &a, hipStream_t stream) {
  return launch_kernel(lqr_dma_kernel<NX, NU, kDmaDepthB, kDmaDepthF, KHBM>, four_traj_per_wave_grid(a.B), dim3(256),
                       LqrDmaLayout<NX, NU, kDmaDepthB, kDmaDepthF, KHBM>::lds_bytes(a.T), stream, a);
}

// lqr_kernel (lqr_kernels.hpp): a lane group per trajectory.  K_LDS: the gains of a solve stay in LDS; else they pass through
// HBM - the caller's arrays, else the workspace.  PAD: a container
template <int NX, int NU, int L>
constexpr size_t group_gain_bytes(int T) { return (size_t)(256 / L) * T * NU * (NX + 1) * sizeof(float); }
template <int NX, int NU, int L, int MODE, bool K_LDS, bool PAD>
static int launch_group(const LqrArgs &a0, hipStream_t stream) {
  constexpr int GPB = 256 / L;
  LqrArgs a = a0;
  if (!K_LDS && a.Ks == nullptr) { a.Ks = a.wsK; a.ks = a.wsk; }
  return with_bools([&](auto masked) {
    return launch_kernel(lqr_kernel<NX, NU, L, decltype(masked)::value, MODE, K_LDS, PAD>, dim3((a.B + GPB - 1) / GPB), dim3(256),
                         K_LDS ? group_gain_bytes<NX, NU, L>(a.T) : 0, stream, a);
  }, a.mask != nullptr);
}

// the wide row kernel (lqr_wide_kernel.hpp); PAD: a container
template <int NX, int NU, bool PAD>
static int launch_wide(const LqrArgs &a, hipStream_t stream) {
  constexpr int DB = 2, DF = 2;
  constexpr size_t lds = LqrWideLayout<NX, NU, DB, DF>::lds_bytes();
  static_assert(lds <= 160 * 1024, "rings beyond a CU's LDS");
  return with_bools([&](auto masked) {
    return launch_kernel_big_lds(lqr_wide_kernel<NX, NU, DB, DF, PAD, decltype(masked)::value>, dim3((a.B + 15) / 16), dim3(256),
                                 lds, stream, a);
  }, a.mask != nullptr);
}

// the runtime-dimension kernels: their launchers (lqr_generic.hpp, lqr_tiled.hpp) take the mode and the sizes as arguments
template <int MODE>
static int launch_generic(const LqrArgs &a, hipStream_t stream) { return launch_lqr_generic(MODE, a.nx_log, a.nu_log, a, stream); }
template <int MODE>
static int launch_tiled(const LqrArgs &a, hipStream_t stream) {
  return launch_lqr_tiled(MODE, a.nx_log, a.nu_log, a, a.tiled_scratch, stream);
}
static LqrLauncher by_mode(int mode, LqrLauncher solve, LqrLauncher backward, LqrLauncher forward) {
  return mode == kSolve ? solve : mode == kBackwardOnly ? backward : forward;
}

// ---- The order of the code object.  The compiler emits the kernels in the order the translation unit first names them, and
// the generated (8,2) stream runs 6 % slower at another offset of the code object (profiles/r05/lqr_dispatch_refactor_ab.txt).
// These functions name the kernels whose first mention the launchers above would move, in the order the code object has
// had; nothing calls them (route_exact and wide_exact_launcher mention them), and the route names what is left in that order by itself.
template <class... K>
static void name_kernels(K...) {}
template <int NX, int NU, int L>
static void kernel_order() {
  if constexpr (L == 16 && LqrAsm<NX, NU, false, false>::kAvailable) {
    if constexpr (LqrAsm<NX, NU, false, true, false, false, false, true, true>::kAvailable)
      name_kernels(lqr_asm_kernel<NX, NU, false, false, true, false, false, false, true, true>);
    if constexpr (LqrAsm<NX, NU, false, true, false, false, false, true>::kAvailable)
      name_kernels(lqr_asm_kernel<NX, NU, false, false, true, false, false, false, true>);
    if constexpr (LqrAsm<NX, NU, false, true, true>::kAvailable)
      name_kernels(lqr_asm_kernel<NX, NU, true, false, true, true>, lqr_asm_kernel<NX, NU, false, false, true, true>);
    if constexpr (LqrAsm<NX, NU, false, false, true>::kAvailable)
      name_kernels(lqr_asm_kernel<NX, NU, true, false, false, true>, lqr_asm_kernel<NX, NU, false, false, false, true>);
    name_kernels(lqr_asm_kernel<NX, NU, true, true, false>, lqr_asm_kernel<NX, NU, false, true, false>);
    if constexpr (LqrAsm<NX, NU, false, false, false, true>::kAvailable)
      name_kernels(lqr_asm_kernel<NX, NU, true, false, false, false, true>, lqr_asm_kernel<NX, NU, false, false, false, false, true>);
    if constexpr (LqrAsm<NX, NU, false, true>::kAvailable) {
      if constexpr (LqrAsm<NX, NU, true, true, false, false, true>::kAvailable)
        name_kernels(lqr_asm_kernel<NX, NU, true, true, true, false, false, true>,
                     lqr_asm_kernel<NX, NU, false, true, true, false, false, true>);
      name_kernels(lqr_asm_kernel<NX, NU, true, false, true>, lqr_asm_kernel<NX, NU, true, true, true>,
                   lqr_asm_kernel<NX, NU, false, false, true>, lqr_asm_kernel<NX, NU, false, true, true>);
    }
    if constexpr (LqrAsm<NX, NU, true, false, false, false, true>::kAvailable)
      name_kernels(lqr_asm_kernel<NX, NU, true, true, false, false, false, true>,
                   lqr_asm_kernel<NX, NU, false, true, false, false, false, true>);
    name_kernels(lqr_asm_kernel<NX, NU, true, false, false>, lqr_asm_kernel<NX, NU, false, false, false>);
  }
  if constexpr (L == 16)
    name_kernels(lqr_dma_kernel<NX, NU, kDmaDepthB, kDmaDepthF, false>, lqr_kernel<NX, NU, L, true, kSolve, true, false>,
                 lqr_kernel<NX, NU, L, false, kSolve, true, false>, lqr_dma_kernel<NX, NU, kDmaDepthB, kDmaDepthF, true>);
}

// ---- The route: which kernel takes a call.  It launches nothing and dereferences nothing; dispatch_lqr and the queries of
// the C ABI (dmpc_lqr_solve_path, dmpc_lqr_saving_available) all ask it, so what a caller is told is what runs.

// The form of a call, set by the entry point that builds it (the generated streams alone take the last four).
enum class LqrForm {
  kPlain,
  kMasked,    // LQR_active: a.mask
  kSplitC,    // DiffLqr.backward's second solve: c as two arrays (a.c, a.c_u), x_init = 0, f = 0
  kSaved,     // the affine re-solve from saved gains (a.Ks_in, a.Quu_in, a.Qxu_in)
  kAdjoint,   // ... whose rollout writes the gradients (a.Vv_in)
  kSaving     // the training form: Quu, Qxu, [V | v] saved next to the gains
};
struct LqrCall {
  int mode;   // LqrMode
  LqrForm form;
  int T, B, nx, nu;
  bool gains;         // the caller takes the gains (a.Ks, a.ks)
  bool ws, scratch;   // a workspace for gain rows / the tiled kernel's scratch behind it were given
  bool mask_dwords;   // the mask can be fetched as dwords: its base is 4-byte aligned
};
struct LqrRoute {
  int path;                                       // DMPC_LQR_PATH_*, or the DMPC_E_* of a refusal
  LqrLauncher launch = nullptr, then = nullptr;   // then: the second launch of a chain (sweep, then rollout)
};

// the kernels that give a wavefront four trajectories: at least one whole wavefront, a horizon with an F
static bool fills_a_wave(int T, int B) { return B >= 4 && T >= 2; }
// ... and whose stream has no ragged last wavefront (the saving and the affine forms)
static bool whole_waves(int B) { return B % 4 == 0; }
// gains that pass through HBM have a place: the caller's arrays, else the workspace
static bool gains_have_a_place(const LqrCall &q) { return q.gains || q.ws; }

// the form of the generated stream that serves a solve of this size (ASM_STASH, ASM_RING, ASM_WS), or -1
template <int NX, int NU>
static int asm_path(int T, int B) {
  if constexpr (LqrAsm<NX, NU, false, false>::kAvailable) {
    if (!fills_a_wave(T, B) || knob_on<Knob::DMPC_NO_ASM>()) return -1;
    if constexpr (LqrAsm<NX, NU, false, true>::kAvailable) {
      if (T <= LqrAsm<NX, NU, false, true>::NSTASH && lqr_asm_lds_bytes<NX, NU, true>(T) <= kAsmLdsBudget &&
          !knob_on<Knob::DMPC_NO_STASH>())
        return DMPC_LQR_PATH_ASM_STASH;
    }
    if (lqr_asm_lds_bytes<NX, NU, false>(T) <= kAsmLdsBudget) return DMPC_LQR_PATH_ASM_RING;
    if constexpr (LqrAsm<NX, NU, false, false, false, true>::kAvailable) {
      if (lqr_asm_lds_bytes<NX, NU, false, false, true>(T) <= kAsmLdsBudget) return DMPC_LQR_PATH_ASM_WS;
    }
  }
  return -1;
}

// lqr_kernel by mode; a solve keeps its gains in LDS while they fit (`told`: the path code of the kernel's family)
template <int NX, int NU, int L, bool PAD>
static LqrRoute route_group(const LqrCall &q, int told) {
  if (q.mode == kSolve) {
    if (group_gain_bytes<NX, NU, L>(q.T) <= kGainLdsBudget) return {told, launch_group<NX, NU, L, kSolve, true, PAD>};
    if (!gains_have_a_place(q)) return {DMPC_E_WORKSPACE};
    return {told, launch_group<NX, NU, L, kSolve, false, PAD>};
  }
  return {told, by_mode(q.mode, nullptr, launch_group<NX, NU, L, kBackwardOnly, false, PAD>,
                        launch_group<NX, NU, L, kForwardOnly, false, PAD>)};
}

// a shape with a specialisation of its own
template <int NX, int NU, int L>
static LqrRoute route_exact(const LqrCall &q) {
  (void)&kernel_order<NX, NU, L>;   // (instantiated first: the order of the code object)
  const int T = q.T, B = q.B;
  const bool masked = q.form == LqrForm::kMasked, plain = q.mode == kSolve && q.form == LqrForm::kPlain;
  const LqrRoute refused{DMPC_E_UNSUPPORTED};
  if constexpr (L == 16 && LqrAsm<NX, NU, false, false>::kAvailable) {
    // fastest: the whole solve as one generated instruction stream; with the F stash (no second read of F) when the horizon fits
    // the stash registers.  ap: the form a plain solve takes.  The stash form's LDS holds the ring form's (one ring per shape,
    // the f area on top), so a horizon that takes the stash form also fits the ring form's sweep
    if constexpr (LqrAsm<NX, NU, false, true>::kAvailable)
      static_assert(lqr_asm_lds_bytes<NX, NU, true>(1) >= lqr_asm_lds_bytes<NX, NU, false>(1),
                    "the stash form's LDS holds the ring form's");
    const int ap = asm_path<NX, NU>(T, B);
    const bool stash = ap == DMPC_LQR_PATH_ASM_STASH, in_lds = stash || ap == DMPC_LQR_PATH_ASM_RING;
    const bool stash_whole = stash && whole_waves(B);   // what the saving and the affine forms ask for
    if (q.form == LqrForm::kSaving) {
      // the stash form alone, with room in LDS for the staging area of the saved blocks.  (asm_launcher also names the ring form
      // of the saving stream, as the dispatch always has: those instances are compiled and no call reaches them)
      bool room = false;
      if constexpr (LqrAsm<NX, NU, true, true, false, false, true>::kAvailable)
        room = stash_whole && lqr_asm_lds_bytes<NX, NU, true, true>(T) <= kAsmLdsBudget;
      return room ? LqrRoute{ap, asm_launcher<NX, NU, false, false, true>(stash)} : refused;
    }
    if (q.form == LqrForm::kSaved || q.form == LqrForm::kAdjoint) {   // affine streams: F in the stash, whole wavefronts
      if (!stash_whole) return refused;
      if constexpr (LqrAsm<NX, NU, false, true, false, false, false, true, true>::kAvailable) {
        if (q.form == LqrForm::kAdjoint) return {ap, launch_asm<NX, NU, true, false, false, false, true, true>};
      }
      if constexpr (LqrAsm<NX, NU, false, true, false, false, false, true>::kAvailable) {
        if (q.form == LqrForm::kSaved) return {ap, launch_asm<NX, NU, true, false, false, false, true>};
      }
      return refused;
    }
    if (q.form == LqrForm::kSplitC) return in_lds ? LqrRoute{ap, asm_launcher<NX, NU>(stash)} : refused;
    if constexpr (LqrAsm<NX, NU, false, false, true>::kAvailable) {
      // LQR_active on the stream: flags fetched as dwords (B * nu a multiple of 4); the caller's Ks / ks are another layout
      if (q.mode == kSolve && masked && !q.gains && (B * NU) % 4 == 0 && q.mask_dwords && in_lds)
        return {ap, asm_launcher<NX, NU, true>(stash)};
    }
    // LqrRecursion.backward(): the ring form's sweep with the gains written to HBM (x == nullptr)
    if (q.mode == kBackwardOnly && !masked && in_lds) return {DMPC_LQR_PATH_ASM_RING, launch_asm<NX, NU, false>};
    // long horizons: the gain rows pass through the workspace instead of LDS (a solve that wants the gains goes to the kernels below)
    if (plain && ap == DMPC_LQR_PATH_ASM_WS && !q.gains && q.ws) return {ap, launch_asm<NX, NU, false, false, true>};
    if (plain && in_lds) return {ap, asm_launcher<NX, NU>(stash)};
  }
  if (q.form != LqrForm::kPlain && !masked) return refused;   // (nothing else reads the streams' own argument forms)
  if constexpr (L == 64 && NX % 4 == 0 && NU % 4 == 0) {
    // large shapes: backward sweep on the matrix cores (lqr_wave_api.hip; plain and LQR_active), gains through HBM; the wavefront
    // that finished a trajectory's sweep rolls it out in the same launch
    if (q.mode != kForwardOnly) {
      if (const LqrLauncher sweep = lqr_wave_exact_launcher(NX, NU, masked, q.mode == kSolve))
        return gains_have_a_place(q) ? LqrRoute{DMPC_LQR_PATH_WAVE_MFMA, sweep} : LqrRoute{DMPC_E_WORKSPACE};
    }
  }
  if constexpr (L == 16) {
    // LDS-DMA staged inputs (lqr_dma_kernel.hpp): the plain solve, gains + rings within the LDS of a CU - or, once the gains of
    // lqr_kernel no longer fit LDS either, with its gain rows through the workspace (its rings alone fit at any horizon).  Measured
    // against lqr_kernel (profiles/r04/khbm_vs_lqr_kernel.txt): behind it while the gains still fit LDS ((8,4) T = 50: 96 against
    // 84 us - hence only then), level at T = 100, ahead at T = 200 ((4,4): 221 against 267 us).  (Told as PREFETCH: the path codes
    // are older than that form)
    if (plain && fills_a_wave(T, B) && !knob_on<Knob::DMPC_NO_DMA>()) {
      if (LqrDmaLayout<NX, NU, kDmaDepthB, kDmaDepthF>::lds_bytes(T) <= kDmaLdsBudget)
        return {DMPC_LQR_PATH_DMA, launch_dma<NX, NU, false>};
      if (group_gain_bytes<NX, NU, L>(T) > kGainLdsBudget && q.ws && !q.gains &&
          LqrDmaLayout<NX, NU, kDmaDepthB, kDmaDepthF, true>::lds_bytes(T) <= kDmaLdsBudget)
        return {DMPC_LQR_PATH_PREFETCH, launch_dma<NX, NU, true>};
    }
  }
  return route_group<NX, NU, L, false>(q, DMPC_LQR_PATH_PREFETCH);
}

// quick single-shape builds for kernel experiments (scripts/*variants.sh): no containers, and no wide kernels unless
// DMPC_EXPERIMENT_WITH_WIDE
#if defined(DMPC_EXPERIMENT_ONLY_32_8) || defined(DMPC_EXPERIMENT_ONLY_8_2) || defined(DMPC_EXPERIMENT_ONLY_4_4) || \
    defined(DMPC_EXPERIMENT_ONLY_8_4)
#define DMPC_EXPERIMENT_ONE_SHAPE
#endif

// The shapes with a register-resident specialisation.  Anything else (ns + 1 <= 64) goes to the
// runtime-dimension LDS kernel in lqr_generic.hpp.
#if defined(DMPC_EXPERIMENT_ONLY_32_8)
#define DMPC_LQR_SHAPES(X) X(32, 8, 64)
#elif defined(DMPC_EXPERIMENT_ONLY_8_2)
#define DMPC_LQR_SHAPES(X) X(8, 2, 16)
#elif defined(DMPC_EXPERIMENT_ONLY_4_4)
#define DMPC_LQR_SHAPES(X) X(4, 4, 16)
#elif defined(DMPC_EXPERIMENT_ONLY_8_4)
#define DMPC_LQR_SHAPES(X) X(8, 4, 16)
#else
#define DMPC_LQR_SHAPES(X) \
  X(1, 1, 16) X(2, 1, 16) X(3, 1, 16) X(2, 2, 16) X(3, 2, 16) X(4, 2, 16) X(6, 2, 16) X(8, 2, 16) \
  X(4, 4, 16) X(8, 4, 16) X(12, 3, 16) X(32, 8, 64)
#endif

// Containers: register-resident kernels that also take any SMALLER problem (lqr_kernel<..., PAD>; the loads pad it in
// place), in the order they are tried - fewest columns first, fewest controls among equals.  Every shape with
// nx + nu <= 15 and nu <= 8 has one.
#ifdef DMPC_EXPERIMENT_ONE_SHAPE
#define DMPC_LQR_CONTAINERS(X)
#else
// (round 4: five to eight controls too - the gain solve on the rows needs no NU x NU LU per lane; before, (5,5) ran a
// wavefront per trajectory inside the (16,8) matrix-core kernel at 0.03 of the roof)
#define DMPC_LQR_CONTAINERS(X) X(3, 1) X(4, 4) X(8, 2) X(5, 5) X(8, 4) X(14, 1) X(13, 2) X(12, 3) X(11, 4) X(10, 5) X(9, 6) X(8, 7) X(7, 8)
#endif

// ... and the wavefront-per-trajectory kernels take what is larger, up to 32 states and 8 controls
#ifdef DMPC_EXPERIMENT_ONE_SHAPE
#define DMPC_LQR_WAVE_CONTAINERS(X)
#else
#define DMPC_LQR_WAVE_CONTAINERS(X) X(16, 8) X(32, 8)
#endif

// 17 to 32 augmented columns with at most 16 states: the wide 16-lane row kernel (lqr_wide_kernel.hpp; two registers per
// matrix row, four trajectories per wavefront) for the plain fused solve of exactly these shapes - round 4; before, a
// wavefront per trajectory inside the (16,8) matrix-core instance.  DMPC_NO_WIDE=1: that path (A/B timing).
#if defined(DMPC_EXPERIMENT_ONE_SHAPE) && !defined(DMPC_EXPERIMENT_WITH_WIDE)
#define DMPC_LQR_WIDE_SHAPES(X)
#else
#define DMPC_LQR_WIDE_SHAPES(X) X(16, 4) X(16, 8) X(12, 4) X(12, 8)
/* ((8,4) as a one-register instance of the same kernel - the template takes it - measured 94 us against lqr_kernel's 84: not used) */
#endif
#define DMPC_LQR_WIDE_CONTAINERS(X) X(12, 4) X(16, 4) X(12, 8) X(16, 8)   /* fewest columns first */
// (kernel_order above: the wide kernels, plain before LQR_active)
[[maybe_unused]] static void kernel_order_wide() {
#define X(NX_, NU_) name_kernels(lqr_wide_kernel<NX_, NU_, 2, 2, false, false>, lqr_wide_kernel<NX_, NU_, 2, 2, false, true>);
  DMPC_LQR_WIDE_SHAPES(X)
#undef X
#define X(NX_, NU_) name_kernels(lqr_wide_kernel<NX_, NU_, 2, 2, true, false>, lqr_wide_kernel<NX_, NU_, 2, 2, true, true>);
  DMPC_LQR_WIDE_CONTAINERS(X)
#undef X
}
static LqrLauncher wide_exact_launcher(int nx, int nu) {
#define X(NX_, NU_) \
  if (nx == NX_ && nu == NU_) return launch_wide<NX_, NU_, false>;
  DMPC_LQR_WIDE_SHAPES(X)
#undef X
  return nullptr;
}
// ... and, padded by its reads (lqr_wide_kernel<..., PAD>), of every other shape with at most 16 states and 8 controls that has
// no 16-lane container (nx + nu >= 16): smallest instance first.  Before, all of them took a wavefront per trajectory.
static bool wide_container_shape(int nx, int nu) {
  return nx >= 1 && nu >= 1 && nx <= 16 && nu <= 8 && nx + nu >= 16 && wide_exact_launcher(nx, nu) == nullptr;
}
// The wide kernel's launcher where it can take a solve of this size, else nullptr: whole wavefronts of four trajectories (a
// padded shape: nothing but), a horizon with an F, 32-bit time strides.  Its gain rows travel through the caller's workspace,
// rows of the INSTANCE's width - dmpc_lqr_workspace_bytes allows for it.
static LqrLauncher wide_launcher(int T, int B, int nx, int nu) {
  if (knob_on<Knob::DMPC_NO_WIDE>() || !fills_a_wave(T, B) || (size_t)B * (nx + nu) * (nx + nu) * 4 >= ((size_t)1 << 31))
    return nullptr;
  if (const LqrLauncher exact = wide_exact_launcher(nx, nu)) return exact;
  if (!wide_container_shape(nx, nu) || !whole_waves(B) || knob_on<Knob::DMPC_NO_CONTAINER>()) return nullptr;
#define X(NX_, NU_) \
  if (nx <= NX_ && nu <= NU_) return launch_wide<NX_, NU_, true>;
  DMPC_LQR_WIDE_CONTAINERS(X)
#undef X
  return nullptr;
}
constexpr size_t kWideContainerGainFloats = 8 * 25;   // gain rows of a wide container, per trajectory-step: at most 8 rows of 25

static bool has_container(int nx, int nu) {
#define X(NX_, NU_) \
  if (nx <= NX_ && nu <= NU_) return true;
  DMPC_LQR_CONTAINERS(X)
  DMPC_LQR_WAVE_CONTAINERS(X)
#undef X
  return false;
}

static int lqr_family(int nx, int nu) {
#define X(NX_, NU_, L_) \
  if (nx == NX_ && nu == NU_) return L_ == 16 ? DMPC_LQR_FAMILY_ROW16 : DMPC_LQR_FAMILY_WAVE;
  DMPC_LQR_SHAPES(X)
#undef X
  if (nx >= 1 && nu >= 1 && has_container(nx, nu)) return DMPC_LQR_FAMILY_CONTAINER;
  if (nx >= 1 && nu >= 1 && nx + nu + 1 <= kGenericMaxCols && lqr_generic_lds_bytes(1, nx, nu, false) <= 64 * 1024)
    return DMPC_LQR_FAMILY_GENERIC;
  // any size: a workgroup per trajectory, matrices in the caller's workspace (lqr_tiled.hpp)
  if (nx >= 1 && nu >= 1) return DMPC_LQR_FAMILY_TILED;
  return DMPC_E_UNSUPPORTED;
}

// a wider problem (up to 32 states, 8 controls) inside the wavefront-per-trajectory instance (NX, NU): sweep on the matrix cores,
// gains through HBM, then the rollout - staged through LDS where that applies, else the forward-only container kernel
template <int NX, int NU>
static LqrRoute route_wave_container(const LqrCall &q) {
  const bool masked = q.form == LqrForm::kMasked;
  LqrLauncher forward = lqr_staged_forward_launcher(q.T, q.nx, q.nu, masked);
  if (forward == nullptr) forward = launch_group<NX, NU, 64, kForwardOnly, false, true>;
  if (q.mode == kForwardOnly) return {DMPC_LQR_PATH_CONTAINER, forward};
  if (!gains_have_a_place(q)) return {DMPC_E_WORKSPACE};
  // a size that IS one of the instances: the exact kernel (rollout in the same launch)
  if (const LqrLauncher exact = lqr_wave_exact_launcher(q.nx, q.nu, masked, q.mode == kSolve))
    return {DMPC_LQR_PATH_CONTAINER, exact};
  return {DMPC_LQR_PATH_CONTAINER, lqr_wave_padded_sweep_launcher(q.nx, q.nu, masked), q.mode == kSolve ? forward : nullptr};
}

static LqrRoute lqr_route(const LqrCall &q) {
  const int nx = q.nx, nu = q.nu;
  const bool plain_or_masked = q.form == LqrForm::kPlain || q.form == LqrForm::kMasked;
  if (q.mode == kSolve && plain_or_masked && q.ws) {
    if (const LqrLauncher wide = wide_launcher(q.T, q.B, nx, nu)) return {DMPC_LQR_PATH_WIDE, wide};
  }
#define X(NX_, NU_, L_) \
  if (nx == NX_ && nu == NU_) return route_exact<NX_, NU_, L_>(q);
  DMPC_LQR_SHAPES(X)
#undef X
  if (!plain_or_masked) return {DMPC_E_UNSUPPORTED};   // (nothing else reads the generated streams' own argument forms)
  const int family = lqr_family(nx, nu);
  // a problem without a specialisation of its own, in the smallest container that holds it
  if (family == DMPC_LQR_FAMILY_CONTAINER && !knob_on<Knob::DMPC_NO_CONTAINER>()) {
#define X(NX_, NU_) \
  if (nx <= NX_ && nu <= NU_) return route_group<NX_, NU_, 16, true>(q, DMPC_LQR_PATH_CONTAINER);
    DMPC_LQR_CONTAINERS(X)
#undef X
#define X(NX_, NU_) \
  if (nx <= NX_ && nu <= NU_) return route_wave_container<NX_, NU_>(q);
    DMPC_LQR_WAVE_CONTAINERS(X)
#undef X
  }
  // (the generic kernel's matrices fit LDS at every size of these two families: lqr_family says so for GENERIC, a container's
  // size is below it - the tiled kernel is for the rest)
  if (family == DMPC_LQR_FAMILY_GENERIC || family == DMPC_LQR_FAMILY_CONTAINER)
    return {DMPC_LQR_PATH_GENERIC,
            by_mode(q.mode, launch_generic<kSolve>, launch_generic<kBackwardOnly>, launch_generic<kForwardOnly>)};
  if (family != DMPC_LQR_FAMILY_TILED) return {DMPC_E_UNSUPPORTED};
  if (q.mode != kForwardOnly && !(q.scratch && gains_have_a_place(q))) return {DMPC_E_WORKSPACE};   // the sweep's matrices live there
  return {DMPC_LQR_PATH_TILED, by_mode(q.mode, launch_tiled<kSolve>, launch_tiled<kBackwardOnly>, launch_tiled<kForwardOnly>)};
}

// (writes the problem's dimensions into the entry point's own `a`: the containers read them, the other kernels ignore them)
static int dispatch_lqr(int mode, LqrForm form, int nx, int nu, LqrArgs &a, hipStream_t stream) {
  const LqrRoute r = lqr_route({mode, form, a.T, a.B, nx, nu, a.Ks != nullptr, a.wsK != nullptr, a.tiled_scratch != nullptr,
                                (reinterpret_cast<uintptr_t>(a.mask) & 3u) == 0});
  if (r.path < 0) return r.path;   // (nothing launched)
  a.nx_log = nx;
  a.nu_log = nu;
  const int rc = r.launch(a, stream);
  return rc != 0 || r.then == nullptr ? rc : r.then(a, stream);
}

// the arguments every form of a call has
static LqrArgs lqr_args(int T, int B, const float *C, const float *c, const float *F, const float *f, const float *x_init,
                        float *x, float *u, int32_t *info) {
  LqrArgs a{};
  a.T = T; a.B = B;
  a.C = C; a.c = c; a.F = F; a.f = f; a.x_init = x_init;
  a.x = x; a.u = u; a.info = info;
  return a;
}
static void set_saved_gains(LqrArgs &a, const float *Ks, const float *Quu, const float *Qxu) {
  a.Ks_in = Ks; a.Quu_in = Quu; a.Qxu_in = Qxu;
}

// DiffLqr.backward's second solve (differentiable_lqr.py:108-114) without a concatenated copy of its inputs: c = [cx; cu]
// as two arrays, x_init = 0, f = 0; with Ks != nullptr the re-solve from saved gains.  DMPC_E_UNSUPPORTED (nothing
// launched) unless a generated stream serves the size.
int lqr_second_solve(int T, int B, int nx, int nu, const float *C, const float *cx, const float *cu, const float *F,
                     const float *Ks, const float *Quu, const float *Qxu, float *x_out, float *u_out, int32_t *info,
                     hipStream_t stream) {
  LqrArgs a = lqr_args(T, B, C, cx, F, nullptr, nullptr, x_out, u_out, info);
  a.c_u = cu;
  if (Ks != nullptr) set_saved_gains(a, Ks, Quu, Qxu);
  return dispatch_lqr(kSolve, Ks != nullptr ? LqrForm::kSaved : LqrForm::kSplitC, nx, nu, a, stream);
}

// DiffLqr.backward (differentiable_lqr.py:78-142) in ONE launch that reads neither C nor c: the affine re-solve from the
// saving solve's K_t, Quu_t, Qxu_t on [grad_x; grad_u], whose rollout of d_tau forms lambda_t = V_t x_t + v_t and
// d_lambda_t = V_t dx_t + v'_t from the saved value functions Vv and writes dC, dc, dF, df, dx_init itself.
// DMPC_E_UNSUPPORTED (nothing launched) unless the generated stream serves the size.
int lqr_adjoint(int T, int B, int nx, int nu, const float *F, const float *grad_x, const float *grad_u, const float *Ks,
                const float *Quu, const float *Qxu, const float *Vv, const float *x, const float *u, int strict_math,
                float *d_x_init, float *dC, float *dc, float *dF, float *df, int32_t *info, hipStream_t stream) {
  LqrArgs a = lqr_args(T, B, nullptr, grad_x, F, nullptr, nullptr, nullptr, nullptr, info);
  a.c_u = grad_u;
  set_saved_gains(a, Ks, Quu, Qxu);
  a.Vv_in = Vv;
  a.tau_x = x;
  a.tau_u = u;
  a.dC = dC; a.dc = dc; a.dF = dF; a.df = df; a.dx0 = d_x_init;
  a.w_a = 0.5f;
  a.w_b = strict_math ? 0.5f : 1.0f;
  a.df_shift = strict_math ? 1 : 0;
  return dispatch_lqr(kSolve, LqrForm::kAdjoint, nx, nu, a, stream);
}

}  // namespace dmpc

using namespace dmpc;

// what a caller is told: the route of a solve of this form that brings the workspace (the queries have no pointers to go by)
static LqrRoute told_route(int T, int B, int nx, int nu, LqrForm form, bool gains) {
  return lqr_route({kSolve, form, T, B, nx, nu, gains, true, true, true});
}
// gain rows in the workspace: [T,B,nu,nx] + [T,B,nu], or - the generated stream at long horizons - rows of 12 floats
// [K_m | 0 | k_m | pad], or rows of nx + nu + 1 floats (the LDS-DMA kernel's workspace form)
static size_t gain_ws_bytes(int T, int B, int nx, int nu) {
  return (size_t)T * B * nu * (nx + nu + 1 > 12 ? nx + nu + 1 : 12) * sizeof(float);
}

extern "C" {

int dmpc_version(void) { return DMPC_VERSION; }

int dmpc_lqr_kernel_family(int nx, int nu) { return lqr_family(nx, nu); }

int dmpc_lqr_solve_path(int T, int B, int nx, int nu) {
  if (T <= 0 || B <= 0) return DMPC_E_BADARG;
  return told_route(T, B, nx, nu, LqrForm::kPlain, false).path;   // a plain solve that takes no gains
}

int dmpc_lqr_saving_available(int T, int B, int nx, int nu) {
  return T > 0 && B > 0 && told_route(T, B, nx, nu, LqrForm::kSaving, true).path >= 0;
}

size_t dmpc_lqr_workspace_bytes(int T, int B, int nx, int nu) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return 0;
  // only touched when the gains do not fit in LDS (long horizons) or by the generic kernel
  size_t bytes = gain_ws_bytes(T, B, nx, nu);
  // (a shape padded inside an instance of the wide row kernel: gain rows of the INSTANCE's width)
  if (wide_container_shape(nx, nu)) bytes = (size_t)T * B * kWideContainerGainFloats * sizeof(float);
  // the shapes beyond a wavefront's 64 columns (the tiled family) keep the matrices of every trajectory behind the gains
  if (lqr_family(nx, nu) == DMPC_LQR_FAMILY_TILED)
    bytes = round_up(bytes, 256) + (size_t)B * tiled_scratch_floats(nx, nu) * sizeof(float);
  return bytes;
}

static float *tiled_scratch_of(void *ws, int T, int B, int nx, int nu) {
  if (ws == nullptr || lqr_family(nx, nu) != DMPC_LQR_FAMILY_TILED) return nullptr;
  return reinterpret_cast<float *>(static_cast<char *>(ws) + round_up(gain_ws_bytes(T, B, nx, nu), 256));
}

int dmpc_lqr_solve(int T, int B, int nx, int nu, const float *C, const float *c, const float *F,
                   const float *f, const float *x_init, const uint8_t *u_zero_mask, float *Ks_out,
                   float *ks_out, float *x_out, float *u_out, void *ws, size_t ws_bytes, int32_t *info,
                   dmpc_stream_t stream) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!C || !c || !x_init || !x_out || !u_out || (T > 1 && !F)) return DMPC_E_BADARG;
  if ((Ks_out == nullptr) != (ks_out == nullptr)) return DMPC_E_BADARG;
  if (!aligned16(C) || !aligned16(c) || !aligned16(F) || !aligned16(f)) return DMPC_E_BADARG;
  LqrArgs a = lqr_args(T, B, C, c, F, f, x_init, x_out, u_out, info);
  a.mask = u_zero_mask;
  a.Ks = Ks_out; a.ks = ks_out;
  if (ws != nullptr) {
    if (ws_bytes < dmpc_lqr_workspace_bytes(T, B, nx, nu)) return DMPC_E_WORKSPACE;
    a.wsK = static_cast<float *>(ws);
    a.wsk = a.wsK + (size_t)T * B * nu * nx;
    a.tiled_scratch = tiled_scratch_of(ws, T, B, nx, nu);
  }
  return dispatch_lqr(kSolve, u_zero_mask ? LqrForm::kMasked : LqrForm::kPlain, nx, nu, a, static_cast<hipStream_t>(stream));
}

int dmpc_lqr_solve_saving(int T, int B, int nx, int nu, const float *C, const float *c, const float *F,
                          const float *f, const float *x_init, float *Ks_out, float *ks_out, float *Quu_out,
                          float *Qxu_out, float *Vv_out, float *x_out, float *u_out, int32_t *info, dmpc_stream_t stream) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!C || !c || !F || !x_init || !x_out || !u_out || !Ks_out || !ks_out || !Quu_out || !Qxu_out || !Vv_out)
    return DMPC_E_BADARG;
  if (!aligned16(C) || !aligned16(c) || !aligned16(F) || !aligned16(f) || !aligned16(Quu_out)) return DMPC_E_BADARG;
  LqrArgs a = lqr_args(T, B, C, c, F, f, x_init, x_out, u_out, info);
  a.Ks = Ks_out; a.ks = ks_out;
  a.Quu_out = Quu_out; a.Qxu_out = Qxu_out; a.Vv_out = Vv_out;
  a.info_store = true;
  return dispatch_lqr(kSolve, LqrForm::kSaving, nx, nu, a, static_cast<hipStream_t>(stream));   // (the stash form of the stream only)
}

int dmpc_lqr_saved_solve(int T, int B, int nx, int nu, const float *c, const float *F, const float *Ks,
                         const float *Quu, const float *Qxu, const float *x_init, float *x_out, float *u_out,
                         int32_t *info, dmpc_stream_t stream) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!c || !F || !Ks || !Quu || !Qxu || !x_init || !x_out || !u_out) return DMPC_E_BADARG;
  if (!aligned16(c) || !aligned16(F) || !aligned16(Ks) || !aligned16(Quu) || !aligned16(Qxu)) return DMPC_E_BADARG;
  LqrArgs a = lqr_args(T, B, nullptr, c, F, nullptr, x_init, x_out, u_out, info);
  set_saved_gains(a, Ks, Quu, Qxu);
  return dispatch_lqr(kSolve, LqrForm::kSaved, nx, nu, a, static_cast<hipStream_t>(stream));
}

int dmpc_lqr_backward_sweep_ws(int T, int B, int nx, int nu, const float *C, const float *c, const float *F,
                               const float *f, const uint8_t *u_zero_mask, float *Ks_out, float *ks_out, void *ws,
                               size_t ws_bytes, int32_t *info, dmpc_stream_t stream) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!C || !c || !Ks_out || !ks_out || (T > 1 && !F)) return DMPC_E_BADARG;
  if (!aligned16(C) || !aligned16(c) || !aligned16(F) || !aligned16(f)) return DMPC_E_BADARG;
  LqrArgs a = lqr_args(T, B, C, c, F, f, nullptr, nullptr, nullptr, info);
  a.mask = u_zero_mask;
  a.Ks = Ks_out; a.ks = ks_out;
  if (ws != nullptr) {
    if (ws_bytes < dmpc_lqr_workspace_bytes(T, B, nx, nu)) return DMPC_E_WORKSPACE;
    a.tiled_scratch = tiled_scratch_of(ws, T, B, nx, nu);
  }
  return dispatch_lqr(kBackwardOnly, u_zero_mask ? LqrForm::kMasked : LqrForm::kPlain, nx, nu, a, static_cast<hipStream_t>(stream));
}

int dmpc_lqr_backward_sweep(int T, int B, int nx, int nu, const float *C, const float *c, const float *F,
                            const float *f, const uint8_t *u_zero_mask, float *Ks_out, float *ks_out,
                            int32_t *info, dmpc_stream_t stream) {
  return dmpc_lqr_backward_sweep_ws(T, B, nx, nu, C, c, F, f, u_zero_mask, Ks_out, ks_out, nullptr, 0, info, stream);
}

int dmpc_lqr_forward_sweep(int T, int B, int nx, int nu, const float *Ks, const float *ks, const float *F,
                           const float *f, const float *x_init, const uint8_t *u_zero_mask, float *x_out,
                           float *u_out, int32_t *info, dmpc_stream_t stream) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!Ks || !ks || !x_init || !x_out || !u_out || (T > 1 && !F)) return DMPC_E_BADARG;
  if (!aligned16(F) || !aligned16(f)) return DMPC_E_BADARG;
  LqrArgs a = lqr_args(T, B, nullptr, nullptr, F, f, x_init, x_out, u_out, info);
  a.mask = u_zero_mask;
  a.Ks = const_cast<float *>(Ks); a.ks = const_cast<float *>(ks);
  return dispatch_lqr(kForwardOnly, u_zero_mask ? LqrForm::kMasked : LqrForm::kPlain, nx, nu, a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
