// knobs.hpp - the DMPC_* environment switches the library reads, and the only place in csrc/ that calls getenv.
// Diagnostics only ("Diagnostics switches"): each one takes a kernel out of reach so that two kernels for
// the same call can be timed or compared.  A flag is on when its value starts with '1'; an integer is read with atoll.
// kLatched: read once per process, at its first use.  kPerCall: read at every use (tests flip these inside one process).
#pragma once
#include <cstdlib>

namespace dmpc {

enum KnobRead { kLatched, kPerCall };

// X(name, read mode, value when unset)
#define DMPC_KNOBS(X)                        \
  X(DMPC_NO_ASM, kLatched, 0)                \
  X(DMPC_NO_STASH, kLatched, 0)              \
  X(DMPC_NO_DMA, kLatched, 0)                \
  X(DMPC_NO_WAVE_MFMA, kLatched, 0)          \
  X(DMPC_NO_WIDE, kLatched, 0)               \
  X(DMPC_NO_CONTAINER, kLatched, 0)          \
  X(DMPC_NO_TILE16, kLatched, 0)             \
  X(DMPC_NO_STAGED_FWD, kLatched, 0)         \
  X(DMPC_NO_STAGED_COSTATE, kLatched, 0)     \
  X(DMPC_NO_COSTATE_DMA, kLatched, 0)        \
  X(DMPC_COSTATE_WIDE_MIN_NS, kLatched, 13)  \
  X(DMPC_NO_ADJOINT, kLatched, 0)            \
  X(DMPC_NO_F64_ROW, kLatched, 0)            \
  X(DMPC_NO_F64_TILE16, kLatched, 0)         \
  X(DMPC_NO_MPC_ASM, kLatched, 0)            \
  X(DMPC_NO_MPC_DMA, kLatched, 0)            \
  X(DMPC_NO_MPC_WAVE, kLatched, 0)           \
  X(DMPC_NO_MPC_FUSED, kLatched, 0)          \
  X(DMPC_NO_MPC_STAGED_FWD, kLatched, 0)     \
  X(DMPC_NO_SPEC_LS, kLatched, 0)            \
  X(DMPC_NO_SPEC4, kLatched, 0)              \
  X(DMPC_NO_COOP_REGISTER, kPerCall, 0)      \
  X(DMPC_FIXED_GRID_MAX, kPerCall, 0)        \
  X(DMPC_NO_DDP_ITER_FUSED, kPerCall, 0)

enum class Knob {
#define X(NAME, READ, UNSET) NAME,
  DMPC_KNOBS(X)
#undef X
};
struct KnobInfo { const char *name; KnobRead read; long long unset; };
inline constexpr KnobInfo kKnobs[] = {
#define X(NAME, READ, UNSET) {#NAME, READ, UNSET},
  DMPC_KNOBS(X)
#undef X
};

inline bool env_flag(const char *name) { const char *e = getenv(name); return e && e[0] == '1'; }

// a latched flag (one value for the whole library: the static belongs to the one instance of this template)
template <Knob K>
inline bool knob_on() {
  static_assert(kKnobs[(int)K].read == kLatched, "a per-call switch: knob_on_now");
  static const bool on = env_flag(kKnobs[(int)K].name);
  return on;
}

// a per-call flag
template <Knob K>
inline bool knob_on_now() {
  static_assert(kKnobs[(int)K].read == kPerCall, "a latched switch: knob_on");
  return env_flag(kKnobs[(int)K].name);
}

// an integer, in its own read mode
template <Knob K>
inline long long knob_int() {
  const auto read = [] { const char *e = getenv(kKnobs[(int)K].name); return e ? atoll(e) : kKnobs[(int)K].unset; };
  if constexpr (kKnobs[(int)K].read == kLatched) {
    static const long long v = read();
    return v;
  } else {
    return read();
  }
}

}  // namespace dmpc
