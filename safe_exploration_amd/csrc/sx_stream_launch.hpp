// The compiled shapes of the fused rollout, and the launchers of the streaming rollout kernel (cem_rollout_kernel<NS, NU,
// BYOUT, SH, MM>).  The launchers' instantiations are compiled in translation units of their own (sx_stream_ns12.hip,
// sx_stream_ns34.hip; the multi-model mode in sx_stream_multi.hip, the per-particle starts in sx_stream_starts.hip, the
// saturating-cost objective in sx_stream_sat.hip and sx_stream_sat_multi.hip; built in parallel with the rest);
// sx_gp_rollout.hip sees the declarations.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_reach.hpp"
#include "sx_rollout.hpp"

// (n_s, n_u, query shift) of every compiled fused rollout: X(NS, NU, SH, ...).  Shift 0 is sx_cem_rollout (and the shape
// set of every other exact-GP entry point), shift > 0 sx_cem_rollout_junk (n_s + n_u + shift <= SX_MAX_D).  Each entry
// has an instantiation of launch_rollout_stream in sx_stream_ns*.hip; ssm_cem.JUNK_FUSED_SHAPES is checked against it.
#define SX_ROLLOUT_SHAPES(X, ...)                                                                                       \
    X(2, 1, 0, __VA_ARGS__) X(4, 1, 0, __VA_ARGS__) X(2, 2, 0, __VA_ARGS__) X(4, 2, 0, __VA_ARGS__)                     \
    X(3, 1, 0, __VA_ARGS__) X(1, 1, 0, __VA_ARGS__) X(2, 1, 1, __VA_ARGS__) X(4, 1, 1, __VA_ARGS__)                     \
    X(3, 1, 1, __VA_ARGS__) X(2, 2, 1, __VA_ARGS__) X(2, 2, 2, __VA_ARGS__) X(3, 2, 1, __VA_ARGS__)                     \
    X(1, 1, 1, __VA_ARGS__)

// return CALL(NS, NU) for the shift-0 shape (ns, nu), SX_ERR_UNSUPPORTED for any other
#define SX_SHIFT0_0(...) __VA_ARGS__
#define SX_SHIFT0_1(...)
#define SX_SHIFT0_2(...)
#define SX_DISPATCH_ONE(NS, NU, SH, ns, nu, CALL) SX_SHIFT0_##SH(if ((ns) == NS && (nu) == NU) return CALL(NS, NU);)
#define SX_DISPATCH(ns, nu, CALL)                               \
    do {                                                        \
        SX_ROLLOUT_SHAPES(SX_DISPATCH_ONE, ns, nu, CALL)        \
        return SX_ERR_UNSUPPORTED;                              \
    } while (0)

// return CALL(NS, NU, SH) for the shape (ns, nu, sh), SX_ERR_UNSUPPORTED for any other
#define SX_ROLLOUT_DISPATCH_ONE(NS, NU, SH, ns, nu, sh, CALL) \
    if ((ns) == NS && (nu) == NU && (sh) == SH) return CALL(NS, NU, SH);
#define SX_ROLLOUT_DISPATCH(ns, nu, sh, CALL)                               \
    do {                                                                    \
        SX_ROLLOUT_SHAPES(SX_ROLLOUT_DISPATCH_ONE, ns, nu, sh, CALL)        \
        return SX_ERR_UNSUPPORTED;                                          \
    } while (0)

namespace sx {

// is (ns, nu, sh) one of SX_ROLLOUT_SHAPES?
inline bool rollout_compiled(int ns, int nu, int sh) {
#define SX_COMPILED(NS, NU, SH, unused) if (ns == NS && nu == NU && sh == SH) return true;
    SX_ROLLOUT_SHAPES(SX_COMPILED, 0)
#undef SX_COMPILED
    return false;
}

// Dynamic LDS bytes of cem_rollout_kernel: Kstar of all outputs (byout = false) or of one output at a time, for the GP
// over ns + nu + sh columns and H steps of nu actions.
inline size_t rollout_stream_lds_bytes(int ns, int nu, int sh, int n_train, int n_pad, int H, bool byout) {
    return (gp_tile_lds_doubles(ns, ns + nu + sh, n_train, n_pad, kRolloutThreads / 64, byout ? 1 : ns) +
            (size_t)SX_TILE * H * nu) * sizeof(double);
}

// Launches cem_rollout_kernel<NS, NU, byout, SH> with `lds` bytes (rollout_stream_lds_bytes) of dynamic LDS on `stream`.
template <int NS, int NU, int SH>
int launch_rollout_stream(const GpConst<NS, NS + NU + SH>& gc, const ReachConst<NS, NU>& rc,
                          const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool byout, size_t lds,
                          hipStream_t stream);

// Launches cem_rollout_kernel<NS, NU, byout, 0, true> over E problems with a GP each: `table` is the device array of their
// GpConst (sx_gp_model_table), `lds` the largest rollout_stream_lds_bytes over them.  rp.status holds E words.
template <int NS, int NU>
int launch_rollout_stream_multi(const GpConst<NS, NS + NU>* table, const ReachConst<NS, NU>& rc,
                                const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool byout, size_t lds,
                                hipStream_t stream);

// Launches cem_rollout_starts_kernel<NS, NU, byout> (sx_cem_rollout_starts: a start state per particle, rp as the
// SX_ROLLOUT_PS sections of sx_rollout_body.inc read it) with `lds` bytes (rollout_stream_lds_bytes, shift 0).
// Instantiated for every shift-0 shape in sx_stream_starts.hip.
template <int NS, int NU>
int launch_rollout_starts(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc,
                          const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool byout, size_t lds,
                          hipStream_t stream);

// Launches cem_rollout_sat_kernel<NS, NU, byout, false> (sx_cem_rollout[_elites]_sat: the saturating cost `sat` on the
// safety ellipsoids as the objective) with `lds` bytes (rollout_stream_lds_bytes, shift 0: the parent's plan).
// Instantiated for every shift-0 shape in sx_stream_sat.hip.
template <int NS, int NU>
int launch_rollout_sat(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                       const RolloutPtrs& rp, const SatConst<NS>& sat, bool byout, size_t lds, hipStream_t stream);

// Launches cem_rollout_sat_kernel<NS, NU, byout, true> over E problems with a GP each (sx_cem_rollout[_elites]_sat_multi;
// `table`, `lds` and rp.status as launch_rollout_stream_multi).  Instantiated in sx_stream_sat_multi.hip.
template <int NS, int NU>
int launch_rollout_sat_multi(const GpConst<NS, NS + NU>* table, const ReachConst<NS, NU>& rc,
                             const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, const SatConst<NS>& sat,
                             bool byout, size_t lds, hipStream_t stream);

}  // namespace sx
