// The compiled shapes of the fused rollout, the streaming plan every exact-GP rollout shares (plan_stream,
// plan_stream_multi: the LDS rule and its fold over several models, written here only), and the launcher of the streaming
// rollout kernel (launch_stream<V, NS, NU> over a variant V of it).  The launcher's instantiations are
// compiled in translation units of their own, beside the kernels (sx_stream_ns12.hip, sx_stream_ns34.hip; the multi-model
// mode in sx_stream_multi.hip, the per-particle starts in sx_stream_starts.hip, the saturating-cost objective in
// sx_stream_sat.hip and sx_stream_sat_multi.hip, the constraint set in sx_stream_cons.hip and sx_stream_cons_sat.hip, in the
// multi-model mode in sx_stream_cons_multi.hip and sx_stream_cons_sat_multi.hip, on the per-particle starts in
// sx_stream_starts_cons.hip, the per-particle starts in the multi-model mode in sx_stream_starts_multi.hip and
// sx_stream_starts_cons_multi.hip, a gain per particle and step in sx_stream_gains.hip; built in parallel with the rest);
// sx_gp_rollout.hip sees the declaration.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_launch.hpp"   // kMaxLdsBytes
#include "sx_reach.hpp"
#include "sx_rollout.hpp"

// (n_s, n_u, query shift) of every compiled fused rollout: X(NS, NU, SH, ...).  Shift 0 is sx_cem_rollout (and the shape
// set of every other exact-GP entry point), shift > 0 sx_cem_rollout_junk (n_s + n_u + shift <= SX_MAX_D).  Each entry
// has an instantiation of launch_stream<StreamPlain<SH>> in sx_stream_ns*.hip; ssm_cem.JUNK_FUSED_SHAPES is checked against it.
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

// The streaming plan of one launch: the form, and the dynamic LDS bytes of its kernel
struct StreamPlan {
    int form;     // SX_FORM_STREAM (Kstar of all outputs in LDS) | SX_FORM_BYOUT | -1: no streaming form fits
    size_t lds;
};

// The LDS rule of the streaming kernels, decided here only, for a GP over ns + nu + sh columns, `steps` steps of nu
// actions in the tile and `extra_bytes` behind them (the step constants of the Taylor and cautious kernels; 0 for the
// safety rollouts): Kstar of all outputs in LDS where they fit, else output by output (n_s > 1), else none; n_pad <= 1024
// (the stage tables are cut for that).  Does not ask whether the shape is compiled.
inline StreamPlan plan_stream(int ns, int nu, int sh, int n_train, int n_pad, int steps, size_t extra_bytes = 0) {
    auto lds = [&](bool byout) { return rollout_stream_lds_bytes(ns, nu, sh, n_train, n_pad, steps, byout) + extra_bytes; };
    if (n_pad <= 1024 && lds(false) <= kMaxLdsBytes) return {SX_FORM_STREAM, lds(false)};
    if (n_pad <= 1024 && ns > 1 && lds(true) <= kMaxLdsBytes) return {SX_FORM_BYOUT, lds(true)};
    return {-1, 0};
}

// One launch for E problems with a GP each (E = 1: the entries that have the streaming kernel only), shift 0: output by
// output for every problem where any model needs it, the LDS of the largest model in that form; a model without a
// streaming form, or a shape that is not compiled, leaves the whole launch without one.
inline StreamPlan plan_stream_multi(const sx_gp_model* models, int E, int steps, size_t extra_bytes = 0) {
    const int ns = models[0].n_s, nu = models[0].n_u;
    if (!rollout_compiled(ns, nu, 0)) return {-1, 0};
    StreamPlan out{SX_FORM_STREAM, 0};
    for (int i = 0; i < E; ++i) {
        const StreamPlan p = plan_stream(ns, nu, 0, models[i].n_train, models[i].n_pad, steps, extra_bytes);
        if (p.form < 0) return p;
        if (p.form == SX_FORM_BYOUT) out.form = SX_FORM_BYOUT;
    }
    for (int i = 0; i < E; ++i)
        out.lds = std::max(out.lds, rollout_stream_lds_bytes(ns, nu, 0, models[i].n_train, models[i].n_pad, steps,
                                                             out.form == SX_FORM_BYOUT) + extra_bytes);
    return out;
}

// The variant of the streaming kernel a launch names: cem_rollout_kernel<V, NS, NU, BYOUT, X...> (sx_rollout.hpp) reads
// these flags, and launch_stream forms X... from them.  The step loop, the forms, the barriers and the LDS plan are the same
// in every variant.
//   SH    the query shift (sx_cem_rollout_junk; described at RolloutGpArg).
//   MM    the first argument is the device table of the problems' GpConst (sx_gp_model_table; at RolloutGpArg too).
//   PS    (sx_cem_rollout_starts[_multi]; SH = 0) a start state per particle: the CEM row of a particle is
//         [x0 (NS) | actions (H NU)], L = NS + H NU entries.  rp.mean / rp.std are [E x L], rp.noise [E x P x L] | NULL,
//         rp.actions the rows [E x P x L] (written when noise is given, read otherwise); rp.x0, rp.q0 and the elite-row
//         fields are unused.  The owner lane of a particle takes its start from its own row (a point, reach_point at t = 0)
//         and pays SX_STATE_VIOLATION_COST once where that start is outside the polytope; a lane past P in the last tile
//         reads through the problem's first particle and writes nothing.
//   SAT   (SH = 0, PS = false) the objective of a step is the saturating cost of sx_sat_cost.hpp on the safety ellipsoid
//         (p_{t+1}, Q_{t+1}), read as a mean and a covariance, from a trailing SatConst<NS> argument; cc.obj_mode is not
//         read.  Nothing else in the step changes.
//   CONS  (SH = 0) the constraint set of sx_conset.hpp, from a trailing ConConst<NS> argument ahead of SAT's: ONE set, shared
//         by all problems with MM.  A step that starts from an ellipsoid pays its action cost where the control ellipsoid
//         (u_t, K Q_t K^T) is not certified inside the action box either (once per step, with the box test), and every step
//         but the last pays SX_STATE_VIOLATION_COST where (p_{t+1}, Q_{t+1}) is not certified inside the obstacle rows.  The
//         objective is SAT's, either one; with an empty set the step is the variant's without CONS (section 3.15).
//         With PS (the static rollout; the reference's static-exploration NLP has the gain fixed, so the set is its
//         constraints term for term): a particle starts from a point, so step 0 pays the box test only, and the prologue
//         tests the start x0 itself against the obstacle rows, SX_STATE_VIOLATION_COST once, beside and independent of the
//         safe-polytope cost of the start (section 3.10, "the constraint set").
//   KF    (sx_cem_rollout_gains; with PS, SH = 0, one model, no SAT, no CONS) a feedback gain per particle and step, from a
//         trailing GainConst argument: dev [E x P x (H - 1) x NU x NS].  At step t >= 1 the owner lane of a particle reads
//         its K_t, forms the lower Cholesky factor of I + K_t^T K_t in registers (gain_chol) and runs reach_ellipsoid on a
//         lane-local copy of rc with these two; rc.kfb / rc.cholB are not read.  Step 0 starts from the point of the row
//         and reads no gain.  Everything else in the step is StreamStarts' (DESIGN.md section 3.16).
template <int SH_, bool MM_, bool PS_, bool SAT_, bool CONS_, bool KF_ = false>
struct StreamVariant {
    static constexpr int SH = SH_;
    static constexpr bool MM = MM_, PS = PS_, SAT = SAT_, CONS = CONS_, KF = KF_;
};
template <int SH, bool MM = false>
using StreamPlain = StreamVariant<SH, MM, false, false, false>;   // sx_cem_rollout[_elites][_junk] (MM: ..._multi)
using StreamStarts = StreamVariant<0, false, true, false, false>;   // sx_cem_rollout_starts
template <bool MM>
using StreamSat = StreamVariant<0, MM, false, true, false>;   // sx_cem_rollout[_elites]_sat (MM: ..._sat_multi)
template <bool SAT, bool MM = false>
using StreamCons = StreamVariant<0, MM, false, SAT, true>;   // sx_cem_rollout[_elites]_cons[_multi], SAT: with a cost
using StreamStartsCons = StreamVariant<0, false, true, false, true>;   // sx_cem_rollout_starts_cons
using StreamStartsMulti = StreamVariant<0, true, true, false, false>;   // sx_cem_rollout_starts_multi
using StreamStartsConsMulti = StreamVariant<0, true, true, false, true>;   // sx_cem_rollout_starts_cons_multi
using StreamGains = StreamVariant<0, false, true, false, false, true>;   // sx_cem_rollout_gains

// The first kernel argument of variant V: the GpConst, or with V::MM the device table of E of them
template <class V, int NS, int NU>
using StreamGpArg = typename RolloutGpArg<NS, NS + NU + V::SH, V::MM>::type;

// Launches cem_rollout_kernel<V, NS, NU, byout, ...> on `stream` over rp.E * ceil(rp.P / SX_TILE) workgroups with `lds`
// bytes of dynamic LDS (plan_stream's; with V::MM plan_stream_multi's, and rp.status holds a word per problem).  `sat` is read with V::SAT
// only, `cons` with V::CONS only and `gains` with V::KF only (NULL otherwise).  SX_ERR_UNSUPPORTED for a grid past INT_MAX.
template <class V, int NS, int NU>
int launch_stream(const StreamGpArg<V, NS, NU>& gp, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                  const RolloutPtrs& rp, const SatConst<NS>* sat, bool byout, size_t lds, hipStream_t stream,
                  const ConConst<NS>* cons = nullptr, const GainConst* gains = nullptr);

}  // namespace sx
