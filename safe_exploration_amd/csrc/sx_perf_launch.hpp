// The form of a variance performance rollout (sx_cem_perf_rollout_var[_multi]), decided here only -- the entries launch
// it, sx_cem_perf_rollout_var[_multi]_form report it -- and the launcher of the multi-model kernels, whose instantiations
// are compiled in sx_perf_multi.hip (sx_perf_taylor_multi.hip for the Taylor form, which plans with the same two
// functions plus the bytes of its step constants).  Host code only.
#pragma once
#include <algorithm>

#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // rollout_compiled, rollout_stream_lds_bytes
#include "sx_perf_var.hpp"

namespace sx {

struct PerfVarPlan {
    int form;     // SX_FORM_STREAM (Kstar of all outputs in LDS) | SX_FORM_BYOUT
    bool ok;      // false: the entry answers SX_ERR_UNSUPPORTED
    size_t lds;   // dynamic LDS bytes
};

// As plan_rollout (sx_gp_rollout.hip) decides the streaming safety kernel's: Kstar of all outputs in LDS where they fit
// beside the n_perf actions of the tile, else output by output (n_s > 1), else unsupported -- there is no resident-W form
// and no workspace path here.  `extra_bytes`: what the kernel keeps in LDS behind the actions (the Taylor form's step
// constants, sx_perf_taylor.hpp).
inline PerfVarPlan plan_perf_var(int ns, int nu, int n_train, int n_pad, int n_perf, size_t extra_bytes = 0) {
    auto lds_bytes = [&](bool byout) {
        return rollout_stream_lds_bytes(ns, nu, 0, n_train, n_pad, n_perf, byout) + extra_bytes;
    };
    const bool compiled = rollout_compiled(ns, nu, 0);
    const bool fits = n_pad <= 1024;
    if (fits && lds_bytes(false) <= kMaxLdsBytes) return {SX_FORM_STREAM, compiled, lds_bytes(false)};
    if (ns > 1 && fits && lds_bytes(true) <= kMaxLdsBytes) return {SX_FORM_BYOUT, compiled, lds_bytes(true)};
    return {SX_FORM_STREAM, false, 0};
}

// One launch for E problems with a GP each, as plan_rollout_multi: output by output for every problem where any model
// needs it, the LDS of the largest model; a model without a form makes the whole launch unsupported.  `extra_bytes` as
// in plan_perf_var.
inline PerfVarPlan plan_perf_var_multi(const sx_gp_model* models, int E, int n_perf, size_t extra_bytes = 0) {
    PerfVarPlan out{SX_FORM_STREAM, true, 0};
    const int ns = models[0].n_s, nu = models[0].n_u;
    for (int i = 0; i < E; ++i) {
        const PerfVarPlan p = plan_perf_var(ns, nu, models[i].n_train, models[i].n_pad, n_perf, extra_bytes);
        if (!p.ok) return {p.form, false, 0};
        if (p.form == SX_FORM_BYOUT) out.form = SX_FORM_BYOUT;
    }
    for (int i = 0; i < E; ++i)
        out.lds = std::max(out.lds, rollout_stream_lds_bytes(ns, nu, 0, models[i].n_train, models[i].n_pad, n_perf,
                                                             out.form == SX_FORM_BYOUT) +
                                        extra_bytes);
    return out;
}

// bytes of the step constants (PerfTaylorConst, sx_perf_taylor.hpp) the Taylor kernels keep in LDS behind the tile's actions
inline size_t perf_taylor_extra_bytes(int ns, int nu) {
    return ((size_t)2 * ns * ns + 2 * ns * nu + 2 * nu + 3 * ns + (size_t)SX_MAX_M * ns + SX_MAX_M) * sizeof(double);
}

// The Taylor form of the multi-model launch (sx_cem_perf_rollout_taylor_multi): plan_perf_var_multi with the step constants.
inline PerfVarPlan plan_perf_taylor_multi(const sx_gp_model* models, int E, int n_perf) {
    return plan_perf_var_multi(models, E, n_perf, perf_taylor_extra_bytes(models[0].n_s, models[0].n_u));
}

// The packed model of sx_gp_pack: W fragments, the stage table, and the padding that holds the mean / Jacobian rows
inline bool perf_var_model_ok(const sx_gp_model& m) {
    if (!m.x_train || m.n_train <= 0 || !m.a_pack || !m.stage_tab) return false;
    return m.n_pad % 16 == 0 && m.n_pad > m.n_train + m.n_s + m.n_u;
}

// Launches cem_perf_var_rollout_multi_kernel<NS, NU, byout> over vp.p.E problems (`table`: sx_gp_model_table's) with `lds`
// bytes; vp.p.status holds E words.
template <int NS, int NU>
int launch_perf_var_multi(const GpConst<NS, NS + NU>* table, const PerfStepConst<NS, NU>& sc, const PerfVarPtrs& vp,
                          bool byout, size_t lds, hipStream_t stream);

// Launches cem_perf_taylor_rollout_multi_kernel<NS, NU, byout> (compiled in sx_perf_taylor_multi.hip) likewise;
// tp.v.p.status holds E words.
template <int NS, int NU>
struct PerfTaylorConst;
struct PerfTaylorPtrs;
template <int NS, int NU>
int launch_perf_taylor_multi(const GpConst<NS, NS + NU>* table, const PerfTaylorConst<NS, NU>& tc, const PerfTaylorPtrs& tp,
                             bool byout, size_t lds, hipStream_t stream);

}  // namespace sx
