// Host side of the cautious rollout, shared by sx_cautious.hip (the parent entries), sx_cautious_sat.hip (the entries with
// the saturating cost) and the translation units of their multi-model kernels (sx_cautious_multi.hip,
// sx_cautious_sat_multi.hip): the form for perf_gp_rollout, the plan, the entries' checks and the multi-model launch.
// Host code only.
#pragma once
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf_launch.hpp"
#include "sx_perf_taylor_host.hpp"   // PerfTaylorForm::make_const
#include "sx_cautious.hpp"

namespace sx {

// bytes of the step constants (CautiousConst) behind the tile's actions: the Taylor form's plus beta
inline size_t cautious_extra_bytes(int ns, int nu) { return perf_taylor_extra_bytes(ns, nu) + sizeof(double); }

// One launch of the multi-model cautious kernel over `table` (sx_gp_model_table's; the status holds a word per problem); one
// output has no output-by-output kernel.
template <bool SAT, int NS, int NU, class... Args>
int launch_cautious_forms(bool byout, unsigned blocks, size_t lds, hipStream_t stream, const Args&... args) {
    if constexpr (NS > 1) {
        if (byout)
            return launch_perf_gp(cem_cautious_rollout_kernel<NS, NU, true, SAT, true>, blocks, lds, stream, args...);
    }
    return launch_perf_gp(cem_cautious_rollout_kernel<NS, NU, false, SAT, true>, blocks, lds, stream, args...);
}

// The multi-model launchers perf_gp_rollout names for the two cautious forms, instantiated for every shape beside their
// kernels (sx_cautious_multi.hip, sx_cautious_sat_multi.hip)
template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const CautiousConst<NS, NU>& cc, const CautiousPtrs& cp,
                         bool byout, unsigned blocks, size_t lds, hipStream_t stream);
template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const CautiousSatConst<NS, NU>& c, const CautiousPtrs& cp,
                         bool byout, unsigned blocks, size_t lds, hipStream_t stream);

// The cautious form for perf_gp_rollout: the Taylor form's plan (T steps of actions, the step constants behind them)
struct CautiousForm {
    template <int NS, int NU>
    using Const = CautiousConst<NS, NU>;
    using Ptrs = CautiousPtrs;
    static const PerfPtrs& base(const Ptrs& cp) { return cp.p; }
    static size_t extra_bytes(int ns, int nu) { return cautious_extra_bytes(ns, nu); }
    template <int NS, int NU>
    static void make_const(const sx_env* env, Const<NS, NU>& cc) {
        static_assert(sizeof(CautiousConst<NS, NU>) == sizeof(PerfTaylorConst<NS, NU>) + sizeof(double),
                      "cautious_extra_bytes counts the fields of CautiousConst");
        PerfTaylorForm::make_const<NS, NU>(env, cc.tc);
        cc.beta = env->beta;
    }
    template <int NS, int NU, bool BYOUT>
    static auto kernel() {
        return cem_cautious_rollout_kernel<NS, NU, BYOUT, false, false, const int4* __restrict__>;
    }
};

// The plan of `n` models of one (n_s, n_u) over T steps (the streaming plan over the cautious constants: output by output
// as soon as one model needs it, the LDS of the largest), where the entries would take the models
inline bool cautious_plan(const sx_gp_model* models, int n, int T, StreamPlan& plan) {
    if (!models || n < 1 || T < 1 || !perf_shape_ok(*models) || !perf_models_ok(models, n, perf_var_model_ok)) return false;
    plan = plan_stream_multi(models, n, T, cautious_extra_bytes(models->n_s, models->n_u));
    return true;
}

// What the four cautious entries check alike before anything touches the device, in the order they answer (`head`: the
// entry's own leading pointers are all there), for one model or the E of a multi-model launch
inline int check_cautious_entry(bool head, const sx_gp_model* models, int n, const sx_env* env, int E, int P, int T,
                                const double* x0, const double* mean, const double* std, const double* noise,
                                const double* rows, const double* obj_cost, const double* con_cost, const int32_t* status) {
    if (!head || !models || !env || !x0 || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || T < 1) return SX_ERR_ARG;
    if (noise && (!mean || !std)) return SX_ERR_ARG;
    StreamPlan plan;
    if (!cautious_plan(models, n, T, plan)) return SX_ERR_ARG;
    if (models->n_s != env->n_s || models->n_u != env->n_u) return SX_ERR_ARG;
    return SX_OK;
}

}  // namespace sx
