// Host side of the cautious rollout, shared by sx_cautious.hip (the parent entry) and sx_cautious_sat.hip (the entry with
// the saturating cost): the form for perf_gp_rollout, the plan and the entry's checks.  Host code only.
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

// (perf_gp_rollout names the multi-model launcher of its form; there is no multi-model cautious launch, and no caller
// hands it a table)
template <int NS, int NU>
inline int launch_perf_gp_multi(const GpConst<NS, NS + NU>*, const CautiousConst<NS, NU>&, const CautiousPtrs&, bool, unsigned,
                         size_t, hipStream_t) {
    return SX_ERR_UNSUPPORTED;
}

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
        return cem_cautious_rollout_kernel<NS, NU, BYOUT, false>;
    }
};

// The plan of a model over T steps (the streaming plan over the cautious constants), where the entry would take the model
inline bool cautious_plan(const sx_gp_model* model, int T, StreamPlan& plan) {
    if (!model || T < 1 || !perf_shape_ok(*model) || !perf_models_ok(model, 1, perf_var_model_ok)) return false;
    plan = plan_stream_multi(model, 1, T, cautious_extra_bytes(model->n_s, model->n_u));
    return true;
}

}  // namespace sx
