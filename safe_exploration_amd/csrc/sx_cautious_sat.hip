// sx_cem_cautious_rollout_sat: the cautious rollout with the saturating cost as its objective
// (cem_cautious_rollout_kernel<..., SAT = true>, sx_cautious.hpp) for every shift-0 shape of SX_ROLLOUT_SHAPES in both
// forms, and its entry.  The plan is the parent's (sx_cem_cautious_rollout_form answers for it): the cost's constants are no LDS.  A
// translation unit of its own: nothing the other objects compile changes with it.
#include "sx_cautious_host.hpp"   // CautiousForm, cautious_plan

namespace sx {

// (there is no multi-model cautious launch, and no caller hands perf_gp_rollout a table)
template <int NS, int NU>
inline int launch_perf_gp_multi(const GpConst<NS, NS + NU>*, const CautiousSatConst<NS, NU>&, const CautiousPtrs&, bool,
                                unsigned, size_t, hipStream_t) {
    return SX_ERR_UNSUPPORTED;
}

struct CautiousSatForm {
    template <int NS, int NU>
    using Const = CautiousSatConst<NS, NU>;
    using Ptrs = CautiousPtrs;
    static const PerfPtrs& base(const Ptrs& cp) { return cp.p; }
    static size_t extra_bytes(int ns, int nu) { return cautious_extra_bytes(ns, nu); }
    template <int NS, int NU>
    static void make_const(const sx_env* env, Const<NS, NU>& c) {
        CautiousForm::make_const<NS, NU>(env, c.cc);
        make_sat_const<NS>(sat_cost_of(env), c.sat);
    }
    template <int NS, int NU, bool BYOUT>
    static auto kernel() {
        return cem_cautious_rollout_kernel<NS, NU, BYOUT, true>;
    }
};

}  // namespace sx

extern "C" int sx_cem_cautious_rollout_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E,
                                           int P, int T, const double* x0, const double* mean, const double* std,
                                           const double* noise, double* rows, double* obj_cost, double* con_cost,
                                           double* traj, double* sigma, double* cov, double* margins, int propagate,
                                           int32_t* status, void* stream) {
    if (!model || !env || !cost || !x0 || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || T < 1) return SX_ERR_ARG;
    if (noise && (!mean || !std)) return SX_ERR_ARG;
    sx::StreamPlan plan;
    if (!sx::cautious_plan(model, T, plan)) return SX_ERR_ARG;
    if (model->n_s != env->n_s || model->n_u != env->n_u) return SX_ERR_ARG;
    if (!sx::sat_cost_ok(cost, env->n_s)) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const sx::SatEnv se = sx::make_sat_env(env, cost);
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, nullptr, mean, std, noise, rows, obj_cost, con_cost, traj, status, E, P,
                                               T, T, 0);
    const sx::CautiousPtrs cp{pp, sigma, cov, margins, se.env.obj_mode, env->m, propagate != 0};
    return sx::perf_gp_dispatch<sx::CautiousSatForm>(model, nullptr, &se.env, cp, (hipStream_t)stream);
}
