// sx_cem_cautious_rollout_sat: the cautious rollout with the saturating cost as its objective
// (cem_cautious_rollout_kernel<..., SAT = true>, sx_cautious.hpp) for every shift-0 shape of SX_ROLLOUT_SHAPES in both
// forms, and its entries (the multi-model kernels are compiled in sx_cautious_sat_multi.hip).  The plan is the parent's (sx_cem_cautious_rollout_form answers for it): the cost's constants are no LDS.  A
// translation unit of its own: nothing the other objects compile changes with it.
#include "sx_cautious_host.hpp"   // CautiousForm, cautious_plan

namespace sx {

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
        return cem_cautious_rollout_kernel<NS, NU, BYOUT, true, false, const int4* __restrict__>;
    }
};

}  // namespace sx

namespace {

// behind check_cautious_entry: the cost, the polytope rows, then the launch for one model (`table` NULL) or E of them
int cautious_sat_launch(const sx_gp_model* models, const void* table, const sx_env* env, const sx_sat_cost* cost, int E,
                        int P, int T, const double* x0, const double* mean, const double* std, const double* noise,
                        double* rows, double* obj_cost, double* con_cost, double* traj, double* sigma, double* cov,
                        double* margins, int propagate, int32_t* status, void* stream) {
    if (!sx::sat_cost_ok(cost, env->n_s)) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const sx::SatEnv se = sx::make_sat_env(env, cost);
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, nullptr, mean, std, noise, rows, obj_cost, con_cost, traj, status, E, P,
                                               T, T, 0);
    const sx::CautiousPtrs cp{pp, sigma, cov, margins, se.env.obj_mode, env->m, propagate != 0};
    return sx::perf_gp_dispatch<sx::CautiousSatForm>(models, table, &se.env, cp, (hipStream_t)stream);
}

}  // namespace

extern "C" int sx_cem_cautious_rollout_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env,
                                                 const sx_sat_cost* cost, int E, int P, int T, const double* x0,
                                                 const double* mean, const double* std, const double* noise, double* rows,
                                                 double* obj_cost, double* con_cost, double* traj, double* sigma,
                                                 double* cov, double* margins, int propagate, int32_t* status,
                                                 void* stream) {
    if (int rc = sx::check_cautious_entry(table && cost, models, E, env, E, P, T, x0, mean, std, noise, rows, obj_cost,
                                          con_cost, status))
        return rc;
    return cautious_sat_launch(models, table, env, cost, E, P, T, x0, mean, std, noise, rows, obj_cost, con_cost, traj,
                               sigma, cov, margins, propagate, status, stream);
}

extern "C" int sx_cem_cautious_rollout_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E,
                                           int P, int T, const double* x0, const double* mean, const double* std,
                                           const double* noise, double* rows, double* obj_cost, double* con_cost,
                                           double* traj, double* sigma, double* cov, double* margins, int propagate,
                                           int32_t* status, void* stream) {
    if (int rc = sx::check_cautious_entry(cost != nullptr, model, 1, env, E, P, T, x0, mean, std, noise, rows, obj_cost,
                                          con_cost, status))
        return rc;
    return cautious_sat_launch(model, nullptr, env, cost, E, P, T, x0, mean, std, noise, rows, obj_cost, con_cost, traj,
                               sigma, cov, margins, propagate, status, stream);
}
