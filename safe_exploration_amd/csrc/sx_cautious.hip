// sx_cem_cautious_rollout: the chance-constrained Taylor rollout of Cautious MPC (sx_cautious.hpp) for every shift-0 shape
// of SX_ROLLOUT_SHAPES in both of its forms, and its entry points, those of the multi-model launch included (its kernels are
// compiled in sx_cautious_multi.hip).  The host path from plan to launch is the performance
// rollouts' (perf_gp_rollout, sx_perf_launch.hpp) over one more form.  A translation unit of its own: nothing the other
// objects compile changes with it.
#include "sx_cautious_host.hpp"   // CautiousForm, cautious_plan

extern "C" int sx_cem_cautious_rollout_form(const sx_gp_model* model, int T) {
    sx::StreamPlan plan;
    if (!sx::cautious_plan(model, 1, T, plan)) return -1;
    return plan.form;
}

extern "C" int sx_cem_cautious_rollout_multi_form(const sx_gp_model* models, int n, int T) {
    sx::StreamPlan plan;
    if (!sx::cautious_plan(models, n, T, plan)) return -1;
    return plan.form;
}

namespace {

// behind check_cautious_entry: the objective, the polytope rows, then the launch for one model (`table` NULL) or E of them
int cautious_launch(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int T, const double* x0,
                    const double* mean, const double* std, const double* noise, double* rows, double* obj_cost,
                    double* con_cost, double* traj, double* sigma, double* cov, double* margins, int propagate,
                    int32_t* status, void* stream) {
    if (env->obj_mode != SX_OBJ_NEG_VARIANCE && env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, nullptr, mean, std, noise, rows, obj_cost, con_cost, traj, status, E, P,
                                               T, T, 0);
    const sx::CautiousPtrs cp{pp, sigma, cov, margins, env->obj_mode, env->m, propagate != 0};
    return sx::perf_gp_dispatch<sx::CautiousForm>(models, table, env, cp, (hipStream_t)stream);
}

}  // namespace

extern "C" int sx_cem_cautious_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P,
                                             int T, const double* x0, const double* mean, const double* std,
                                             const double* noise, double* rows, double* obj_cost, double* con_cost,
                                             double* traj, double* sigma, double* cov, double* margins, int propagate,
                                             int32_t* status, void* stream) {
    if (int rc = sx::check_cautious_entry(table, models, E, env, E, P, T, x0, mean, std, noise, rows, obj_cost, con_cost,
                                          status))
        return rc;
    return cautious_launch(models, table, env, E, P, T, x0, mean, std, noise, rows, obj_cost, con_cost, traj, sigma, cov,
                           margins, propagate, status, stream);
}

extern "C" int sx_cem_cautious_rollout(const sx_gp_model* model, const sx_env* env, int E, int P, int T, const double* x0,
                                       const double* mean, const double* std, const double* noise, double* rows,
                                       double* obj_cost, double* con_cost, double* traj, double* sigma, double* cov,
                                       double* margins, int propagate, int32_t* status, void* stream) {
    if (int rc = sx::check_cautious_entry(true, model, 1, env, E, P, T, x0, mean, std, noise, rows, obj_cost, con_cost,
                                          status))
        return rc;
    return cautious_launch(model, nullptr, env, E, P, T, x0, mean, std, noise, rows, obj_cost, con_cost, traj, sigma, cov,
                           margins, propagate, status, stream);
}
