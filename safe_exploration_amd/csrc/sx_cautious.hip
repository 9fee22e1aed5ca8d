// sx_cem_cautious_rollout: the chance-constrained Taylor rollout of Cautious MPC (sx_cautious.hpp) for every shift-0 shape
// of SX_ROLLOUT_SHAPES in both of its forms, and its entry points.  The host path from plan to launch is the performance
// rollouts' (perf_gp_rollout, sx_perf_launch.hpp) over one more form.  A translation unit of its own: nothing the other
// objects compile changes with it.
#include "sx_cautious_host.hpp"   // CautiousForm, cautious_plan

extern "C" int sx_cem_cautious_rollout_form(const sx_gp_model* model, int T) {
    sx::StreamPlan plan;
    if (!sx::cautious_plan(model, T, plan)) return -1;
    return plan.form;
}

extern "C" int sx_cem_cautious_rollout(const sx_gp_model* model, const sx_env* env, int E, int P, int T, const double* x0,
                                       const double* mean, const double* std, const double* noise, double* rows,
                                       double* obj_cost, double* con_cost, double* traj, double* sigma, double* cov,
                                       double* margins, int propagate, int32_t* status, void* stream) {
    if (!model || !env || !x0 || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || T < 1) return SX_ERR_ARG;
    if (noise && (!mean || !std)) return SX_ERR_ARG;
    sx::StreamPlan plan;
    if (!sx::cautious_plan(model, T, plan)) return SX_ERR_ARG;
    if (model->n_s != env->n_s || model->n_u != env->n_u) return SX_ERR_ARG;
    if (env->obj_mode != SX_OBJ_NEG_VARIANCE && env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, nullptr, mean, std, noise, rows, obj_cost, con_cost, traj, status, E, P,
                                               T, T, 0);
    const sx::CautiousPtrs cp{pp, sigma, cov, margins, env->obj_mode, env->m, propagate != 0};
    return sx::perf_gp_dispatch<sx::CautiousForm>(model, nullptr, env, cp, (hipStream_t)stream);
}
