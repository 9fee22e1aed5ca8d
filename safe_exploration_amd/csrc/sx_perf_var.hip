// sx_cem_perf_rollout_var: the performance-trajectory kernel with the posterior variance (sx_perf_var.hpp) for every
// shift-0 shape of SX_ROLLOUT_SHAPES in both of its forms, its launcher and the entry point.  A translation unit of its
// own: nothing the other objects compile changes with it.
#include <climits>
#include <cstring>

#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH, rollout_stream_lds_bytes
#include "sx_perf_launch.hpp"
#include "sx_perf_var.hpp"

namespace sx {

static_assert(kPerfVarThreads == kRolloutThreads, "the stage table of sx_gp_pack is cut for the safety kernel's waves");

template <int NS, int NU, bool BYOUT>
static int launch_perf_var(const GpConst<NS, NS + NU>& gc, const PerfStepConst<NS, NU>& sc, const PerfVarPtrs& vp,
                           unsigned blocks, size_t lds, hipStream_t stream) {
    if (int r = allow_lds(cem_perf_var_rollout_kernel<NS, NU, BYOUT>, lds)) return r;
    hipLaunchKernelGGL((cem_perf_var_rollout_kernel<NS, NU, BYOUT>), dim3(blocks), dim3(kPerfVarThreads), lds, stream, gc,
                       gc.stage_tab, sc, vp);
    return check_launch();
}

// The launch in the form plan_perf_var (sx_perf_launch.hpp) picks.
template <int NS, int NU>
static int perf_var_rollout(const sx_gp_model* m, const sx_env* env, const PerfVarPtrs& vp, hipStream_t stream) {
    const PerfPtrs& pp = vp.p;
    const PerfVarPlan plan = plan_perf_var(NS, NU, m->n_train, m->n_pad, pp.n_perf);
    const int64_t blocks = (int64_t)pp.E * ((pp.P + SX_TILE - 1) / SX_TILE);
    if (!plan.ok || blocks > INT_MAX) return SX_ERR_UNSUPPORTED;
    PerfStepConst<NS, NU> sc;
    std::memset(&sc, 0, sizeof(sc));
    make_perf_step<NS, NU>(env, sc);
    const GpConst<NS, NS + NU> gc = make_gp_const<NS, NU>(m, kPerfVarThreads / 64);
    return plan.form == SX_FORM_BYOUT ? launch_perf_var<NS, NU, true>(gc, sc, vp, (unsigned)blocks, plan.lds, stream)
                                      : launch_perf_var<NS, NU, false>(gc, sc, vp, (unsigned)blocks, plan.lds, stream);
}

static int perf_var_dispatch(const sx_gp_model* m, const sx_env* env, const PerfVarPtrs& vp, hipStream_t stream) {
#define CALL(NS, NU) perf_var_rollout<NS, NU>(m, env, vp, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

template <int NS, int NU>
static int perf_var_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env, const PerfVarPtrs& vp,
                                  hipStream_t stream) {
    const PerfVarPlan plan = plan_perf_var_multi(models, vp.p.E, vp.p.n_perf);
    if (!plan.ok) return SX_ERR_UNSUPPORTED;
    PerfStepConst<NS, NU> sc;
    std::memset(&sc, 0, sizeof(sc));
    make_perf_step<NS, NU>(env, sc);
    return launch_perf_var_multi<NS, NU>(static_cast<const GpConst<NS, NS + NU>*>(table), sc, vp,
                                         plan.form == SX_FORM_BYOUT, plan.lds, stream);
}

static int perf_var_multi_dispatch(const sx_gp_model* models, const void* table, const sx_env* env, const PerfVarPtrs& vp,
                                   hipStream_t stream) {
#define CALL(NS, NU) perf_var_rollout_multi<NS, NU>(models, table, env, vp, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

// E packed models of one (n_s, n_u): checked before anything touches the device
static bool perf_var_models_ok(const sx_gp_model* models, int E) {
    if (!models || E <= 0) return false;
    const int ns = models[0].n_s, nu = models[0].n_u;
    if (ns <= 0 || ns > SX_MAX_NS || nu <= 0 || nu > SX_MAX_NU) return false;
    for (int i = 0; i < E; ++i)
        if (models[i].n_s != ns || models[i].n_u != nu || !perf_var_model_ok(models[i])) return false;
    return true;
}

}  // namespace sx

extern "C" int sx_cem_perf_rollout_var_form(const sx_gp_model* model, int n_perf) {
    if (!model || n_perf <= 1 || model->n_s <= 0 || model->n_u <= 0 || !sx::perf_var_model_ok(*model)) return -1;
    const sx::PerfVarPlan plan = sx::plan_perf_var(model->n_s, model->n_u, model->n_train, model->n_pad, n_perf);
    return plan.ok ? plan.form : -1;
}

extern "C" int sx_cem_perf_rollout_var_multi_form(const sx_gp_model* models, int E, int n_perf) {
    if (n_perf <= 1 || !sx::perf_var_models_ok(models, E)) return -1;
    const sx::PerfVarPlan plan = sx::plan_perf_var_multi(models, E, n_perf);
    return plan.ok ? plan.form : -1;
}

extern "C" int sx_cem_perf_rollout_var_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P,
                                             int H, int n_perf, int r, const double* x0, const double* safe_actions,
                                             const double* tail_mean, const double* tail_std, const double* tail_noise,
                                             double* rows, double* obj_cost, double* con_cost, double* perf_traj,
                                             double* perf_sigma, int32_t* status, void* stream) {
    if (!models || !table || !env || !x0 || !safe_actions || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || H <= 0 || r < 1 || r > H || n_perf <= r) return SX_ERR_ARG;
    if (tail_noise && (!tail_mean || !tail_std)) return SX_ERR_ARG;
    if (!sx::perf_var_models_ok(models, E) || models[0].n_s != env->n_s || models[0].n_u != env->n_u) return SX_ERR_ARG;
    if (env->obj_mode != SX_OBJ_NEG_VARIANCE && env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    const sx::PerfVarPtrs vp{{x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj, status,
                              E, P, H, n_perf, r},
                             perf_sigma, env->obj_mode};
    return sx::perf_var_multi_dispatch(models, table, env, vp, (hipStream_t)stream);
}

extern "C" int sx_cem_perf_rollout_var(const sx_gp_model* model, const sx_env* env, int E, int P, int H, int n_perf, int r,
                                       const double* x0, const double* safe_actions, const double* tail_mean,
                                       const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                                       double* con_cost, double* perf_traj, double* perf_sigma, int32_t* status,
                                       void* stream) {
    if (!model || !env || !x0 || !safe_actions || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || H <= 0 || r < 1 || r > H || n_perf <= r) return SX_ERR_ARG;
    if (tail_noise && (!tail_mean || !tail_std)) return SX_ERR_ARG;
    if (!model->x_train || model->n_train <= 0 || model->n_s != env->n_s || model->n_u != env->n_u) return SX_ERR_ARG;
    if (!sx::perf_var_model_ok(*model)) return SX_ERR_ARG;
    if (env->obj_mode != SX_OBJ_NEG_VARIANCE && env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    const sx::PerfVarPtrs vp{{x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj, status,
                              E, P, H, n_perf, r},
                             perf_sigma, env->obj_mode};
    return sx::perf_var_dispatch(model, env, vp, (hipStream_t)stream);
}
