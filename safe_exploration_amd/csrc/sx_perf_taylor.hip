// sx_cem_perf_rollout_taylor: the performance-trajectory kernel with Taylor uncertainty propagation (sx_perf_taylor.hpp)
// for every shift-0 shape of SX_ROLLOUT_SHAPES in both of its forms, its launcher and the entry points, those of the
// multi-model launch included (its kernels are compiled in sx_perf_taylor_multi.hip).  A translation unit of its own:
// nothing the other objects compile changes with it.
#include <climits>
#include <cstring>

#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf_launch.hpp"     // plan_perf_var, perf_var_model_ok
#include "sx_perf_taylor.hpp"

namespace sx {

static_assert(kPerfVarThreads == kRolloutThreads, "the stage table of sx_gp_pack is cut for the safety kernel's waves");

static PerfVarPlan plan_perf_taylor(const sx_gp_model* m, int n_perf) {
    return plan_perf_var(m->n_s, m->n_u, m->n_train, m->n_pad, n_perf, perf_taylor_extra_bytes(m->n_s, m->n_u));
}

template <int NS, int NU>
static void make_perf_taylor_const(const sx_env* env, PerfTaylorConst<NS, NU>& tc) {
    std::memset(&tc, 0, sizeof(tc));
    make_perf_step<NS, NU>(env, tc.step);
    for (int i = 0; i < NS; ++i)
        for (int j = 0; j < NS; ++j) {
            double s = env->a[i * NS + j];
            for (int c = 0; c < NU; ++c) s += env->b[i * NU + c] * env->k_fb[c * NS + j];
            tc.abk[i * NS + j] = s;
        }
    for (int i = 0; i < NU * NS; ++i) tc.k_fb[i] = env->k_fb[i];
    for (int i = 0; i < env->m * NS; ++i) tc.h_mat[i] = env->h_mat[i];
    for (int i = 0; i < env->m; ++i) tc.h_vec[i] = env->h_vec[i];
}

template <int NS, int NU, bool BYOUT>
static int launch_perf_taylor(const GpConst<NS, NS + NU>& gc, const PerfTaylorConst<NS, NU>& tc, const PerfTaylorPtrs& tp,
                              unsigned blocks, size_t lds, hipStream_t stream) {
    if (int r = allow_lds(cem_perf_taylor_rollout_kernel<NS, NU, BYOUT>, lds)) return r;
    hipLaunchKernelGGL((cem_perf_taylor_rollout_kernel<NS, NU, BYOUT>), dim3(blocks), dim3(kPerfVarThreads), lds, stream,
                       gc, gc.stage_tab, tc, tp);
    return check_launch();
}

// The launch in the form plan_perf_var (sx_perf_launch.hpp) picks for the variance kernel's LDS plus the step constants.
template <int NS, int NU>
static int perf_taylor_rollout(const sx_gp_model* m, const sx_env* env, const PerfTaylorPtrs& tp, hipStream_t stream) {
    static_assert(sizeof(PerfTaylorConst<NS, NU>) ==
                      (2 * NS * NS + 2 * NS * NU + 2 * NU + 3 * NS + SX_MAX_M * NS + SX_MAX_M) * sizeof(double),
                  "perf_taylor_extra_bytes counts the fields of PerfTaylorConst");
    const PerfPtrs& pp = tp.v.p;
    const PerfVarPlan plan = plan_perf_taylor(m, pp.n_perf);
    const int64_t blocks = (int64_t)pp.E * ((pp.P + SX_TILE - 1) / SX_TILE);
    if (!plan.ok || blocks > INT_MAX) return SX_ERR_UNSUPPORTED;
    PerfTaylorConst<NS, NU> tc;
    make_perf_taylor_const<NS, NU>(env, tc);
    const GpConst<NS, NS + NU> gc = make_gp_const<NS, NU>(m, kPerfVarThreads / 64);
    return plan.form == SX_FORM_BYOUT ? launch_perf_taylor<NS, NU, true>(gc, tc, tp, (unsigned)blocks, plan.lds, stream)
                                      : launch_perf_taylor<NS, NU, false>(gc, tc, tp, (unsigned)blocks, plan.lds, stream);
}

static int perf_taylor_dispatch(const sx_gp_model* m, const sx_env* env, const PerfTaylorPtrs& tp, hipStream_t stream) {
#define CALL(NS, NU) perf_taylor_rollout<NS, NU>(m, env, tp, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

// One launch over tp.v.p.E problems with a GP each, in the form plan_perf_taylor_multi picks for all of them.
template <int NS, int NU>
static int perf_taylor_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env,
                                     const PerfTaylorPtrs& tp, hipStream_t stream) {
    const PerfVarPlan plan = plan_perf_taylor_multi(models, tp.v.p.E, tp.v.p.n_perf);
    if (!plan.ok) return SX_ERR_UNSUPPORTED;
    PerfTaylorConst<NS, NU> tc;
    make_perf_taylor_const<NS, NU>(env, tc);
    return launch_perf_taylor_multi<NS, NU>(static_cast<const GpConst<NS, NS + NU>*>(table), tc, tp,
                                            plan.form == SX_FORM_BYOUT, plan.lds, stream);
}

static int perf_taylor_multi_dispatch(const sx_gp_model* models, const void* table, const sx_env* env,
                                      const PerfTaylorPtrs& tp, hipStream_t stream) {
#define CALL(NS, NU) perf_taylor_rollout_multi<NS, NU>(models, table, env, tp, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

static bool perf_taylor_shape_ok(const sx_gp_model* model) {
    return model->n_s > 0 && model->n_s <= SX_MAX_NS && model->n_u > 0 && model->n_u <= SX_MAX_NU;
}

// E packed models of one (n_s, n_u): checked before anything touches the device
static bool perf_taylor_models_ok(const sx_gp_model* models, int E) {
    if (!models || E <= 0 || !perf_taylor_shape_ok(models)) return false;
    for (int i = 0; i < E; ++i)
        if (models[i].n_s != models[0].n_s || models[i].n_u != models[0].n_u || !perf_var_model_ok(models[i])) return false;
    return true;
}

}  // namespace sx

extern "C" int sx_cem_perf_rollout_taylor_form(const sx_gp_model* model, int n_perf) {
    if (!model || n_perf <= 1 || !sx::perf_taylor_shape_ok(model) || !sx::perf_var_model_ok(*model)) return -1;
    const sx::PerfVarPlan plan = sx::plan_perf_taylor(model, n_perf);
    return plan.ok ? plan.form : -1;
}

extern "C" int sx_cem_perf_rollout_taylor_multi_form(const sx_gp_model* models, int E, int n_perf) {
    if (n_perf <= 1 || !sx::perf_taylor_models_ok(models, E)) return -1;
    const sx::PerfVarPlan plan = sx::plan_perf_taylor_multi(models, E, n_perf);
    return plan.ok ? plan.form : -1;
}

extern "C" int sx_cem_perf_rollout_taylor_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E,
                                                int P, int H, int n_perf, int r, const double* x0,
                                                const double* safe_actions, const double* tail_mean,
                                                const double* tail_std, const double* tail_noise, double* rows,
                                                double* obj_cost, double* con_cost, double* perf_traj, double* perf_sigma,
                                                double* perf_cov, int terminal_safety, int32_t* status, void* stream) {
    if (!models || !table || !env || !x0 || !safe_actions || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || H <= 0 || r < 1 || r > H || n_perf <= r) return SX_ERR_ARG;
    if (tail_noise && (!tail_mean || !tail_std)) return SX_ERR_ARG;
    if (!sx::perf_taylor_models_ok(models, E) || models[0].n_s != env->n_s || models[0].n_u != env->n_u)
        return SX_ERR_ARG;
    if (env->obj_mode != SX_OBJ_NEG_VARIANCE && env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    if (terminal_safety && (n_perf < H + 2 || env->m <= 0)) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const sx::PerfTaylorPtrs tp{{{x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj,
                                  status, E, P, H, n_perf, r},
                                 perf_sigma, env->obj_mode},
                                perf_cov, env->m, terminal_safety ? H + 1 : -1};
    return sx::perf_taylor_multi_dispatch(models, table, env, tp, (hipStream_t)stream);
}

extern "C" int sx_cem_perf_rollout_taylor(const sx_gp_model* model, const sx_env* env, int E, int P, int H, int n_perf,
                                          int r, const double* x0, const double* safe_actions, const double* tail_mean,
                                          const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                                          double* con_cost, double* perf_traj, double* perf_sigma, double* perf_cov,
                                          int terminal_safety, int32_t* status, void* stream) {
    if (!model || !env || !x0 || !safe_actions || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || H <= 0 || r < 1 || r > H || n_perf <= r) return SX_ERR_ARG;
    if (tail_noise && (!tail_mean || !tail_std)) return SX_ERR_ARG;
    if (!model->x_train || model->n_train <= 0 || model->n_s != env->n_s || model->n_u != env->n_u) return SX_ERR_ARG;
    if (!sx::perf_taylor_shape_ok(model) || !sx::perf_var_model_ok(*model)) return SX_ERR_ARG;
    if (env->obj_mode != SX_OBJ_NEG_VARIANCE && env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    if (terminal_safety && (n_perf < H + 2 || env->m <= 0)) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const sx::PerfTaylorPtrs tp{{{x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj,
                                  status, E, P, H, n_perf, r},
                                 perf_sigma, env->obj_mode},
                                perf_cov, env->m, terminal_safety ? H + 1 : -1};
    return sx::perf_taylor_dispatch(model, env, tp, (hipStream_t)stream);
}
