// sx_cem_perf_rollout_var: the performance-trajectory kernel with the posterior variance (sx_perf_var.hpp) for every
// shift-0 shape of SX_ROLLOUT_SHAPES in both of its forms, its launcher and the entry point.  A translation unit of its
// own: nothing the other objects compile changes with it.
#include <climits>
#include <cstring>

#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH, rollout_stream_lds_bytes
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

// The form of the launch, as plan_rollout (sx_gp_rollout.hpp) decides the streaming safety kernel's: Kstar of all outputs
// in LDS where they fit beside the n_perf actions of the tile, else output by output (n_s > 1), else SX_ERR_UNSUPPORTED --
// there is no resident-W form and no workspace path here.
template <int NS, int NU>
static int perf_var_rollout(const sx_gp_model* m, const sx_env* env, const PerfVarPtrs& vp, hipStream_t stream) {
    const PerfPtrs& pp = vp.p;
    auto lds_bytes = [&](bool byout) { return rollout_stream_lds_bytes(NS, NU, 0, m->n_train, m->n_pad, pp.n_perf, byout); };
    const bool fits = m->n_pad <= 1024;
    const bool all_at_once = fits && lds_bytes(false) <= kMaxLdsBytes;
    const bool by_output = !all_at_once && NS > 1 && fits && lds_bytes(true) <= kMaxLdsBytes;
    const int64_t blocks = (int64_t)pp.E * ((pp.P + SX_TILE - 1) / SX_TILE);
    if ((!all_at_once && !by_output) || blocks > INT_MAX) return SX_ERR_UNSUPPORTED;
    PerfStepConst<NS, NU> sc;
    std::memset(&sc, 0, sizeof(sc));
    for (int i = 0; i < NS * NS; ++i) sc.a[i] = env->a[i];
    for (int i = 0; i < NS * NU; ++i) sc.b[i] = env->b[i];
    for (int c = 0; c < NU; ++c) {
        sc.u_min[c] = env->u_min[c];
        sc.u_max[c] = env->u_max[c];
    }
    for (int i = 0; i < NS; ++i) {
        sc.w_abs[i] = env->obj_w_abs[i];
        sc.target[i] = env->obj_target[i];
        sc.w_lin[i] = env->obj_w_lin[i];
    }
    const GpConst<NS, NS + NU> gc = make_gp_const<NS, NU>(m, kPerfVarThreads / 64);
    return by_output ? launch_perf_var<NS, NU, true>(gc, sc, vp, (unsigned)blocks, lds_bytes(true), stream)
                     : launch_perf_var<NS, NU, false>(gc, sc, vp, (unsigned)blocks, lds_bytes(false), stream);
}

static int perf_var_dispatch(const sx_gp_model* m, const sx_env* env, const PerfVarPtrs& vp, hipStream_t stream) {
#define CALL(NS, NU) perf_var_rollout<NS, NU>(m, env, vp, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

}  // namespace sx

extern "C" int sx_cem_perf_rollout_var(const sx_gp_model* model, const sx_env* env, int E, int P, int H, int n_perf, int r,
                                       const double* x0, const double* safe_actions, const double* tail_mean,
                                       const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                                       double* con_cost, double* perf_traj, double* perf_sigma, int32_t* status,
                                       void* stream) {
    if (!model || !env || !x0 || !safe_actions || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || H <= 0 || r < 1 || r > H || n_perf <= r) return SX_ERR_ARG;
    if (tail_noise && (!tail_mean || !tail_std)) return SX_ERR_ARG;
    if (!model->x_train || model->n_train <= 0 || model->n_s != env->n_s || model->n_u != env->n_u) return SX_ERR_ARG;
    // the packed model of sx_gp_pack: W fragments, the stage table, and the padding that holds the mean / Jacobian rows
    if (!model->a_pack || !model->stage_tab) return SX_ERR_ARG;
    if (model->n_pad % 16 != 0 || model->n_pad <= model->n_train + model->n_s + model->n_u) return SX_ERR_ARG;
    if (env->obj_mode != SX_OBJ_NEG_VARIANCE && env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    const sx::PerfVarPtrs vp{{x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj, status,
                              E, P, H, n_perf, r},
                             perf_sigma, env->obj_mode};
    return sx::perf_var_dispatch(model, env, vp, (hipStream_t)stream);
}
