// sx_cem_perf_rollout: the performance-trajectory kernel (sx_perf.hpp) for every shift-0 shape of SX_ROLLOUT_SHAPES, its
// launcher and the entry point.  A translation unit of its own: nothing the other objects compile changes with it.
#include <climits>
#include <cstring>

#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf.hpp"

namespace sx {

template <int NS, int NU>
int launch_perf_rollout(const PerfConst<NS, NU>& pc, const PerfPtrs& pp, hipStream_t stream) {
    const int64_t blocks = ((int64_t)pp.E * pp.P + kPerfTile - 1) / kPerfTile;
    const size_t lds = perf_lds_bytes(NS, NU, pc.n_train);
    if (blocks > INT_MAX || lds > kMaxLdsBytes) return SX_ERR_UNSUPPORTED;
    if (int r = allow_lds(cem_perf_rollout_kernel<NS, NU>, lds)) return r;
    hipLaunchKernelGGL((cem_perf_rollout_kernel<NS, NU>), dim3((unsigned)blocks), dim3(kPerfThreads), lds, stream, pc, pp);
    return check_launch();
}

template <int NS, int NU>
static int perf_rollout(const sx_gp_model* m, const double* alpha, const sx_env* env, const PerfPtrs& pp,
                        hipStream_t stream) {
    PerfConst<NS, NU> pc;
    std::memset(&pc, 0, sizeof(pc));
    exp_hyper(*m, pc.k_nh_ils2, pc.k_log_os);
    for (int i = 0; i < NS * NS; ++i) pc.step.a[i] = env->a[i];
    for (int i = 0; i < NS * NU; ++i) pc.step.b[i] = env->b[i];
    for (int c = 0; c < NU; ++c) {
        pc.step.u_min[c] = env->u_min[c];
        pc.step.u_max[c] = env->u_max[c];
    }
    for (int i = 0; i < NS; ++i) {
        pc.step.w_abs[i] = env->obj_w_abs[i];
        pc.step.target[i] = env->obj_target[i];
        pc.step.w_lin[i] = env->obj_w_lin[i];
    }
    pc.x_train = m->x_train;
    pc.alpha = alpha;
    pc.n_train = m->n_train;
    pc.n_pad = perf_n_pad(m->n_train);
    return launch_perf_rollout<NS, NU>(pc, pp, stream);
}

static int perf_dispatch(const sx_gp_model* m, const double* alpha, const sx_env* env, const PerfPtrs& pp,
                         hipStream_t stream) {
#define CALL(NS, NU) perf_rollout<NS, NU>(m, alpha, env, pp, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

}  // namespace sx

extern "C" int sx_cem_perf_rollout(const sx_gp_model* model, const double* alpha, const sx_env* env, int E, int P, int H,
                                   int n_perf, int r, const double* x0, const double* safe_actions,
                                   const double* tail_mean, const double* tail_std, const double* tail_noise, double* rows,
                                   double* obj_cost, double* con_cost, double* perf_traj, int32_t* status, void* stream) {
    if (!model || !alpha || !env || !x0 || !safe_actions || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || H <= 0 || r < 1 || r > H || n_perf <= r) return SX_ERR_ARG;
    if (tail_noise && (!tail_mean || !tail_std)) return SX_ERR_ARG;
    if (!model->x_train || model->n_train <= 0 || model->n_s != env->n_s || model->n_u != env->n_u) return SX_ERR_ARG;
    if (env->obj_mode == SX_OBJ_NEG_VARIANCE) return SX_ERR_UNSUPPORTED;   // needs || W k* ||^2: the safety kernels' product
    if (env->obj_mode != SX_OBJ_AFFINE_ABS) return SX_ERR_ARG;
    const sx::PerfPtrs pp{x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj, status,
                          E, P, H, n_perf, r};
    return sx::perf_dispatch(model, alpha, env, pp, (hipStream_t)stream);
}
