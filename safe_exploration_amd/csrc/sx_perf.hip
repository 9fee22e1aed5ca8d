// sx_cem_perf_rollout: the performance-trajectory kernel (sx_perf.hpp) for every shift-0 shape of SX_ROLLOUT_SHAPES, its
// launcher and the entry point; the entries of the multi-model mode (sx_cem_perf_table[_bytes], sx_cem_perf_rollout_multi),
// whose kernels sx_perf_multi.hip compiles.  A translation unit of its own: nothing the other objects compile changes with it.
#include <algorithm>
#include <vector>
#include <climits>
#include <cstring>

#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf.hpp"
#include "sx_perf_launch.hpp"   // the entries' shared checks

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
    make_perf_step<NS, NU>(env, pc.step);
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

// Bytes of one sx_cem_perf_table entry (SX_ERR_UNSUPPORTED for a shape without a kernel)
template <int NS, int NU>
static int64_t perf_entry_bytes() {
    return (int64_t)sizeof(PerfGpEntry<NS, NU>);
}
static int64_t perf_entry_bytes(int ns, int nu) {
#define CALL(NS, NU) perf_entry_bytes<NS, NU>()
    SX_DISPATCH(ns, nu, CALL);
#undef CALL
}

template <int NS, int NU>
static int build_perf_table(const sx_gp_model* models, const double* const* alphas, int E, void* table, hipStream_t stream) {
    std::vector<PerfGpEntry<NS, NU>> host(E);
    for (int i = 0; i < E; ++i) {
        std::memset(&host[i], 0, sizeof(host[i]));
        exp_hyper(models[i], host[i].k_nh_ils2, host[i].k_log_os);
        host[i].x_train = models[i].x_train;
        host[i].alpha = alphas[i];
        host[i].n_train = models[i].n_train;
        host[i].n_pad = perf_n_pad(models[i].n_train);
    }
    return copy_model_table(host, table, stream);
}

template <int NS, int NU>
static int perf_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env, const PerfPtrs& pp,
                              hipStream_t stream) {
    size_t lds = 0;   // the launch's allocation: the largest model's
    for (int i = 0; i < pp.E; ++i) lds = std::max(lds, perf_lds_bytes(NS, NU, models[i].n_train));
    if (lds > kMaxLdsBytes) return SX_ERR_UNSUPPORTED;
    PerfStepConst<NS, NU> step;
    std::memset(&step, 0, sizeof(step));
    make_perf_step<NS, NU>(env, step);
    return launch_perf_rollout_multi<NS, NU>(static_cast<const PerfGpEntry<NS, NU>*>(table), step, pp, lds, stream);
}

static int perf_multi_dispatch(const sx_gp_model* models, const void* table, const sx_env* env, const PerfPtrs& pp,
                               hipStream_t stream) {
#define CALL(NS, NU) perf_rollout_multi<NS, NU>(models, table, env, pp, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

}  // namespace sx

extern "C" int64_t sx_cem_perf_table_bytes(int n_s, int n_u, int E) {
    if (E <= 0 || n_s <= 0 || n_s > SX_MAX_NS || n_u <= 0 || n_u > SX_MAX_NU) return -1;
    const int64_t entry = sx::perf_entry_bytes(n_s, n_u);
    return entry == SX_ERR_UNSUPPORTED ? -1 : entry * E;
}

extern "C" int sx_cem_perf_table(const sx_gp_model* models, const double* const* alphas, int E, void* table, void* stream) {
    if (!table || !alphas || !models || E <= 0 || !sx::perf_shape_ok(models[0])) return SX_ERR_ARG;
    if (!sx::perf_models_ok(models, E, sx::perf_model_has_data)) return SX_ERR_ARG;
    for (int i = 0; i < E; ++i)
        if (!alphas[i]) return SX_ERR_ARG;
#define CALL(NS, NU) sx::build_perf_table<NS, NU>(models, alphas, E, table, (hipStream_t)stream)
    SX_DISPATCH(models[0].n_s, models[0].n_u, CALL);
#undef CALL
}

extern "C" int sx_cem_perf_rollout_multi(const sx_gp_model* models, const void* perf_table, const sx_env* env, int E, int P,
                                         int H, int n_perf, int r, const double* x0, const double* safe_actions,
                                         const double* tail_mean, const double* tail_std, const double* tail_noise,
                                         double* rows, double* obj_cost, double* con_cost, double* perf_traj,
                                         int32_t* status, void* stream) {
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    if (int rc = sx::check_perf_entry(perf_table, models, E, true, sx::perf_model_has_data, env, pp, false)) return rc;
    return sx::perf_multi_dispatch(models, perf_table, env, pp, (hipStream_t)stream);
}

extern "C" int sx_cem_perf_rollout(const sx_gp_model* model, const double* alpha, const sx_env* env, int E, int P, int H,
                                   int n_perf, int r, const double* x0, const double* safe_actions,
                                   const double* tail_mean, const double* tail_std, const double* tail_noise, double* rows,
                                   double* obj_cost, double* con_cost, double* perf_traj, int32_t* status, void* stream) {
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    // SX_OBJ_NEG_VARIANCE needs || W k* ||^2, the safety kernels' product: SX_ERR_UNSUPPORTED here
    if (int rc = sx::check_perf_entry(alpha, model, 1, false, sx::perf_model_has_data, env, pp, false)) return rc;
    return sx::perf_dispatch(model, alpha, env, pp, (hipStream_t)stream);
}
