// sx_cem_perf_rollout_var: the performance-trajectory kernel with the posterior variance (sx_perf_var.hpp) for every
// shift-0 shape of SX_ROLLOUT_SHAPES in both of its forms, its launcher and the entry point.  A translation unit of its
// own: nothing the other objects compile changes with it.
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf_launch.hpp"
#include "sx_perf_var.hpp"

namespace sx {

// The variance form for perf_gp_rollout (sx_perf_launch.hpp): the mean-only step constants, nothing behind the actions
struct PerfVarForm {
    template <int NS, int NU>
    using Const = PerfStepConst<NS, NU>;
    using Ptrs = PerfVarPtrs;
    static const PerfPtrs& base(const Ptrs& vp) { return vp.p; }
    static size_t extra_bytes(int, int) { return 0; }
    template <int NS, int NU>
    static void make_const(const sx_env* env, Const<NS, NU>& sc) {
        make_perf_step<NS, NU>(env, sc);
    }
    template <int NS, int NU, bool BYOUT>
    static auto kernel() {
        return cem_perf_gp_rollout_kernel<PerfVarKind, NS, NU, BYOUT, false, const int4* __restrict__>;
    }
};

static int perf_var_launch(const sx_gp_model* models, const void* table, const sx_env* env, const PerfPtrs& pp,
                           double* perf_sigma, void* stream) {
    const PerfVarPtrs vp{pp, perf_sigma, env->obj_mode};
    return perf_gp_dispatch<PerfVarForm>(models, table, env, vp, (hipStream_t)stream);
}

}  // namespace sx

extern "C" int sx_cem_perf_rollout_var_form(const sx_gp_model* model, int n_perf) {
    return sx::perf_gp_form(model, 1, n_perf, false);
}

extern "C" int sx_cem_perf_rollout_var_multi_form(const sx_gp_model* models, int E, int n_perf) {
    return sx::perf_gp_form(models, E, n_perf, false);
}

extern "C" int sx_cem_perf_rollout_var_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P,
                                             int H, int n_perf, int r, const double* x0, const double* safe_actions,
                                             const double* tail_mean, const double* tail_std, const double* tail_noise,
                                             double* rows, double* obj_cost, double* con_cost, double* perf_traj,
                                             double* perf_sigma, int32_t* status, void* stream) {
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    if (int rc = sx::check_perf_entry(table, models, E, true, sx::perf_var_model_ok, env, pp, true)) return rc;
    return sx::perf_var_launch(models, table, env, pp, perf_sigma, stream);
}

extern "C" int sx_cem_perf_rollout_var(const sx_gp_model* model, const sx_env* env, int E, int P, int H, int n_perf, int r,
                                       const double* x0, const double* safe_actions, const double* tail_mean,
                                       const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                                       double* con_cost, double* perf_traj, double* perf_sigma, int32_t* status,
                                       void* stream) {
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    if (int rc = sx::check_perf_entry(true, model, 1, false, sx::perf_var_model_ok, env, pp, true)) return rc;
    return sx::perf_var_launch(model, nullptr, env, pp, perf_sigma, stream);
}
