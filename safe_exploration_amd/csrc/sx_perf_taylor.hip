// sx_cem_perf_rollout_taylor: the performance-trajectory kernel with Taylor uncertainty propagation (sx_perf_taylor.hpp)
// for every shift-0 shape of SX_ROLLOUT_SHAPES in both of its forms, its launcher and the entry points, those of the
// multi-model launch included (its kernels are compiled in sx_perf_taylor_multi.hip).  A translation unit of its own:
// nothing the other objects compile changes with it.
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf_launch.hpp"
#include "sx_perf_taylor.hpp"

namespace sx {

// The Taylor form for perf_gp_rollout (sx_perf_launch.hpp): the variance form's plan with the step constants behind the
// tile's actions
struct PerfTaylorForm {
    template <int NS, int NU>
    using Const = PerfTaylorConst<NS, NU>;
    using Ptrs = PerfTaylorPtrs;
    static const PerfPtrs& base(const Ptrs& tp) { return tp.v.p; }
    static size_t extra_bytes(int ns, int nu) { return perf_taylor_extra_bytes(ns, nu); }
    template <int NS, int NU>
    static void make_const(const sx_env* env, Const<NS, NU>& tc) {
        static_assert(sizeof(PerfTaylorConst<NS, NU>) ==
                          (2 * NS * NS + 2 * NS * NU + 2 * NU + 3 * NS + SX_MAX_M * NS + SX_MAX_M) * sizeof(double),
                      "perf_taylor_extra_bytes counts the fields of PerfTaylorConst");
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
    static auto kernel() {
        return cem_perf_taylor_rollout_kernel<NS, NU, BYOUT>;
    }
};

// What both Taylor entries do behind check_perf_entry: terminal_safety, then the polytope rows, then the launch
static int perf_taylor_launch(const sx_gp_model* models, const void* table, const sx_env* env, const PerfPtrs& pp,
                              double* perf_sigma, double* perf_cov, int terminal_safety, void* stream) {
    if (terminal_safety && (pp.n_perf < pp.H + 2 || env->m <= 0)) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const PerfTaylorPtrs tp{{pp, perf_sigma, env->obj_mode}, perf_cov, env->m, terminal_safety ? pp.H + 1 : -1};
    return perf_gp_dispatch<PerfTaylorForm>(models, table, env, tp, (hipStream_t)stream);
}

}  // namespace sx

extern "C" int sx_cem_perf_rollout_taylor_form(const sx_gp_model* model, int n_perf) {
    return sx::perf_gp_form(model, 1, n_perf, true);
}

extern "C" int sx_cem_perf_rollout_taylor_multi_form(const sx_gp_model* models, int E, int n_perf) {
    return sx::perf_gp_form(models, E, n_perf, true);
}

extern "C" int sx_cem_perf_rollout_taylor_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E,
                                                int P, int H, int n_perf, int r, const double* x0,
                                                const double* safe_actions, const double* tail_mean,
                                                const double* tail_std, const double* tail_noise, double* rows,
                                                double* obj_cost, double* con_cost, double* perf_traj, double* perf_sigma,
                                                double* perf_cov, int terminal_safety, int32_t* status, void* stream) {
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    if (int rc = sx::check_perf_entry(table, models, E, true, sx::perf_var_model_ok, env, pp, true)) return rc;
    return sx::perf_taylor_launch(models, table, env, pp, perf_sigma, perf_cov, terminal_safety, stream);
}

extern "C" int sx_cem_perf_rollout_taylor(const sx_gp_model* model, const sx_env* env, int E, int P, int H, int n_perf,
                                          int r, const double* x0, const double* safe_actions, const double* tail_mean,
                                          const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                                          double* con_cost, double* perf_traj, double* perf_sigma, double* perf_cov,
                                          int terminal_safety, int32_t* status, void* stream) {
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    if (int rc = sx::check_perf_entry(true, model, 1, true, sx::perf_var_model_ok, env, pp, true)) return rc;
    return sx::perf_taylor_launch(model, nullptr, env, pp, perf_sigma, perf_cov, terminal_safety, stream);
}
