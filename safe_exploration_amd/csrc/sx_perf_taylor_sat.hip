// sx_cem_perf_rollout_taylor_sat[_multi]: the Taylor performance rollout with the saturating cost as its objective
// (cem_perf_gp_rollout_kernel of kind PerfTaylorKind<true>) for every shift-0 shape of SX_ROLLOUT_SHAPES in both forms, and
// the two entries (the multi-model kernels are compiled in sx_perf_taylor_sat_multi.hip).  The plan is the parent's: the
// cost's constants are no LDS.  A translation unit of its own: nothing the other objects compile changes with it.
#include "sx_perf_taylor_host.hpp"   // PerfTaylorForm, perf_taylor_launch

namespace sx {

struct PerfTaylorSatForm {
    template <int NS, int NU>
    using Const = PerfTaylorSatConst<NS, NU>;
    using Ptrs = PerfTaylorPtrs;
    static const PerfPtrs& base(const Ptrs& tp) { return tp.p; }
    static size_t extra_bytes(int ns, int nu) { return perf_taylor_extra_bytes(ns, nu); }
    template <int NS, int NU>
    static void make_const(const sx_env* env, Const<NS, NU>& c) {
        PerfTaylorForm::make_const<NS, NU>(env, c.tc);
        make_sat_const<NS>(sat_cost_of(env), c.sat);
    }
    template <int NS, int NU, bool BYOUT>
    static auto kernel() {
        return cem_perf_gp_rollout_kernel<PerfTaylorKind<true>, NS, NU, BYOUT, false, const int4* __restrict__>;
    }
};

}  // namespace sx

extern "C" int sx_cem_perf_rollout_taylor_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env,
                                                    const sx_sat_cost* cost, int E, int P, int H, int n_perf, int r,
                                                    const double* x0, const double* safe_actions, const double* tail_mean,
                                                    const double* tail_std, const double* tail_noise, double* rows,
                                                    double* obj_cost, double* con_cost, double* perf_traj,
                                                    double* perf_sigma, double* perf_cov, int terminal_safety,
                                                    int32_t* status, void* stream) {
    if (!env || !cost) return SX_ERR_ARG;
    const sx::SatEnv se = sx::make_sat_env(env, cost);
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    if (int rc = sx::check_perf_entry(table, models, E, true, sx::perf_var_model_ok, &se.env, pp, true)) return rc;
    if (!sx::sat_cost_ok(cost, env->n_s)) return SX_ERR_ARG;
    return sx::perf_taylor_launch<sx::PerfTaylorSatForm>(models, table, &se.env, pp, perf_sigma, perf_cov, terminal_safety,
                                                         stream);
}

extern "C" int sx_cem_perf_rollout_taylor_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E,
                                              int P, int H, int n_perf, int r, const double* x0, const double* safe_actions,
                                              const double* tail_mean, const double* tail_std, const double* tail_noise,
                                              double* rows, double* obj_cost, double* con_cost, double* perf_traj,
                                              double* perf_sigma, double* perf_cov, int terminal_safety, int32_t* status,
                                              void* stream) {
    if (!env || !cost) return SX_ERR_ARG;
    const sx::SatEnv se = sx::make_sat_env(env, cost);
    const sx::PerfPtrs pp = sx::make_perf_ptrs(x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost,
                                               perf_traj, status, E, P, H, n_perf, r);
    if (int rc = sx::check_perf_entry(true, model, 1, true, sx::perf_var_model_ok, &se.env, pp, true)) return rc;
    if (!sx::sat_cost_ok(cost, env->n_s)) return SX_ERR_ARG;
    return sx::perf_taylor_launch<sx::PerfTaylorSatForm>(model, nullptr, &se.env, pp, perf_sigma, perf_cov, terminal_safety,
                                                         stream);
}
