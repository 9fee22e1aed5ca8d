// sx_cem_perf_rollout_taylor: the performance-trajectory kernel with Taylor uncertainty propagation (sx_perf_taylor.hpp)
// for every shift-0 shape of SX_ROLLOUT_SHAPES in both of its forms, its launcher and the entry points, those of the
// multi-model launch included (its kernels are compiled in sx_perf_taylor_multi.hip).  A translation unit of its own:
// nothing the other objects compile changes with it.
#include "sx_perf_taylor_host.hpp"   // PerfTaylorForm, perf_taylor_launch

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
