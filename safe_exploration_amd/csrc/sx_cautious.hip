// sx_cem_cautious_rollout: the chance-constrained Taylor rollout of Cautious MPC (sx_cautious.hpp) for every shift-0 shape
// of SX_ROLLOUT_SHAPES in both of its forms, and its entry points.  The host path from plan to launch is the performance
// rollouts' (perf_gp_rollout, sx_perf_launch.hpp) over one more form.  A translation unit of its own: nothing the other
// objects compile changes with it.
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf_launch.hpp"
#include "sx_cautious.hpp"

namespace sx {

// bytes of the step constants (CautiousConst) behind the tile's actions: the Taylor form's plus beta
inline size_t cautious_extra_bytes(int ns, int nu) { return perf_taylor_extra_bytes(ns, nu) + sizeof(double); }

// (perf_gp_rollout names the multi-model launcher of its form; there is no multi-model cautious launch, and no caller
// hands it a table)
template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>*, const CautiousConst<NS, NU>&, const CautiousPtrs&, bool, unsigned,
                         size_t, hipStream_t) {
    return SX_ERR_UNSUPPORTED;
}

// The cautious form for perf_gp_rollout: the Taylor form's plan (T steps of actions, the step constants behind them)
struct CautiousForm {
    template <int NS, int NU>
    using Const = CautiousConst<NS, NU>;
    using Ptrs = CautiousPtrs;
    static const PerfPtrs& base(const Ptrs& cp) { return cp.p; }
    static size_t extra_bytes(int ns, int nu) { return cautious_extra_bytes(ns, nu); }
    template <int NS, int NU>
    static void make_const(const sx_env* env, Const<NS, NU>& cc) {
        static_assert(sizeof(CautiousConst<NS, NU>) == sizeof(PerfTaylorConst<NS, NU>) + sizeof(double),
                      "cautious_extra_bytes counts the fields of CautiousConst");
        PerfTaylorConst<NS, NU>& tc = cc.tc;
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
        cc.beta = env->beta;
    }
    template <int NS, int NU, bool BYOUT>
    static auto kernel() {
        return cem_cautious_rollout_kernel<NS, NU, BYOUT>;
    }
};

// The plan of a model over T steps (plan_perf_var over the cautious constants), where the entry would take the model
static bool cautious_plan(const sx_gp_model* model, int T, PerfVarPlan& plan) {
    if (!model || T < 1 || !perf_shape_ok(*model) || !perf_models_ok(model, 1, perf_var_model_ok)) return false;
    plan = plan_perf_var(model->n_s, model->n_u, model->n_train, model->n_pad, T, cautious_extra_bytes(model->n_s, model->n_u));
    return true;
}

}  // namespace sx

extern "C" int sx_cem_cautious_rollout_form(const sx_gp_model* model, int T) {
    sx::PerfVarPlan plan;
    if (!sx::cautious_plan(model, T, plan)) return -1;
    return plan.ok ? plan.form : -1;
}

extern "C" int sx_cem_cautious_rollout(const sx_gp_model* model, const sx_env* env, int E, int P, int T, const double* x0,
                                       const double* mean, const double* std, const double* noise, double* rows,
                                       double* obj_cost, double* con_cost, double* traj, double* sigma, double* cov,
                                       double* margins, int propagate, int32_t* status, void* stream) {
    if (!model || !env || !x0 || !rows || !obj_cost || !con_cost || !status) return SX_ERR_ARG;
    if (E <= 0 || P <= 0 || T < 1) return SX_ERR_ARG;
    if (noise && (!mean || !std)) return SX_ERR_ARG;
    sx::PerfVarPlan plan;
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
