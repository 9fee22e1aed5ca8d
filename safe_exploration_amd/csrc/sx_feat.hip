// The feature-space GP (sx_feat.hpp, sx_feat_fit.hpp): its one-model kernels and launchers, and the entries sx_feat_features,
// sx_feat_fit, sx_feat_predict, sx_cem_rollout_feat[_junk|_multi], sx_feat_model_table[_bytes].  The multi-model rollout
// kernels are compiled in sx_model_multi.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/sx_amd.h"
#include "sx_feat.hpp"
#include "sx_feat_fit.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_model_multi.hpp"
#include "sx_model_shapes.hpp"

namespace sx {

template <int NS, int NU>
static int launch_feat_predict(const sx_feat_model* m, const double* z, int P, double* mean, double* var, double* jac,
                               hipStream_t stream) {
    const FeatConst fc = make_feat_const(m);
    const size_t lds = kFeatLdsDoubles * sizeof(double);
    if (int rc = allow_lds(feat_predict_kernel<NS, NU>, lds)) return rc;
    hipLaunchKernelGGL((feat_predict_kernel<NS, NU>), dim3((P + kFeatWave - 1) / kFeatWave), dim3(kFeatWave), lds, stream, fc, z,
                       P, mean, var, jac);
    return check_launch();
}

template <int NS, int NU, int SH = 0>
static int launch_rollout_feat(const sx_feat_model* m, const sx_env* env, const FeatRolloutPtrs& rp, hipStream_t stream) {
    const FeatConst fc = make_feat_const(m);
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if (int r = env_consts<NS, NU>(env, rc, cc)) return r;
    const size_t lds = kFeatLdsDoubles * sizeof(double);
    if (int r = allow_lds(cem_rollout_feat_kernel<NS, NU, SH>, lds)) return r;
    const int64_t total = (int64_t)rp.E * rp.P;
    launch(SX_PROF_ROLLOUT_FEAT, cem_rollout_feat_kernel<NS, NU, SH>, dim3((unsigned)((total + kFeatWave - 1) / kFeatWave)),
           dim3(kFeatWave), lds, stream, fc, rc, cc, rp);
    return check_launch();
}

// sx_cem_rollout_feat_multi after its checks: the problems' shared constants, then the launch
template <int NS, int NU>
static int feat_multi_launch(const FeatConst* table, const sx_env* env, const FeatRolloutPtrs& rp, hipStream_t stream) {
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if (int r = env_consts<NS, NU>(env, rc, cc)) return r;
    return launch_rollout_feat_multi<NS, NU>(table, rc, cc, rp, stream);
}

}  // namespace sx

extern "C" {

// wide: the kept-column model of sx_cem_rollout_feat_junk, n_u = real actions + query shift, n_s + n_u <= SX_MAX_D
static bool feat_model_ok(const sx_feat_model* m, bool wide = false) {
    if (!m || m->n_s <= 0 || m->n_s > SX_MAX_NS || m->n_u <= 0) return false;
    if (m->n_u > (wide ? SX_MAX_D - m->n_s : SX_MAX_NU)) return false;
    if (m->n_layers < 0 || m->n_layers > SX_FEAT_MAX_LAYERS || m->n_feat <= 0 || m->n_feat > SX_FEAT_MAX_WIDTH) return false;
    if (m->width[0] != m->n_s + m->n_u) return false;
    for (int l = 1; l <= m->n_layers; ++l)
        if (m->width[l] <= 0 || m->width[l] > SX_FEAT_MAX_WIDTH) return false;
    if (m->n_layers == 0 ? m->n_feat != m->n_s + m->n_u : (m->n_feat != m->width[m->n_layers] || !m->net)) return false;
    return true;
}

int sx_feat_features(const sx_feat_model* model, const double* x, int N, double* phi, void* stream) {
    if (!feat_model_ok(model, true) || N < 0) return SX_ERR_ARG;
    if (N == 0) return SX_OK;
    if (!x || !phi) return SX_ERR_ARG;
    const sx::FeatConst fc = sx::make_feat_const(model);
    const size_t lds = sx::kFeatLdsDoubles * sizeof(double);
    const dim3 grid((N + sx::kFeatWave - 1) / sx::kFeatWave);
#define FEAT_D(DD)                                                                                                          \
    if (fc.d_in == DD) {                                                                                                   \
        if (int rc = sx::allow_lds(sx::feat_features_kernel<DD>, lds)) return rc;                                          \
        hipLaunchKernelGGL(sx::feat_features_kernel<DD>, grid, dim3(sx::kFeatWave), lds, (hipStream_t)stream, fc, x, N, phi); \
        return sx::check_launch();                                                                                         \
    }
    FEAT_D(2) FEAT_D(3) FEAT_D(4) FEAT_D(5) FEAT_D(6)
#undef FEAT_D
    return SX_ERR_UNSUPPORTED;
}

int sx_feat_fit(const sx_feat_model* model, const double* phi, const double* y, int N, const double* lambda, double* wbar,
                double* minv, double* stats, int32_t* status, void* stream) {
    if (!feat_model_ok(model, true) || !phi || !y || N <= 0 || !lambda || !wbar || !minv || !stats || !status) return SX_ERR_ARG;
    sx::FeatFitArgs fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.phi = phi;
    fa.y = y;
    for (int d = 0; d < model->n_s; ++d) fa.lambda[d] = lambda[d];
    fa.wbar = wbar;
    fa.minv = minv;
    fa.stats = stats;
    fa.status = status;
    fa.n = N;
    fa.F = model->n_feat;
    fa.n_s = model->n_s;
    hipLaunchKernelGGL(sx::feat_fit_kernel, dim3(model->n_s), dim3(1024), 0, (hipStream_t)stream, fa);
    return sx::check_launch();
}

int sx_feat_predict(const sx_feat_model* model, const double* z, int P, double* mean, double* var, double* jac, void* stream) {
    if (!feat_model_ok(model) || P < 0) return SX_ERR_ARG;
    if (P == 0) return SX_OK;
    if (!z || !mean || !var || !model->wbar || !model->minv) return SX_ERR_ARG;
#define CALL(NS, NU) sx::launch_feat_predict<NS, NU>(model, z, P, mean, var, jac, (hipStream_t)stream)
    SX_DISPATCH(model->n_s, model->n_u, CALL);
#undef CALL
}

int sx_cem_rollout_feat(const sx_feat_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                        const double* mean, const double* std, const double* noise, double* actions, double* traj,
                        double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream) {
    return sx_cem_rollout_feat_junk(model, env, 0, E, P, H, x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost,
                                    status, stream);
}

int sx_cem_rollout_feat_junk(const sx_feat_model* model, const sx_env* env, int query_shift, int E, int P, int H,
                             const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                             double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                             int32_t* status, void* stream) {
    const sx::FeatRolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    if (!feat_model_ok(model, query_shift > 0) || !model->wbar || !model->minv) return SX_ERR_ARG;
    if (!sx::rollout_args_ok(env, rp) || !sx::junk_env_ok(env, model->n_s, model->n_u, query_shift)) return SX_ERR_ARG;
#define CALL(NS, NU, SH) sx::launch_rollout_feat<NS, NU, SH>(model, env, rp, (hipStream_t)stream)
#define CALL_0(NS, NU) CALL(NS, NU, 0)
    SX_MODEL_JUNK_DISPATCH(env->n_s, env->n_u, query_shift, CALL);
#undef CALL_0
#undef CALL
}

// The E models of sx_feat_model_table / sx_cem_rollout_feat_multi share (n_s, n_u), checked with the arguments (SX_ERR_ARG),
// and their architecture, which fixes the kernel and its LDS for the whole launch (SX_ERR_UNSUPPORTED otherwise, like a
// shape without a kernel).
static int feat_models_check(const sx_feat_model* models, int E) {
    if (!models || E <= 0) return SX_ERR_ARG;
    const sx_feat_model& a = models[0];
    for (int i = 0; i < E; ++i) {
        const sx_feat_model& m = models[i];
        if (!feat_model_ok(&m) || m.n_s != a.n_s || m.n_u != a.n_u) return SX_ERR_ARG;
    }
    for (int i = 1; i < E; ++i) {
        const sx_feat_model& m = models[i];
        if (m.n_layers != a.n_layers || m.normalise != a.normalise || m.n_feat != a.n_feat) return SX_ERR_UNSUPPORTED;
        for (int l = 0; l <= a.n_layers; ++l)
            if (m.width[l] != a.width[l]) return SX_ERR_UNSUPPORTED;
    }
    if (!sx::rollout_compiled(a.n_s, a.n_u, 0)) return SX_ERR_UNSUPPORTED;
    return SX_OK;
}

int64_t sx_feat_model_table_bytes(const sx_feat_model* models, int E) {
    return feat_models_check(models, E) == SX_OK ? (int64_t)E * (int64_t)sizeof(sx::FeatConst) : -1;
}

int sx_feat_model_table(const sx_feat_model* models, int E, void* table, void* stream) {
    if (!table) return SX_ERR_ARG;
    if (int r = feat_models_check(models, E)) return r;
    for (int i = 0; i < E; ++i)
        if (!models[i].wbar || !models[i].minv) return SX_ERR_ARG;
    std::vector<sx::FeatConst> host(E);
    for (int i = 0; i < E; ++i) host[i] = sx::make_feat_const(&models[i]);
    return sx::copy_model_table(host, table, (hipStream_t)stream);
}

int sx_cem_rollout_feat_multi(const sx_feat_model* models, const void* table, const sx_env* env, int E, int P, int H,
                              const double* x0, const double* q0, const double* mean, const double* std,
                              const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                              double* con_cost, int32_t* status, void* stream) {
    const sx::FeatRolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    if (!table || !sx::rollout_args_ok(env, rp)) return SX_ERR_ARG;
    const int check = feat_models_check(models, E);
    if (check == SX_ERR_ARG || models[0].n_s != env->n_s || models[0].n_u != env->n_u) return SX_ERR_ARG;
    if (check != SX_OK) return check;
    const auto* tab = static_cast<const sx::FeatConst*>(table);
#define CALL(NS, NU) sx::feat_multi_launch<NS, NU>(tab, env, rp, (hipStream_t)stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

}  // extern "C"
