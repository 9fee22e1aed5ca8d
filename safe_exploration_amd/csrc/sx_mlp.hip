// The MC-dropout ensemble (sx_mlp.hpp, sx_mlp_mfma.hpp): its one-model kernels and launchers, and the entries sx_mlp_predict,
// sx_cem_rollout_mlp[_junk|_multi], sx_mlp_model_table[_bytes].  The multi-model rollout kernels are compiled in
// sx_model_multi.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/sx_amd.h"
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_mlp.hpp"
#include "sx_mlp_mfma.hpp"
#include "sx_model_multi.hpp"
#include "sx_model_shapes.hpp"

namespace sx {

// SX_MLP_PATH=valu keeps every network on the one-particle-per-lane kernel (A/B runs; the default is the matrix-core
// kernel wherever mlp_mfma_ok() holds)
static bool mlp_use_mfma(const MlpConst& mc) {
    const char* e = getenv("SX_MLP_PATH");   // read per launch, so that a test can switch between the two kernels
    return !(e && strcmp(e, "valu") == 0) && mlp_mfma_ok(mc);
}

template <int NS, int NU, int L, bool FULL>
static int launch_mlp_predict_mfma(const MlpConst& mc, const double* z, int P, double* mean, double* var, double* jac,
                                   hipStream_t stream) {
    const size_t lds = (size_t)MmLds<NS, NS + NU>::total * sizeof(double);
    if (int rc = allow_lds(mlp_predict_mfma_kernel<NS, NU, L, FULL>, lds)) return rc;
    hipLaunchKernelGGL((mlp_predict_mfma_kernel<NS, NU, L, FULL>), dim3((P + kMmTile - 1) / kMmTile), dim3(kMmThreads), lds, stream,
                       mc, z, P, mean, var, jac);
    return check_launch();
}

template <int NS, int NU>
static int launch_mlp_predict(const sx_mlp_model* m, const double* z, int P, double* mean, double* var, double* jac,
                              hipStream_t stream) {
    const MlpConst mc = make_mlp_const(m);
    if (mlp_use_mfma(mc)) {
        return mlp_mfma_form(mc, [&](auto l, auto full) {
            return launch_mlp_predict_mfma<NS, NU, decltype(l)::value, decltype(full)::value>(mc, z, P, mean, var, jac, stream);
        });
    }
    const size_t lds = mlp_lds_doubles(mc.n_hidden, mc.wmax) * sizeof(double);
    if (int rc = allow_lds(mlp_predict_kernel<NS, NU>, lds)) return rc;
    hipLaunchKernelGGL((mlp_predict_kernel<NS, NU>), dim3((P + kMlpLanes - 1) / kMlpLanes), dim3(kMlpLanes), lds, stream, mc, z,
                       P, mean, var, jac);
    return check_launch();
}

template <int NS, int NU, int L, bool FULL, int SH>
static int launch_rollout_mlp_mfma(const MlpConst& mc, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                                   const FeatRolloutPtrs& rp, hipStream_t stream) {
    const size_t lds = (size_t)MmLds<NS, NS + NU + SH>::total * sizeof(double);
    if (int r = allow_lds(cem_rollout_mlp_mfma_kernel<NS, NU, L, FULL, SH>, lds)) return r;
    const int64_t total = (int64_t)rp.E * rp.P;
    launch(SX_PROF_ROLLOUT_MLP, cem_rollout_mlp_mfma_kernel<NS, NU, L, FULL, SH>,
           dim3((unsigned)((total + kMmTile - 1) / kMmTile)),
           dim3(kMmThreads), lds, stream, mc, rc, cc, rp);
    return check_launch();
}

template <int NS, int NU, int SH = 0>
static int launch_rollout_mlp(const sx_mlp_model* m, const sx_env* env, const FeatRolloutPtrs& rp, hipStream_t stream) {
    const MlpConst mc = make_mlp_const(m);
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if (int r = env_consts<NS, NU>(env, rc, cc)) return r;
    if (mlp_use_mfma(mc)) {
        return mlp_mfma_form(mc, [&](auto l, auto full) {
            return launch_rollout_mlp_mfma<NS, NU, decltype(l)::value, decltype(full)::value, SH>(mc, rc, cc, rp, stream);
        });
    }
    const size_t lds = mlp_lds_doubles(mc.n_hidden, mc.wmax) * sizeof(double);
    if (int r = allow_lds(cem_rollout_mlp_kernel<NS, NU, SH>, lds)) return r;
    const int64_t total = (int64_t)rp.E * rp.P;
    launch(SX_PROF_ROLLOUT_MLP, cem_rollout_mlp_kernel<NS, NU, SH>, dim3((unsigned)((total + kMlpLanes - 1) / kMlpLanes)),
           dim3(kMlpLanes), lds, stream, mc, rc, cc, rp);
    return check_launch();
}

// sx_cem_rollout_mlp_multi after its checks: the problems' shared constants, then the launch
template <int NS, int NU>
static int mlp_multi_launch(const MlpConst* table, const MlpConst& arch, bool mfma, const sx_env* env,
                            const FeatRolloutPtrs& rp, hipStream_t stream) {
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if (int r = env_consts<NS, NU>(env, rc, cc)) return r;
    return launch_rollout_mlp_multi<NS, NU>(table, arch, mfma, rc, cc, rp, stream);
}

}  // namespace sx

extern "C" {

// wide: the kept-column model of sx_cem_rollout_mlp_junk, n_u = real actions + query shift, n_s + n_u <= SX_MAX_D
static bool mlp_model_ok(const sx_mlp_model* m, bool wide = false) {
    if (!m || m->n_s <= 0 || m->n_s > SX_MAX_NS || m->n_u <= 0) return false;
    if (m->n_u > (wide ? SX_MAX_D - m->n_s : SX_MAX_NU)) return false;
    if (m->n_hidden < 0 || m->n_hidden > SX_MLP_MAX_HIDDEN || m->n_out < m->n_s || m->n_samples <= 0) return false;
    if (m->predict_std && m->n_out < 2 * m->n_s) return false;
    if (m->width[0] != m->n_s + m->n_u || !m->net || !m->masks) return false;
    for (int l = 1; l <= m->n_hidden; ++l)
        if (m->width[l] <= 0 || m->width[l] > SX_MLP_MAX_WIDTH) return false;
    return true;
}

int sx_mlp_predict(const sx_mlp_model* model, const double* z, int P, double* mean, double* var, double* jac, void* stream) {
    if (!mlp_model_ok(model) || P < 0) return SX_ERR_ARG;
    if (P == 0) return SX_OK;
    if (!z || !mean || !var) return SX_ERR_ARG;
#define CALL(NS, NU) sx::launch_mlp_predict<NS, NU>(model, z, P, mean, var, jac, (hipStream_t)stream)
    SX_DISPATCH(model->n_s, model->n_u, CALL);
#undef CALL
}

int sx_cem_rollout_mlp(const sx_mlp_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                       const double* mean, const double* std, const double* noise, double* actions, double* traj,
                       double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream) {
    return sx_cem_rollout_mlp_junk(model, env, 0, E, P, H, x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost,
                                   status, stream);
}

int sx_cem_rollout_mlp_junk(const sx_mlp_model* model, const sx_env* env, int query_shift, int E, int P, int H,
                            const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                            double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                            int32_t* status, void* stream) {
    const sx::FeatRolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    if (!mlp_model_ok(model, query_shift > 0)) return SX_ERR_ARG;
    if (!sx::rollout_args_ok(env, rp) || !sx::junk_env_ok(env, model->n_s, model->n_u, query_shift)) return SX_ERR_ARG;
#define CALL(NS, NU, SH) sx::launch_rollout_mlp<NS, NU, SH>(model, env, rp, (hipStream_t)stream)
#define CALL_0(NS, NU) CALL(NS, NU, 0)
    SX_MODEL_JUNK_DISPATCH(env->n_s, env->n_u, query_shift, CALL);
#undef CALL_0
#undef CALL
}

// The E models of sx_mlp_model_table / sx_cem_rollout_mlp_multi share (n_s, n_u), checked with the arguments (SX_ERR_ARG),
// and their architecture, which fixes the kernel and its LDS for the whole launch (SX_ERR_UNSUPPORTED otherwise, like a
// shape without a kernel).
static int mlp_models_check(const sx_mlp_model* models, int E) {
    if (!models || E <= 0) return SX_ERR_ARG;
    const sx_mlp_model& a = models[0];
    for (int i = 0; i < E; ++i) {
        const sx_mlp_model& m = models[i];
        if (!mlp_model_ok(&m) || m.n_s != a.n_s || m.n_u != a.n_u) return SX_ERR_ARG;
    }
    for (int i = 1; i < E; ++i) {
        const sx_mlp_model& m = models[i];
        if (m.n_hidden != a.n_hidden || m.n_out != a.n_out || m.n_samples != a.n_samples || m.predict_std != a.predict_std)
            return SX_ERR_UNSUPPORTED;
        for (int l = 0; l <= a.n_hidden; ++l)
            if (m.width[l] != a.width[l]) return SX_ERR_UNSUPPORTED;
    }
    if (!sx::rollout_compiled(a.n_s, a.n_u, 0)) return SX_ERR_UNSUPPORTED;
    return SX_OK;
}

int64_t sx_mlp_model_table_bytes(const sx_mlp_model* models, int E) {
    return mlp_models_check(models, E) == SX_OK ? (int64_t)E * (int64_t)sizeof(sx::MlpConst) : -1;
}

int sx_mlp_model_table(const sx_mlp_model* models, int E, void* table, void* stream) {
    if (!table) return SX_ERR_ARG;
    if (int r = mlp_models_check(models, E)) return r;
    std::vector<sx::MlpConst> host(E);
    for (int i = 0; i < E; ++i) host[i] = sx::make_mlp_const(&models[i]);
    return sx::copy_model_table(host, table, (hipStream_t)stream);
}

int sx_cem_rollout_mlp_multi(const sx_mlp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                             const double* x0, const double* q0, const double* mean, const double* std,
                             const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                             double* con_cost, int32_t* status, void* stream) {
    const sx::FeatRolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    if (!table || !sx::rollout_args_ok(env, rp)) return SX_ERR_ARG;
    const int check = mlp_models_check(models, E);
    if (check == SX_ERR_ARG || models[0].n_s != env->n_s || models[0].n_u != env->n_u) return SX_ERR_ARG;
    if (check != SX_OK) return check;
    const auto* tab = static_cast<const sx::MlpConst*>(table);
    const sx::MlpConst arch = sx::make_mlp_const(&models[0]);
    const bool mfma = sx::mlp_use_mfma(arch);   // (the same answer for every model: they share the architecture)
#define CALL(NS, NU) sx::mlp_multi_launch<NS, NU>(tab, arch, mfma, env, rp, (hipStream_t)stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

}  // extern "C"
