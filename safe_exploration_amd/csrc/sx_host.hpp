// Host code the translation units of libsxamd share: what a launcher derives from an sx_gp_model or an sx_env, and the
// argument checks every rollout entry makes alike.  Inline / template host code only, no kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_reach.hpp"
#include "sx_rollout.hpp"

namespace sx {

constexpr int kPredictThreads = 64 * SX_WAVES;   // sx_gp_predict: one 16-point tile per workgroup

// The hyper-parameters of `m` into the arrays of a kernel argument: inv_ls2 [n_s x D], and where the argument has them
// outputscale [n_s] and noise [n_s].
inline void copy_hyper(const sx_gp_model& m, double* inv_ls2, double* outputscale = nullptr, double* noise = nullptr) {
    for (int i = 0; i < m.n_s * (m.n_s + m.n_u); ++i) inv_ls2[i] = m.inv_ls2[i];
    for (int d = 0; d < m.n_s; ++d) {
        if (outputscale) outputscale[d] = m.outputscale[d];
        if (noise) noise[d] = m.noise[d];
    }
}

// The constants of the kernel value k(x, z) = exp2(sum_j k_nh_ils2 (x_j - z_j)^2 + k_log_os): -inv_ls2 / 2 and
// log(outputscale), scaled by kExpScale (and unscaled, where the argument keeps those too).
inline void exp_hyper(const sx_gp_model& m, double* k_nh_ils2, double* k_log_os, double* nh_ils2 = nullptr,
                      double* log_os = nullptr) {
    for (int i = 0; i < m.n_s * (m.n_s + m.n_u); ++i) {
        const double nh = -0.5 * m.inv_ls2[i];
        if (nh_ils2) nh_ils2[i] = nh;
        k_nh_ils2[i] = nh * kExpScale;
    }
    for (int d = 0; d < m.n_s; ++d) {
        const double l = std::log(m.outputscale[d]);
        if (log_os) log_os[d] = l;
        k_log_os[d] = l * kExpScale;
    }
}

template <int NS, int NU>
static GpConst<NS, NS + NU> make_gp_const(const sx_gp_model* m, int nw) {
    GpConst<NS, NS + NU> gc;
    copy_hyper(*m, gc.inv_ls2, gc.outputscale, gc.noise);
    exp_hyper(*m, gc.k_nh_ils2, gc.k_log_os, gc.nh_ils2, gc.log_os);
    gc.x_train = m->x_train;
    gc.a_pack = m->a_pack;
    gc.stage_tab = reinterpret_cast<const int4*>(m->stage_tab);
    gc.n_train = m->n_train;
    gc.n_pad = m->n_pad;
    gc.stage_cap = gp_stage_cap(NS, m->n_pad, nw);
    gc.stage_cap_one = gp_stage_cap(1, m->n_pad, nw);
    return gc;
}

template <int NS, int NU>
static bool make_reach_const(const sx_env* env, ReachConst<NS, NU>& rc) {
    for (int i = 0; i < NS * NS; ++i) rc.a[i] = env->a[i];
    for (int i = 0; i < NS * NU; ++i) rc.b[i] = env->b[i];
    for (int i = 0; i < NU * NS; ++i) rc.kfb[i] = env->k_fb[i];
    for (int i = 0; i < NS; ++i) {
        rc.l_mu[i] = env->l_mu[i];
        rc.l_sigma[i] = env->l_sigma[i];
    }
    rc.beta = env->beta;
    // B = I + kfb^T kfb is SPD; lower Cholesky on the host
    double B[NS][NS];
    for (int i = 0; i < NS; ++i)
        for (int j = 0; j < NS; ++j) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int c = 0; c < NU; ++c) s += env->k_fb[c * NS + i] * env->k_fb[c * NS + j];
            B[i][j] = s;
        }
    for (int i = 0; i < NS * NS; ++i) rc.cholB[i] = 0.0;
    for (int j = 0; j < NS; ++j) {
        double s = B[j][j];
        for (int k = 0; k < j; ++k) s -= rc.cholB[j * NS + k] * rc.cholB[j * NS + k];
        if (!(s > 0.0)) return false;
        const double ljj = std::sqrt(s);
        rc.cholB[j * NS + j] = ljj;
        for (int i = j + 1; i < NS; ++i) {
            double t = B[i][j];
            for (int k = 0; k < j; ++k) t -= rc.cholB[i * NS + k] * rc.cholB[j * NS + k];
            rc.cholB[i * NS + j] = t / ljj;
        }
    }
    return true;
}

template <int NS, int NU>
static void make_cost_const(const sx_env* env, CostConst<SX_MAX_M, NS, NU>& cc) {
    std::memset(&cc, 0, sizeof(cc));
    for (int r = 0; r < env->m; ++r) {
        for (int i = 0; i < NS; ++i) cc.h_mat[r * NS + i] = env->h_mat[r * NS + i];
        cc.h_vec[r] = env->h_vec[r];
    }
    for (int c = 0; c < NU; ++c) {
        cc.u_min[c] = env->u_min[c];
        cc.u_max[c] = env->u_max[c];
    }
    for (int i = 0; i < NS; ++i) {
        cc.w_abs[i] = env->obj_w_abs[i];
        cc.target[i] = env->obj_target[i];
        cc.w_lin[i] = env->obj_w_lin[i];
    }
    cc.m = env->m;
    cc.obj_mode = env->obj_mode;
    cc.con_mode = env->con_mode;
}

// The reachability and cost constants of a rollout launch: SX_ERR_UNSUPPORTED for a constraint count outside
// 1 .. SX_MAX_M, SX_ERR_ARG where B = I + kfb^T kfb has no Cholesky factor
template <int NS, int NU>
static int env_consts(const sx_env* env, ReachConst<NS, NU>& rc, CostConst<SX_MAX_M, NS, NU>& cc) {
    if (env->m <= 0 || env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    if (!make_reach_const<NS, NU>(env, rc)) return SX_ERR_ARG;
    make_cost_const<NS, NU>(env, cc);
    return SX_OK;
}

// The arguments every rollout entry checks alike, before anything touches the device (SX_ERR_ARG where false): env, the
// buffers, E, P, H, and what the actions come from -- with noise, the sampling distribution (mean, std) or, in the elite
// row form (rp.elite_rows), k elite rows and both or neither of the refit's outputs.
template <typename Ptrs>
static bool rollout_args_ok(const sx_env* env, const Ptrs& rp) {
    if (!env || !rp.x0 || !rp.actions || !rp.obj_cost || !rp.con_cost || !rp.status) return false;
    if (rp.E <= 0 || rp.P <= 0 || rp.H <= 0) return false;
    if constexpr (std::is_same<Ptrs, RolloutPtrs>::value) {
        if (rp.elite_rows) return rp.noise && rp.elite_k > 0 && (rp.mean_out == nullptr) == (rp.std_out == nullptr);
    }
    return !rp.noise || (rp.mean && rp.std);
}

// sx_gp_model_table / sx_feat_model_table / sx_mlp_model_table: one host -> device copy of the E entries on `stream`,
// waited for
template <typename C>
static int copy_model_table(const std::vector<C>& host, void* table, hipStream_t stream) {
    if (hipMemcpyAsync(table, host.data(), host.size() * sizeof(C), hipMemcpyHostToDevice, stream) != hipSuccess)
        return SX_ERR_LAUNCH;
    // (the copy reads `host`, which ends with the caller)
    return hipStreamSynchronize(stream) == hipSuccess ? SX_OK : SX_ERR_LAUNCH;
}

}  // namespace sx
