// The exact-GP warm path: the kernels of sx_fit.hpp and sx_fit_blocked.hpp, their launch sequences and the entries
// sx_gp_pack_sizes, sx_gp_fit[_table|_multi], sx_gp_mll_grad[_multi], sx_gp_predict_var_jac, sx_gp_predict_mean_hessian and
// sx_gp_pack.  Every argument check of an entry answers before its first HIP call (tests/test_gp_warm_host.py,
// tests/test_multi_fit_host.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/sx_amd.h"
#include "sx_fit.hpp"
#include "sx_fit_blocked.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"

namespace sx {

// The model shapes of the warm path.  wide: n_s + n_u <= SX_MAX_D, the kept-column model of a junk-dimension rollout
// (sx_gp_pack_sizes, sx_gp_fit, sx_gp_pack and the table / multi entries); else n_u <= SX_MAX_NU.
static bool gp_shape_ok(int n_s, int n_u, int n_train, bool wide) {
    if (n_s <= 0 || n_s > SX_MAX_NS || n_u <= 0 || n_train <= 0) return false;
    return n_u <= (wide ? SX_MAX_D - n_s : SX_MAX_NU);
}
static bool gp_shape_ok(const sx_gp_model& m, bool wide) { return gp_shape_ok(m.n_s, m.n_u, m.n_train, wide); }

// the one-workgroup fit's panel width for N points (sx_gp_fit): as wide as the LDS left beside the static arrays allows
// (vec 32 KB + red 8 KB), at most 32
static int fit_panel_cols(int n) {
    const size_t lds_budget = 112 * 1024;
    const int nb = (int)(lds_budget / (sizeof(double) * (size_t)n));
    return nb > 32 ? 32 : (nb < 1 ? 1 : nb);
}
// the one-workgroup kernel serves N <= kBlockedFitMinN with 32 panel columns: its dynamic LDS needs no grant
static_assert(kBlockedFitMinN * 32 * sizeof(double) < 64 * 1024, "gp_fit_kernel's panel must stay below 64 KB of LDS");

static int blocks_of(int n) { return (n + kFB - 1) / kFB; }

// The blocked factorisation (sx_fit_blocked.hpp) of one model (MM = false: `arg` is its BlockedFitArgs, rows = n_s) or of
// the blocked problems of a table (MM = true: `arg` is the table, rows = E n_s): nb block columns -- the most of any
// problem -- and alpha_lds bytes, a double per training point of the largest problem, for fit_alpha_logdet_kernel.
template <bool MM>
static void launch_blocked_fit(const typename FitArg<BlockedFitArgs, MM>::type& arg, int nb, int rows, size_t alpha_lds,
                               hipStream_t s) {
    hipLaunchKernelGGL(fit_kmat_kernel<MM>, dim3(nb, nb, rows), dim3(kFThreads), 0, s, arg);
    for (int p = 0; p < nb; ++p) {
        hipLaunchKernelGGL(fit_potrf_diag_kernel<MM>, dim3(rows), dim3(kFThreads), 0, s, arg, p);
        const int m = nb - p - 1;
        if (m > 0) {
            hipLaunchKernelGGL(fit_trsm_kernel<MM>, dim3(m, rows), dim3(kFThreads), 0, s, arg, p);
            hipLaunchKernelGGL(fit_syrk_kernel<MM>, dim3(m, m, rows), dim3(kFThreads), 0, s, arg, p);
        }
    }
    hipLaunchKernelGGL(fit_trtri_kernel<MM>, dim3(nb, rows, kFB / 16), dim3(kFThreads), 0, s, arg);
    hipLaunchKernelGGL(fit_alpha_logdet_kernel<MM>, dim3(rows), dim3(1024), alpha_lds, s, arg);
}

// The blocked MLL and gradient, `arg`, nb and rows as above
template <bool MM>
static void launch_blocked_mll(const typename FitArg<BlockedMllArgs, MM>::type& arg, int nb, int rows, hipStream_t s) {
    hipLaunchKernelGGL(mll_pairs_kernel<MM>, dim3(nb, nb, rows), dim3(kFThreads), 0, s, arg);
    hipLaunchKernelGGL(mll_reduce_kernel<MM>, dim3(rows), dim3(256), 0, s, arg);
}

// ---- E exact GPs' fit and MLL gradient in one launch sequence (sx_gp_fit_table, sx_gp_fit_multi, sx_gp_mll_grad_multi)

// the E models of a multi-model fit: one (n_s, n_u), a training set each; SX_OK, or the code to answer
static int fit_models_check(const sx_gp_model* models, int E) {
    if (!models || E <= 0 || !gp_shape_ok(models[0], true)) return SX_ERR_ARG;
    const int ns = models[0].n_s, nu = models[0].n_u;
    for (int e = 0; e < E; ++e)
        if (models[e].n_s != ns || models[e].n_u != nu || models[e].n_train <= 0 || !models[e].x_train) return SX_ERR_ARG;
    for (int e = 0; e < E; ++e)
        if (models[e].n_train > kFitMaxN) return SX_ERR_UNSUPPORTED;
    return SX_OK;
}

// what one multi-model launch sequence needs: the largest block count of the blocked problems (0: none), the largest N of
// the one-workgroup problems (0: none), the largest N of all
struct FitMultiPlan {
    int nb_max = 0, small_n_max = 0, n_max = 0;
};
static FitMultiPlan plan_fit_multi(const sx_gp_model* models, int E) {
    FitMultiPlan plan;
    for (int e = 0; e < E; ++e) {
        const int n = models[e].n_train;
        plan.n_max = std::max(plan.n_max, n);
        if (n > kBlockedFitMinN)
            plan.nb_max = std::max(plan.nb_max, blocks_of(n));
        else
            plan.small_n_max = std::max(plan.small_n_max, n);
    }
    return plan;
}

}  // namespace sx

extern "C" {

int sx_gp_pack_sizes(int n_s, int n_u, int n_train, int64_t* a_doubles, int64_t* tab_ints) {
    if (!sx::gp_shape_ok(n_s, n_u, n_train, true)) return SX_ERR_ARG;
    const int n_pad = sx::gp_n_pad(n_train, n_s + n_u);
    if (a_doubles) *a_doubles = sx::a_pack_doubles(n_s, n_pad);
    if (tab_ints) *tab_ints = sx::gp_stage_tab_ints(n_s, n_pad, SX_WAVES);
    return SX_OK;
}

int sx_gp_fit(const sx_gp_model* model, const double* y_train, double* work, double* linv, double* alpha,
              double* logdet, int32_t* status, void* stream) {
    if (!model || !model->x_train || !y_train || !work || !linv || !alpha || !logdet || !status) return SX_ERR_ARG;
    if (!sx::gp_shape_ok(*model, true)) return SX_ERR_ARG;
    if (model->n_train > sx::kFitMaxN) return SX_ERR_UNSUPPORTED;
    auto fill = [&](auto& a) {   // what FitArgs and BlockedFitArgs share
        std::memset(&a, 0, sizeof(a));
        sx::copy_hyper(*model, a.inv_ls2, a.outputscale, a.noise);
        a.x = model->x_train;
        a.y = y_train;
        a.lmat = work;
        a.linv = linv;
        a.alpha = alpha;
        a.logdet = logdet;
        a.status = status;
        a.n = model->n_train;
        a.D = model->n_s + model->n_u;
        a.n_s = model->n_s;
    };
    if (model->n_train > sx::kBlockedFitMinN) {
        sx::BlockedFitArgs ba;
        fill(ba);
        ba.nblk = sx::blocks_of(ba.n);
        sx::launch_blocked_fit<false>(ba, ba.nblk, ba.n_s, sizeof(double) * (size_t)ba.n, (hipStream_t)stream);
        return sx::check_launch();
    }
    sx::FitArgs fa;
    fill(fa);
    fa.panel_cols = sx::fit_panel_cols(fa.n);
    const size_t lds = sizeof(double) * (size_t)fa.n * fa.panel_cols;
    hipLaunchKernelGGL(sx::gp_fit_kernel<false>, dim3(model->n_s), dim3(sx::kFitThreads), lds, (hipStream_t)stream, fa);
    return sx::check_launch();
}

int sx_gp_mll_grad(const sx_gp_model* model, const double* y_train, const double* linv, const double* alpha,
                   const double* logdet, double* work, double* mll, double* grad, void* stream) {
    if (!model || !model->x_train || !y_train || !linv || !alpha || !logdet || !work || !mll || !grad) return SX_ERR_ARG;
    if (!sx::gp_shape_ok(*model, false)) return SX_ERR_ARG;
    auto fill = [&](auto& a) {   // what MllArgs and BlockedMllArgs share
        std::memset(&a, 0, sizeof(a));
        a.x = model->x_train;
        a.y = y_train;
        a.linv = linv;
        a.alpha = alpha;
        a.logdet = logdet;
        a.mll = mll;
        a.grad = grad;
        a.n = model->n_train;
        a.D = model->n_s + model->n_u;
        a.n_s = model->n_s;
    };
    if (model->n_train > sx::kBlockedFitMinN) {
        sx::BlockedMllArgs ba;
        fill(ba);
        sx::copy_hyper(*model, ba.inv_ls2, ba.outputscale);
        ba.scratch = work;
        ba.nblk = sx::blocks_of(ba.n);
        sx::launch_blocked_mll<false>(ba, ba.nblk, ba.n_s, (hipStream_t)stream);
        return sx::check_launch();
    }
    sx::MllArgs ma;
    fill(ma);
    sx::copy_hyper(*model, ma.inv_ls2, ma.outputscale, ma.noise);
    hipLaunchKernelGGL(sx::gp_mll_grad_kernel<false>, dim3(model->n_s), dim3(sx::kFitThreads), 0, (hipStream_t)stream, ma);
    return sx::check_launch();
}

int64_t sx_gp_fit_table_bytes(int E) {
    if (E <= 0) return -1;
    return (int64_t)E * (int64_t)sizeof(sx::GpFitEntry);
}

int sx_gp_fit_table(const sx_gp_model* models, int E, const double* const* y_train, double* const* work,
                    double* const* linv, double* const* alpha, double* const* logdet, int32_t* status, double* mll,
                    double* grad, void* table) {
    if (!y_train || !work || !linv || !alpha || !logdet || !status || !mll || !grad || !table) return SX_ERR_ARG;
    if (int r = sx::fit_models_check(models, E)) return r;
    for (int e = 0; e < E; ++e)
        if (!y_train[e] || !work[e] || !linv[e] || !alpha[e] || !logdet[e]) return SX_ERR_ARG;
    const int ns = models[0].n_s, D = ns + models[0].n_u;
    sx::GpFitEntry* out = static_cast<sx::GpFitEntry*>(table);
    for (int e = 0; e < E; ++e) {
        const sx_gp_model& m = models[e];
        sx::GpFitEntry t;
        std::memset(&t, 0, sizeof(t));
        sx::copy_hyper(m, t.inv_ls2, t.outputscale, t.noise);
        t.x = m.x_train;
        t.y = y_train[e];
        t.lmat = t.scratch = work[e];
        t.linv = linv[e];
        t.alpha = alpha[e];
        t.logdet = logdet[e];
        t.status = status + e;
        t.mll = mll + (size_t)e * ns;
        t.grad = grad + (size_t)e * ns * (D + 2);
        t.n = m.n_train;
        t.D = D;
        t.n_s = ns;
        t.nblk = m.n_train > sx::kBlockedFitMinN ? sx::blocks_of(m.n_train) : 0;
        t.panel_cols = sx::fit_panel_cols(m.n_train);
        std::memcpy(out + e, &t, sizeof(t));
    }
    return SX_OK;
}

int sx_gp_fit_multi(const sx_gp_model* models, int E, const void* table, void* stream) {
    if (!table) return SX_ERR_ARG;
    if (int r = sx::fit_models_check(models, E)) return r;
    const sx::FitMultiPlan plan = sx::plan_fit_multi(models, E);
    const sx::GpFitEntry* tab = static_cast<const sx::GpFitEntry*>(table);
    hipStream_t s = (hipStream_t)stream;
    const int rows = E * models[0].n_s;   // the (problem, output) grid dimension
    if (plan.small_n_max > 0) {
        // N <= 96: the panel is 32 columns wide for every such problem, at most 24 KB of LDS
        const size_t lds = sizeof(double) * (size_t)plan.small_n_max * sx::fit_panel_cols(plan.small_n_max);
        hipLaunchKernelGGL(sx::gp_fit_kernel<true>, dim3(rows), dim3(sx::kFitThreads), lds, s, tab);
    }
    if (plan.nb_max > 0) sx::launch_blocked_fit<true>(tab, plan.nb_max, rows, sizeof(double) * (size_t)plan.n_max, s);
    return sx::check_launch();
}

int sx_gp_mll_grad_multi(const sx_gp_model* models, int E, const void* table, void* stream) {
    if (!table) return SX_ERR_ARG;
    if (int r = sx::fit_models_check(models, E)) return r;
    const sx::FitMultiPlan plan = sx::plan_fit_multi(models, E);
    const sx::GpFitEntry* tab = static_cast<const sx::GpFitEntry*>(table);
    hipStream_t s = (hipStream_t)stream;
    const int rows = E * models[0].n_s;
    if (plan.small_n_max > 0)
        hipLaunchKernelGGL(sx::gp_mll_grad_kernel<true>, dim3(rows), dim3(sx::kFitThreads), 0, s, tab);
    if (plan.nb_max > 0) sx::launch_blocked_mll<true>(tab, plan.nb_max, rows, s);
    return sx::check_launch();
}

int sx_gp_predict_var_jac(const sx_gp_model* model, const double* linv, const double* z, int P, double* jac_var,
                          void* stream) {
    if (!model || P < 0) return SX_ERR_ARG;
    if (P == 0) return SX_OK;
    if (!model->x_train || !linv || !z || !jac_var) return SX_ERR_ARG;
    if (!sx::gp_shape_ok(*model, false)) return SX_ERR_ARG;
    const size_t lds = 2 * (size_t)model->n_train * sizeof(double);
    if (lds > 128 * 1024) return SX_ERR_UNSUPPORTED;  // N <= 8192
    sx::VarJacArgs va;
    std::memset(&va, 0, sizeof(va));
    sx::copy_hyper(*model, va.inv_ls2, va.outputscale);
    va.x = model->x_train;
    va.linv = linv;
    va.z = z;
    va.jac_var = jac_var;
    va.n = model->n_train;
    va.D = model->n_s + model->n_u;
    va.n_s = model->n_s;
    if (int r = sx::allow_lds(sx::gp_var_jac_kernel, lds)) return r;
    hipLaunchKernelGGL(sx::gp_var_jac_kernel, dim3(P, model->n_s), dim3(256), lds, (hipStream_t)stream, va);
    return sx::check_launch();
}

int sx_gp_predict_mean_hessian(const sx_gp_model* model, const double* alpha, const double* z, int P, double* hess,
                               void* stream) {
    if (!model || P < 0) return SX_ERR_ARG;
    if (P == 0) return SX_OK;
    if (!model->x_train || !alpha || !z || !hess) return SX_ERR_ARG;
    if (!sx::gp_shape_ok(*model, false)) return SX_ERR_ARG;
    sx::MeanHessArgs ha;
    std::memset(&ha, 0, sizeof(ha));
    sx::copy_hyper(*model, ha.inv_ls2, ha.outputscale);
    ha.x = model->x_train;
    ha.alpha = alpha;
    ha.z = z;
    ha.hess = hess;
    ha.n = model->n_train;
    ha.D = model->n_s + model->n_u;
    ha.n_s = model->n_s;
    hipLaunchKernelGGL(sx::gp_mean_hessian_kernel, dim3(P, model->n_s), dim3(256), 0, (hipStream_t)stream, ha);
    return sx::check_launch();
}

int sx_gp_pack(sx_gp_model* model, const double* linv, const double* alpha, void* stream) {
    if (!model || !linv || !alpha || !model->x_train || !model->a_pack || !model->stage_tab) return SX_ERR_ARG;
    if (!sx::gp_shape_ok(*model, true)) return SX_ERR_ARG;
    const int D = model->n_s + model->n_u;
    model->n_pad = sx::gp_n_pad(model->n_train, D);
    const bool has_tab = model->n_pad <= 1024;  // beyond that only the large-training-set path runs (no stage table)
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = sx::a_pack_doubles(model->n_s, model->n_pad);
    int grid = (int)((total + 255) / 256);
    if (grid > 8192) grid = 8192;
    sx::PackArgs<SX_MAX_NS, SX_MAX_D> args;
    std::memset(&args, 0, sizeof(args));
    sx::copy_hyper(*model, args.inv_ls2);
    hipLaunchKernelGGL(sx::pack_a_kernel, dim3(grid), dim3(256), 0, s, linv, alpha, model->x_train, args, model->n_s, D,
                       model->n_train, model->n_pad, const_cast<double*>(model->a_pack));
    if (has_tab)
        hipLaunchKernelGGL(sx::build_stage_tab_kernel, dim3(1), dim3(64), 0, s,
                           reinterpret_cast<int4*>(const_cast<int32_t*>(model->stage_tab)), model->n_s, model->n_train,
                           model->n_pad, SX_WAVES, sx::gp_stage_cap(model->n_s, model->n_pad, SX_WAVES),
                           sx::gp_stage_cap(1, model->n_pad, SX_WAVES));
    return sx::check_launch();
}

}  // extern "C"
