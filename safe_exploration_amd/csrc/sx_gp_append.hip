// sx_gp_append, sx_gp_append_workspace_bytes and the lockstep form sx_gp_append_table[_bytes] / sx_gp_append_multi: the kernels
// of sx_gp_append.hpp and their launch sequence.  Every argument check answers before the first HIP call
// (tests/test_gp_append_host.py, tests/test_gp_append_multi_host.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/sx_amd.h"
#include "sx_gp_append.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"

namespace sx {

constexpr int kAppendMaxRows = 65535;   // E n_s: the (problem, output) dimension of a grid (its y-extent)

// a model shape sx_gp_fit takes (the wide split of the inputs included)
static bool append_shape_ok(const sx_gp_model& m) {
    return m.n_s > 0 && m.n_s <= SX_MAX_NS && m.n_u > 0 && m.n_u <= SX_MAX_D - m.n_s && m.n_train > 0;
}

// `a` for n_old fitted rows and k new ones of `model`, the workspace cut up; the caller sets the buffers
static void append_fill(AppendArgs& a, const sx_gp_model& model, int n_old, int k, void* workspace) {
    const int n_s = model.n_s;
    copy_hyper(model, a.inv_ls2, a.outputscale, a.noise);
    a.x = model.x_train;
    a.n = n_old;
    a.k = k;
    a.D = n_s + model.n_u;
    a.n_s = n_s;
    a.nblk = append_blocks(n_old);
    a.nparts = append_parts(n_old);
    double* w = static_cast<double*>(workspace);
    a.kc = w;
    w += (size_t)n_s * n_old * kAT;
    a.b = w;
    w += (size_t)n_s * n_old * kAT;
    a.kcc = w;
    w += (size_t)n_s * kAT * kAT;
    a.ws = w;
    w += (size_t)n_s * kAT * kAT;
    a.btb = w;
    w += (size_t)n_s * a.nparts * kAT * kAT;
    a.tpart = w;
}

// The six launches: of one model (MM = false: `arg` is its AppendArgs, rows = n_s) or of the problems of a table (MM = true:
// rows = E n_s); n_max fitted rows in the largest problem, which sizes every x-extent.
template <bool MM>
static void launch_append(const typename AppendArg<MM>::type& arg, int n_max, int k, int rows, hipStream_t s) {
    const dim3 block(kAThreads);
    const int nblk = append_blocks(n_max), nparts = append_parts(n_max);
    const int kc_grid = (int)(((int64_t)(n_max + k) * kAT + kAThreads - 1) / kAThreads);
    hipLaunchKernelGGL(append_kc_kernel<MM>, dim3(kc_grid, rows), block, 0, s, arg);
    hipLaunchKernelGGL(append_b_kernel<MM>, dim3(nblk, rows), block, 0, s, arg);
    hipLaunchKernelGGL(append_btb_kernel<MM>, dim3(nparts, rows), block, 0, s, arg);
    hipLaunchKernelGGL(append_schur_kernel<MM>, dim3(rows), block, 0, s, arg);
    hipLaunchKernelGGL(append_wbot_kernel<MM>, dim3(nblk, rows), block, 0, s, arg);
    hipLaunchKernelGGL(append_copy_alpha_kernel<MM>, dim3(append_copy_grid(n_max), rows), block, 0, s, arg);
}

// the E models of a lockstep append of k rows each: one (n_s, n_u), N_e = n_train - k >= 1; SX_OK, or SX_ERR_ARG
static int append_models_check(const sx_gp_model* models, int E, int k) {
    if (!models || E <= 0 || k < 1 || k > kAppendMaxK || !append_shape_ok(models[0])) return SX_ERR_ARG;
    for (int e = 0; e < E; ++e) {
        const sx_gp_model& m = models[e];
        if (m.n_s != models[0].n_s || m.n_u != models[0].n_u || !m.x_train || m.n_train <= 0 || m.n_train - k < 1)
            return SX_ERR_ARG;
    }
    return SX_OK;
}
// ... and what is beyond the kernels' limits (after every argument error)
static int append_models_supported(const sx_gp_model* models, int E) {
    for (int e = 0; e < E; ++e)
        if (models[e].n_train > kAppendMaxN) return SX_ERR_UNSUPPORTED;
    if ((int64_t)E * models[0].n_s > kAppendMaxRows) return SX_ERR_UNSUPPORTED;
    return SX_OK;
}

}  // namespace sx

extern "C" {

int64_t sx_gp_append_workspace_bytes(int n_s, int n_train, int k) {
    if (n_s <= 0 || n_s > SX_MAX_NS || k < 1 || k > sx::kAppendMaxK || n_train - k < 1 || n_train > sx::kAppendMaxN) return -1;
    return sx::append_workspace_doubles(n_s, n_train - k) * (int64_t)sizeof(double);
}

int sx_gp_append(const sx_gp_model* model, int n_old, const double* y_train, const double* linv_old, const double* alpha_old,
                 const double* logdet_old, double* linv, double* alpha, double* logdet, int32_t* status, void* workspace,
                 int64_t workspace_bytes, void* stream) {
    if (!model || !model->x_train || !y_train || !linv_old || !alpha_old || !logdet_old || !linv || !alpha || !logdet ||
        !status || !workspace)
        return SX_ERR_ARG;
    const int n_s = model->n_s, n2 = model->n_train;
    if (!sx::append_shape_ok(*model)) return SX_ERR_ARG;
    if (n_old < 1) return SX_ERR_ARG;
    const int k = n2 - n_old;
    if (k < 1 || k > sx::kAppendMaxK) return SX_ERR_ARG;
    if (workspace_bytes < sx::append_workspace_doubles(n_s, n_old) * (int64_t)sizeof(double)) return SX_ERR_ARG;
    if (n2 > sx::kAppendMaxN) return SX_ERR_UNSUPPORTED;

    sx::AppendArgs a;
    std::memset(&a, 0, sizeof(a));
    sx::append_fill(a, *model, n_old, k, workspace);
    a.y = y_train;
    a.w_old = linv_old;
    a.alpha_old = alpha_old;
    a.logdet_old = logdet_old;
    a.w_new = linv;
    a.alpha = alpha;
    a.logdet = logdet;
    a.status = status;
    sx::launch_append<false>(a, n_old, k, n_s, (hipStream_t)stream);
    return sx::check_launch();
}

int64_t sx_gp_append_table_bytes(int E) {
    if (E <= 0) return -1;
    return (int64_t)E * (int64_t)sizeof(sx::AppendEntry);
}

int sx_gp_append_table(const sx_gp_model* models, int E, int k, const double* const* y_train, const double* const* linv_old,
                       const double* const* alpha_old, const double* const* logdet_old, double* const* linv,
                       double* const* alpha, double* const* logdet, int32_t* status, void* const* workspace,
                       const int64_t* workspace_bytes, void* table) {
    if (!y_train || !linv_old || !alpha_old || !logdet_old || !linv || !alpha || !logdet || !status || !workspace ||
        !workspace_bytes || !table)
        return SX_ERR_ARG;
    if (int r = sx::append_models_check(models, E, k)) return r;
    const int n_s = models[0].n_s;
    for (int e = 0; e < E; ++e) {
        if (!y_train[e] || !linv_old[e] || !alpha_old[e] || !logdet_old[e] || !linv[e] || !alpha[e] || !logdet[e] ||
            !workspace[e])
            return SX_ERR_ARG;
        if (workspace_bytes[e] < sx::append_workspace_doubles(n_s, models[e].n_train - k) * (int64_t)sizeof(double))
            return SX_ERR_ARG;
    }
    if (int r = sx::append_models_supported(models, E)) return r;
    sx::AppendEntry* out = static_cast<sx::AppendEntry*>(table);
    for (int e = 0; e < E; ++e) {
        const int n_old = models[e].n_train - k;
        sx::AppendEntry t;
        std::memset(&t, 0, sizeof(t));
        sx::append_fill(t, models[e], n_old, k, workspace[e]);
        t.y = y_train[e];
        t.w_old = linv_old[e];
        t.alpha_old = alpha_old[e];
        t.logdet_old = logdet_old[e];
        t.w_new = linv[e];
        t.alpha = alpha[e];
        t.logdet = logdet[e];
        t.status = status + e;
        t.copy_grid = sx::append_copy_grid(n_old);
        std::memcpy(out + e, &t, sizeof(t));
    }
    return SX_OK;
}

int sx_gp_append_multi(const sx_gp_model* models, int E, int k, const void* table, void* stream) {
    if (!table) return SX_ERR_ARG;
    if (int r = sx::append_models_check(models, E, k)) return r;
    if (int r = sx::append_models_supported(models, E)) return r;
    int n_max = 0;
    for (int e = 0; e < E; ++e) n_max = std::max(n_max, models[e].n_train - k);
    sx::launch_append<true>(static_cast<const sx::AppendEntry*>(table), n_max, k, E * models[0].n_s, (hipStream_t)stream);
    return sx::check_launch();
}

}  // extern "C"
