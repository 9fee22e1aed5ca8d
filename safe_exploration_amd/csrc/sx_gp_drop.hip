// sx_gp_drop, sx_gp_drop_workspace_bytes and the lockstep form sx_gp_drop_table[_bytes] / sx_gp_drop_multi: the kernels of
// sx_gp_drop.hpp and their launch sequence.  Every argument check answers before the first HIP call
// (tests/test_gp_drop_host.py, tests/test_gp_drop_multi_host.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/sx_amd.h"
#include "sx_gp_drop.hpp"
#include "sx_launch.hpp"

namespace sx {

constexpr int kDropMaxRows = 65535;   // E n_s: the (problem, output) dimension of a grid (its y-extent)

// the table and the main kernel for KB stages
template <int KB, bool MM>
static void launch_stages(const typename DropArg<MM>::type& arg, int blocks, int rows, hipStream_t s) {
    hipLaunchKernelGGL((drop_table_kernel<KB, MM>), dim3(rows), dim3(kDT), 0, s, arg);
    hipLaunchKernelGGL((drop_main_kernel<KB, MM>), dim3(blocks, rows), dim3(kDT), 0, s, arg);
}

// The seven launches: of one model (MM = false: `arg` is its DropArgs, rows = n_s) or of the problems of a table (MM = true:
// rows = E n_s); m_max kept rows in the largest problem, which sizes every x-extent of the grids that have one.
template <bool MM>
static void launch_drop(const typename DropArg<MM>::type& arg, int m_max, int k, int rows, hipStream_t s) {
    const int blocks = drop_blocks(m_max);
    hipLaunchKernelGGL(drop_l11_kernel<MM>, dim3(rows), dim3(kDThreads), 0, s, arg);
    hipLaunchKernelGGL(drop_v_kernel<MM>, dim3(blocks, rows), dim3(kDThreads), 0, s, arg);
    switch (drop_stages(k)) {
        case 1: launch_stages<1, MM>(arg, blocks, rows, s); break;
        case 2: launch_stages<2, MM>(arg, blocks, rows, s); break;
        case 4: launch_stages<4, MM>(arg, blocks, rows, s); break;
        case 8: launch_stages<8, MM>(arg, blocks, rows, s); break;
        case 16: launch_stages<16, MM>(arg, blocks, rows, s); break;
        case 32: launch_stages<32, MM>(arg, blocks, rows, s); break;
        default: launch_stages<64, MM>(arg, blocks, rows, s); break;
    }
    hipLaunchKernelGGL(drop_t_kernel<MM>, dim3(drop_blocks4(m_max), rows), dim3(kDThreads), 0, s, arg);
    hipLaunchKernelGGL(drop_alpha_kernel<MM>, dim3(blocks, rows), dim3(kDThreads), 0, s, arg);
    hipLaunchKernelGGL(drop_logdet_kernel<MM>, dim3(rows), dim3(kDThreads), 0, s, arg);
}

// `a` for n_old fitted rows of which the first k go, the workspace cut up; the caller sets the buffers
static void drop_fill(DropArgs& a, int n_s, int n_old, int k, void* workspace) {
    const int m = n_old - k;
    a.n = n_old;
    a.k = k;
    a.m = m;
    a.n_s = n_s;
    double* w = static_cast<double*>(workspace);
    a.l11 = w;
    w += (size_t)n_s * kDT * kDT;
    a.v = w;
    w += (size_t)n_s * m * kDT;
    a.tab = w;
    w += (size_t)n_s * m * drop_stages(k) * 3;
    a.t = w;
}

// the E problems of a lockstep drop of k rows each: N_e - k >= 1; SX_OK, or SX_ERR_ARG
static int drop_problems_check(int n_s, int E, int k, const int* n_old) {
    if (!n_old || E <= 0 || n_s <= 0 || n_s > SX_MAX_NS || k < 1 || k > kDropMaxK) return SX_ERR_ARG;
    for (int e = 0; e < E; ++e)
        if (n_old[e] < 1 || n_old[e] - k < 1) return SX_ERR_ARG;
    return SX_OK;
}
// ... and what is beyond the kernels' limits (after every argument error)
static int drop_problems_supported(int n_s, int E, const int* n_old) {
    for (int e = 0; e < E; ++e)
        if (n_old[e] > kDropMaxN) return SX_ERR_UNSUPPORTED;
    if ((int64_t)E * n_s > kDropMaxRows) return SX_ERR_UNSUPPORTED;
    return SX_OK;
}

}  // namespace sx

extern "C" {

int64_t sx_gp_drop_workspace_bytes(int n_s, int n_old, int k) {
    if (n_s <= 0 || n_s > SX_MAX_NS || k < 1 || k > sx::kDropMaxK || n_old - k < 1 || n_old > sx::kDropMaxN) return -1;
    return sx::drop_workspace_doubles(n_s, n_old - k, k) * (int64_t)sizeof(double);
}

int sx_gp_drop(int n_s, int n_old, int k, const double* y_train, const double* linv_old, double* linv, double* alpha,
               double* logdet, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!y_train || !linv_old || !linv || !alpha || !logdet || !status || !workspace) return SX_ERR_ARG;
    if (n_s <= 0 || n_s > SX_MAX_NS || k < 1 || k > sx::kDropMaxK || n_old < 1 || n_old - k < 1) return SX_ERR_ARG;
    const int m = n_old - k;
    // (n_old beyond the limit: the size the workspace is measured against is still that of (n_s, m, k))
    if (workspace_bytes < sx::drop_workspace_doubles(n_s, m, k) * (int64_t)sizeof(double)) return SX_ERR_ARG;
    if (n_old > sx::kDropMaxN) return SX_ERR_UNSUPPORTED;

    sx::DropArgs a;
    std::memset(&a, 0, sizeof(a));
    sx::drop_fill(a, n_s, n_old, k, workspace);
    a.y = y_train;
    a.w_old = linv_old;
    a.w_new = linv;
    a.alpha = alpha;
    a.logdet = logdet;
    a.status = status;
    sx::launch_drop<false>(a, m, k, n_s, (hipStream_t)stream);
    return sx::check_launch();
}

int64_t sx_gp_drop_table_bytes(int E) {
    if (E <= 0) return -1;
    return (int64_t)E * (int64_t)sizeof(sx::DropEntry);
}

int sx_gp_drop_table(int n_s, int E, int k, const int* n_old, const double* const* y_train, const double* const* linv_old,
                     double* const* linv, double* const* alpha, double* const* logdet, int32_t* status,
                     void* const* workspace, const int64_t* workspace_bytes, void* table) {
    if (!y_train || !linv_old || !linv || !alpha || !logdet || !status || !workspace || !workspace_bytes || !table)
        return SX_ERR_ARG;
    if (int r = sx::drop_problems_check(n_s, E, k, n_old)) return r;
    for (int e = 0; e < E; ++e) {
        if (!y_train[e] || !linv_old[e] || !linv[e] || !alpha[e] || !logdet[e] || !workspace[e]) return SX_ERR_ARG;
        // (n_old beyond the limit: the size the workspace is measured against is still that of (n_s, m, k))
        if (workspace_bytes[e] < sx::drop_workspace_doubles(n_s, n_old[e] - k, k) * (int64_t)sizeof(double)) return SX_ERR_ARG;
    }
    if (int r = sx::drop_problems_supported(n_s, E, n_old)) return r;
    sx::DropEntry* out = static_cast<sx::DropEntry*>(table);
    for (int e = 0; e < E; ++e) {
        sx::DropEntry t;
        std::memset(&t, 0, sizeof(t));
        sx::drop_fill(t, n_s, n_old[e], k, workspace[e]);
        t.y = y_train[e];
        t.w_old = linv_old[e];
        t.w_new = linv[e];
        t.alpha = alpha[e];
        t.logdet = logdet[e];
        t.status = status + e;
        t.blocks = sx::drop_blocks(t.m);
        t.blocks4 = sx::drop_blocks4(t.m);
        std::memcpy(out + e, &t, sizeof(t));
    }
    return SX_OK;
}

int sx_gp_drop_multi(int n_s, int E, int k, const int* n_old, const void* table, void* stream) {
    if (!table) return SX_ERR_ARG;
    if (int r = sx::drop_problems_check(n_s, E, k, n_old)) return r;
    if (int r = sx::drop_problems_supported(n_s, E, n_old)) return r;
    int m_max = 0;
    for (int e = 0; e < E; ++e) m_max = std::max(m_max, n_old[e] - k);
    sx::launch_drop<true>(static_cast<const sx::DropEntry*>(table), m_max, k, E * n_s, (hipStream_t)stream);
    return sx::check_launch();
}

}  // extern "C"
