// sx_gp_drop and sx_gp_drop_workspace_bytes: the kernels of sx_gp_drop.hpp and their launch sequence.  Every argument check
// answers before the first HIP call (tests/test_gp_drop_host.py).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/sx_amd.h"
#include "sx_gp_drop.hpp"
#include "sx_launch.hpp"

namespace sx {

// the table and the main kernel for KB stages
template <int KB>
static void launch_stages(const DropArgs& a, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(drop_table_kernel<KB>, dim3(a.n_s), dim3(kDT), 0, s, a);
    hipLaunchKernelGGL(drop_main_kernel<KB>, dim3(blocks, a.n_s), dim3(kDT), 0, s, a);
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
    a.y = y_train;
    a.w_old = linv_old;
    a.w_new = linv;
    a.alpha = alpha;
    a.logdet = logdet;
    a.status = status;
    a.n = n_old;
    a.k = k;
    a.m = m;
    a.n_s = n_s;
    double* w = static_cast<double*>(workspace);
    a.l11 = w;
    w += (size_t)n_s * sx::kDT * sx::kDT;
    a.v = w;
    w += (size_t)n_s * m * sx::kDT;
    a.tab = w;
    w += (size_t)n_s * m * sx::drop_stages(k) * 3;
    a.t = w;

    hipStream_t s = (hipStream_t)stream;
    const int blocks = (m + sx::kDT - 1) / sx::kDT;
    hipLaunchKernelGGL(sx::drop_l11_kernel, dim3(n_s), dim3(sx::kDThreads), 0, s, a);
    hipLaunchKernelGGL(sx::drop_v_kernel, dim3(blocks, n_s), dim3(sx::kDThreads), 0, s, a);
    switch (sx::drop_stages(k)) {
        case 1: sx::launch_stages<1>(a, blocks, s); break;
        case 2: sx::launch_stages<2>(a, blocks, s); break;
        case 4: sx::launch_stages<4>(a, blocks, s); break;
        case 8: sx::launch_stages<8>(a, blocks, s); break;
        case 16: sx::launch_stages<16>(a, blocks, s); break;
        case 32: sx::launch_stages<32>(a, blocks, s); break;
        default: sx::launch_stages<64>(a, blocks, s); break;
    }
    hipLaunchKernelGGL(sx::drop_t_kernel, dim3((m + 3) / 4, n_s), dim3(sx::kDThreads), 0, s, a);
    hipLaunchKernelGGL(sx::drop_alpha_kernel, dim3(blocks, n_s), dim3(sx::kDThreads), 0, s, a);
    hipLaunchKernelGGL(sx::drop_logdet_kernel, dim3(n_s), dim3(sx::kDThreads), 0, s, a);
    return sx::check_launch();
}

}  // extern "C"
