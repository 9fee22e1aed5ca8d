// sx_gp_append and sx_gp_append_workspace_bytes: the kernels of sx_gp_append.hpp and their launch sequence.  Every argument
// check answers before the first HIP call (tests/test_gp_append_host.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/sx_amd.h"
#include "sx_gp_append.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"

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
    const int n_s = model->n_s, n_u = model->n_u, n2 = model->n_train;
    if (n_s <= 0 || n_s > SX_MAX_NS || n_u <= 0 || n_u > SX_MAX_D - n_s || n2 <= 0) return SX_ERR_ARG;
    if (n_old < 1) return SX_ERR_ARG;
    const int k = n2 - n_old;
    if (k < 1 || k > sx::kAppendMaxK) return SX_ERR_ARG;
    if (workspace_bytes < sx::append_workspace_doubles(n_s, n_old) * (int64_t)sizeof(double)) return SX_ERR_ARG;
    if (n2 > sx::kAppendMaxN) return SX_ERR_UNSUPPORTED;

    sx::AppendArgs a;
    std::memset(&a, 0, sizeof(a));
    sx::copy_hyper(*model, a.inv_ls2, a.outputscale, a.noise);
    a.x = model->x_train;
    a.y = y_train;
    a.w_old = linv_old;
    a.alpha_old = alpha_old;
    a.logdet_old = logdet_old;
    a.w_new = linv;
    a.alpha = alpha;
    a.logdet = logdet;
    a.status = status;
    a.n = n_old;
    a.k = k;
    a.D = n_s + n_u;
    a.n_s = n_s;
    a.nblk = sx::append_blocks(n_old);
    a.nparts = sx::append_parts(n_old);
    double* w = static_cast<double*>(workspace);
    a.kc = w;
    w += (size_t)n_s * n_old * sx::kAT;
    a.b = w;
    w += (size_t)n_s * n_old * sx::kAT;
    a.kcc = w;
    w += (size_t)n_s * sx::kAT * sx::kAT;
    a.ws = w;
    w += (size_t)n_s * sx::kAT * sx::kAT;
    a.btb = w;
    w += (size_t)n_s * a.nparts * sx::kAT * sx::kAT;
    a.tpart = w;

    hipStream_t s = (hipStream_t)stream;
    const dim3 block(sx::kAThreads);
    const int kc_grid = (int)(((int64_t)n2 * sx::kAT + sx::kAThreads - 1) / sx::kAThreads);
    hipLaunchKernelGGL(sx::append_kc_kernel, dim3(kc_grid, n_s), block, 0, s, a);
    hipLaunchKernelGGL(sx::append_b_kernel, dim3(a.nblk, n_s), block, 0, s, a);
    hipLaunchKernelGGL(sx::append_btb_kernel, dim3(a.nparts, n_s), block, 0, s, a);
    hipLaunchKernelGGL(sx::append_schur_kernel, dim3(n_s), block, 0, s, a);
    hipLaunchKernelGGL(sx::append_wbot_kernel, dim3(a.nblk, n_s), block, 0, s, a);
    const int copy_grid = std::min(512, (n_old + 7) / 8);
    hipLaunchKernelGGL(sx::append_copy_alpha_kernel, dim3(copy_grid, n_s), block, 0, s, a);
    return sx::check_launch();
}

}  // extern "C"
