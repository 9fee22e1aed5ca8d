// sx_feat_fit: the weight-space fit of the degenerate-kernel GPs of sx_feat.hpp.  A non-template kernel, so that only
// sx_feat.hip includes it (sx_feat.hpp itself is included by more than one translation unit).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_feat.hpp"

namespace sx {

// ---- sx_feat_fit: A_d = Phi^T Phi + lambda_d I, M_d = chol(A_d)^-1, wbar_d = M_d^T M_d Phi^T y_d ------------------------
// One workgroup of 1024 threads per output; F <= 32, so A (F x F) has one thread per entry and lives in LDS.
// stats[d] = { y_d^T y_d, |M_d Phi^T y_d|^2, sum log diag chol(A_d) }: what the exact marginal likelihood needs.
struct FeatFitArgs {
    const double* phi;   // [N x F]
    const double* y;     // [N x n_s]
    double lambda[SX_MAX_NS];
    double* wbar;        // [n_s x F]
    double* minv;        // [n_s x F x F]
    double* stats;       // [n_s x 3]
    int* status;
    int n, F, n_s;
};

__global__ __launch_bounds__(1024) void feat_fit_kernel(FeatFitArgs a) {
    __shared__ double A[SX_FEAT_MAX_WIDTH][SX_FEAT_MAX_WIDTH + 1];
    __shared__ double Li[SX_FEAT_MAX_WIDTH][SX_FEAT_MAX_WIDTH + 1];
    __shared__ double b[SX_FEAT_MAX_WIDTH], t[SX_FEAT_MAX_WIDTH];
    __shared__ double yy_part[16];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int F = a.F, n = a.n;
    const int r = tid / SX_FEAT_MAX_WIDTH, c = tid % SX_FEAT_MAX_WIDTH;
    if (r < F && c <= r) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s = fma(a.phi[(size_t)i * F + r], a.phi[(size_t)i * F + c], s);
        if (r == c) s += a.lambda[d];
        A[r][c] = s;
        A[c][r] = s;
    }
    if (tid < F) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s = fma(a.phi[(size_t)i * F + tid], a.y[(size_t)i * a.n_s + d], s);
        b[tid] = s;
    }
    {
        double s = 0.0;
        for (int i = tid; i < n; i += 1024) {
            const double v = a.y[(size_t)i * a.n_s + d];
            s = fma(v, v, s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if ((tid & 63) == 0) yy_part[tid >> 6] = s;
    }
    __syncthreads();
    // Cholesky A = L L^T in place (lower), column by column; F <= 32: one wave's worth of rows
    bool bad = false;
    for (int j = 0; j < F; ++j) {
        if (tid == 0) {
            const double p = A[j][j];
            if (!(p > 0.0)) bad = true;
            A[j][j] = sqrt(p);
        }
        __syncthreads();
        if (tid > j && tid < F) A[tid][j] /= A[j][j];
        __syncthreads();
        if (r > j && r < F && c > j && c <= r) A[r][c] -= A[r][j] * A[c][j];
        __syncthreads();
    }
    // M = L^-1 by forward substitution, one column per thread
    if (tid < F) {
        const int col = tid;
        for (int i = 0; i < F; ++i) {
            double s = (i == col) ? 1.0 : 0.0;
            for (int k = col; k < i; ++k) s -= A[i][k] * Li[k][col];
            Li[i][col] = (i >= col) ? s / A[i][i] : 0.0;
        }
    }
    __syncthreads();
    if (tid < F) {   // t = M b
        double s = 0.0;
        for (int k = 0; k <= tid; ++k) s = fma(Li[tid][k], b[k], s);
        t[tid] = s;
    }
    __syncthreads();
    if (tid < F) {   // wbar = M^T t
        double s = 0.0;
        for (int k = tid; k < F; ++k) s = fma(Li[k][tid], t[k], s);
        a.wbar[(size_t)d * F + tid] = s;
    }
    if (r < F && c < F) a.minv[((size_t)d * F + r) * F + c] = (c <= r) ? Li[r][c] : 0.0;
    if (tid == 0) {
        double yy = 0.0, tt = 0.0, ld = 0.0;
        for (int w = 0; w < 16; ++w) yy += yy_part[w];
        for (int k = 0; k < F; ++k) {
            tt = fma(t[k], t[k], tt);
            ld += log(A[k][k]);
        }
        a.stats[d * 3 + 0] = yy;
        a.stats[d * 3 + 1] = tt;
        a.stats[d * 3 + 2] = ld;
        if (bad) atomicOr(a.status, SX_STATUS_NOT_PD);
    }
}

}  // namespace sx
