// sx_gp_append: k <= 64 rows appended to a fitted exact GP without refactorising the old ones.
//
// Per output, with X [N x D], W = L^-1 of the fit, alpha, sum log diag L, and k new rows (X_c, y_c):
//   K_c = k(X, X_c) [N x k],  K_cc = k(X_c, X_c) + noise I,  B = W K_c,  S = K_cc - B^T B = L_s L_s^T,  W_s = L_s^-1,
//   W' = [ W 0 ; -W_s B^T W  W_s ],  alpha' = [alpha; 0] + W_bot^T (W_bot y'),  logdet' = logdet + sum log diag L_s.
//
// Six launches, all outputs side by side in the grid, 64 x 64 tiles on the f64 matrix cores (the k columns are padded to
// 64 with zeros, S and W_s with the identity; only the 16-column tiles and 16-row strips that hold one of the k columns
// are computed):
//   append_kc_kernel      K_c (zero padded) and K_cc into the workspace
//   append_b_kernel       B = W K_c, one workgroup per 64-row block of W; on the vector ALU, every dot product accumulated
//                         in twice the working precision (the kernel's comment says why)
//   append_btb_kernel     B^T B of kAppendPartBlocks row blocks per workgroup, summed in row order
//   append_schur_kernel   one workgroup per output: S = K_cc - sum of the partial products in part order, L_s, W_s (into
//                         the workspace and into the diagonal block of the new rows), sum log diag L_s
//   append_wbot_kernel    -W_s (B^T W) for one 64-column block of W per workgroup; its share of t = W_bot y'
//   append_copy_alpha_kernel   the old rows into the new stride, alpha'
// Every sum has a fixed order that depends on N and k only.  The bandwidth of the path is reading W twice.
//
// sx_gp_append_multi: the same six launches for E problems that share (n_s, D, k) and differ in N (MM = true).  The kernels
// then take the device table of the problems' AppendEntry, the grid's output index is e n_s + d and the x-extent of a launch is
// the largest problem's; a workgroup beyond its own problem's extent returns at once, and every loop over blocks, parts or
// the copy grid runs over the extents kept in the problem's entry, never the launch's: problem e's sums have the order, and
// its outputs the bits, of its own sx_gp_append.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"

namespace sx {

constexpr int kAppendMaxK = 64;         // the new rows of one call: one tile
constexpr int kAppendMaxN = 4096;       // N + k: sx_gp_fit's limit (kFitMaxN, sx_fit.hpp)
constexpr int kAT = 64;                 // tile edge
constexpr int kATLd = kAT + 1;          // LDS row stride of a staged tile (odd: an MFMA operand's 16 rows spread over banks)
constexpr int kAThreads = 256;          // 4 waves; wave w owns rows 16 w .. 16 w + 15 of a 64 x 64 result
constexpr int kAppendPartBlocks = 4;    // 64-row blocks of B per partial product of B^T B

struct AppendArgs {
    double inv_ls2[SX_MAX_NS * SX_MAX_D];
    double outputscale[SX_MAX_NS];
    double noise[SX_MAX_NS];
    const double* x;          // [(N + k) x D]
    const double* y;          // [(N + k) x n_s]
    const double* w_old;      // [n_s x N x N]
    const double* alpha_old;  // [n_s x N]
    const double* logdet_old; // [n_s]
    double* w_new;            // [n_s x (N + k) x (N + k)]
    double* alpha;            // [n_s x (N + k)]
    double* logdet;           // [n_s]
    int* status;
    // the workspace
    double* kc;               // [n_s x N x 64]        K_c, columns >= k zero
    double* b;                // [n_s x N x 64]        B
    double* kcc;              // [n_s x 64 x 64]       K_cc (rows, columns < k)
    double* btb;              // [n_s x nparts x 64 x 64]
    double* ws;               // [n_s x 64 x 64]       W_s, identity beyond k
    double* tpart;            // [n_s x (nblk + 1) x 64]   t = W_bot y' by column block of W, then the new columns' share
    int n, k, D, n_s, nblk, nparts;
};

// One problem of sx_gp_append_multi: an entry of the device table sx_gp_append_table lays out -- the problem's AppendArgs
// (status: its own word) and the x-extent of its own append_copy_alpha_kernel launch.
struct AppendEntry : AppendArgs {
    int copy_grid;
    int pad_;
};
static_assert(sizeof(AppendEntry) == SX_GP_APPEND_ENTRY_BYTES, "include/sx_amd.h: SX_GP_APPEND_ENTRY_BYTES");

// The argument of the append kernels, after FitArg (sx_fit.hpp): the AppendArgs itself (one model, the grid's output index
// is the output d), or with MM = true the device table of E problems' AppendEntry, of which the workgroup binds the entry
// of its problem: the grid's output index is then e n_s + d.  The pointer is restrict-qualified and never written and the
// index is uniform, so the entry is read through the constant address space (scalar loads, and the device pointers it holds
// are taken to be global, as those of a kernel argument are).
// (entry() and output() answer by value, so that the plain mode's statements keep their form and its ISA.)
template <bool MM>
struct AppendArg {
    using type = AppendArgs;
    __device__ static const AppendArgs& entry(const type& a, int) { return a; }
    __device__ static int output(const type&, int idx) { return idx; }
};
template <>
struct AppendArg<true> {
    using type = const AppendEntry* __restrict__;
    using ConstE = __attribute__((address_space(4))) const AppendEntry;
    __device__ static int problem(type table, int idx) { return idx / ((const ConstE*)table)[0].n_s; }
    __device__ static const AppendEntry& entry(type table, int idx) {
        return *(const AppendEntry*)((const ConstE*)table + problem(table, idx));
    }
    __device__ static int output(type table, int idx) { return idx - problem(table, idx) * ((const ConstE*)table)[0].n_s; }
};

__host__ __device__ inline int append_blocks(int n) { return (n + kAT - 1) / kAT; }
__host__ __device__ inline int append_parts(int n) { return (append_blocks(n) + kAppendPartBlocks - 1) / kAppendPartBlocks; }
// doubles of the workspace for n fitted rows and n_s outputs
inline int64_t append_workspace_doubles(int n_s, int n) {
    return (int64_t)n_s * (2 * (int64_t)n * kAT + 2 * kAT * kAT + (int64_t)append_parts(n) * kAT * kAT
                           + (int64_t)(append_blocks(n) + 1) * kAT);
}
// the x-extent of append_copy_alpha_kernel for n fitted rows
inline int append_copy_grid(int n) { return (n + 7) / 8 < 512 ? (n + 7) / 8 : 512; }

// rows r0 .. r0 + 63, columns c0 .. c0 + 63 of the row-major M (leading dimension ld, `rows` x `cols`) -> LDS [64][kATLd];
// zero outside the matrix (all 16 loads of a thread are issued before the first store)
__device__ __forceinline__ void append_load_tile(double* dst, const double* M, int ld, int rows, int cols, int r0, int c0) {
    constexpr int kPer = kAT * kAT / kAThreads;
    double v[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int idx = threadIdx.x + u * kAThreads;
        const int gr = r0 + (idx >> 6), gc = c0 + (idx & 63);
        v[u] = (gr < rows && gc < cols) ? M[(size_t)gr * ld + gc] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int idx = threadIdx.x + u * kAThreads;
        dst[(idx >> 6) * kATLd + (idx & 63)] = v[u];
    }
}

// acc[c] += A[16 w .. 16 w + 15][0..63] . B[0..63][16 c .. 16 c + 15] for the column tiles c < ct, operands staged in LDS:
// B[k][col] = Bs[k][col];  A[row][k] = As[row][k], or As[k][row] with AT (the left operand staged transposed)
template <bool AT>
__device__ __forceinline__ void append_mma(v4d (&acc)[4], const double* As, const double* Bs, int ct) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* ap = AT ? As + (lane >> 4) * kATLd + 16 * wave + (lane & 15)
                          : As + (16 * wave + (lane & 15)) * kATLd + (lane >> 4);
    const double* bp = Bs + (lane >> 4) * kATLd + (lane & 15);
#pragma unroll 4
    for (int k0 = 0; k0 < kAT; k0 += 4) {
        const double a = AT ? ap[k0 * kATLd] : ap[k0];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < ct) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bp[k0 * kATLd + 16 * c], acc[c], 0, 0, 0);
    }
}

// the wave's 16 x 64 result strip: lane holds D[(lane >> 4) + 4 r][16 c + (lane & 15)]
template <class F>
__device__ __forceinline__ void append_for_each(const v4d (&acc)[4], F&& f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) f(16 * wave + (lane >> 4) + 4 * r, 16 * c + (lane & 15), acc[c][r]);
}

// K_c [N x 64] (columns >= k zero) and K_cc [64 x 64] (rows and columns < k; the rest is never read): an element per thread
template <bool MM = false>
__global__ __launch_bounds__(kAThreads) void append_kc_kernel(typename AppendArg<MM>::type arg) {
    const auto& a = AppendArg<MM>::entry(arg, blockIdx.y);
    const int d = AppendArg<MM>::output(arg, blockIdx.y), n = a.n, k = a.k;
    // (the bound is the problem's own: beyond it the thread returns, whatever the launch's extent)
    const int64_t idx = (int64_t)blockIdx.x * kAThreads + threadIdx.x;
    if (idx >= (int64_t)(n + k) * kAT) return;
    const int i = (int)(idx >> 6), j = (int)(idx & 63);
    double v = 0.0;
    if (j < k) {
        v = gp_kernel_value(a, d, a.D, i, n + j);
        if (i == n + j) v += a.noise[d];
    }
    if (i < n)
        a.kc[((size_t)d * n + i) * kAT + j] = v;
    else
        a.kcc[((size_t)d * kAT + (i - n)) * kAT + j] = v;
}

// s + c += a b with the rounding errors of the product and of the sum kept in c (Ogita, Rump and Oishi's Dot2: TwoProduct by
// fma, Knuth's TwoSum).  No contraction: the error terms are exact only for the individually rounded operations.
__device__ __forceinline__ void append_dot2(double a, double b, double& s, double& c) {
#pragma clang fp contract(off)
    const double p = a * b;
    const double ep = __builtin_fma(a, b, -p);
    const double t = s + p;
    const double z = t - s;
    const double es = (s - (t - z)) + (p - z);
    s = t;
    c += ep + es;
}

// s + c += p, the rounding error of the sum kept in c (TwoSum)
__device__ __forceinline__ void append_two_sum(double p, double& s, double& c) {
#pragma clang fp contract(off)
    const double t = s + p;
    const double z = t - s;
    c += (s - (t - z)) + (p - z);
    s = t;
}

// B = W K_c: row block blockIdx.x of W, W is lower triangular (zeros above the diagonal, as sx_gp_fit leaves them).  This
// is the one product of the path that multiplies by an explicit inverse: |W| |K_c| exceeds |B| by up to the condition number
// of L, and plainly accumulated its rounding sets the error of the new rows (tests/test_gp_append_host.py,
// test_plain_float64_product_with_the_inverse_sets_the_error_of_the_new_rows).  So each dot product is accumulated
// in twice the working precision, on the vector ALU.  The 16 threads of a row group (4 rows: ty) share the column groups
// in use (4 columns each, rounded up to a power of two: cgp) and, where those are fewer than 16, the depth: thread tx works
// on column group tx % cgp and on every (16 / cgp)-th element of a dot product, and the slices are added at the end, in
// slice order and with the same care.  The split depends on k only.  N^2 k / 2 terms of ~10 operations: far below the fit.
template <bool MM = false>
__global__ __launch_bounds__(kAThreads) void append_b_kernel(typename AppendArg<MM>::type arg) {
    __shared__ double As[kAT * kATLd];
    __shared__ double Bs[kAT * kATLd];
    const auto& a = AppendArg<MM>::entry(arg, blockIdx.y);
    const int bi = blockIdx.x, d = AppendArg<MM>::output(arg, blockIdx.y), n = a.n, k = a.k;
    if constexpr (MM) {
        if (bi >= a.nblk) return;   // beyond this problem's row blocks (uniform; before any barrier)
    }
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int cgp = 1;
    while (4 * cgp < k) cgp <<= 1;
    const int nsl = 16 / cgp, g = tx & (cgp - 1), sl = tx / cgp;
    const int jn = min(4, k - 4 * g);   // this thread's columns in use (<= 0: none)
    const double* W = a.w_old + (size_t)d * n * n;
    const double* Kc = a.kc + (size_t)d * n * kAT;
    double s[4][4] = {}, c[4][4] = {};
    for (int kb = 0; kb <= bi; ++kb) {
        __syncthreads();
        append_load_tile(As, W, n, n, n, bi * kAT, kb * kAT);
        append_load_tile(Bs, Kc, kAT, n, kAT, kb * kAT, 0);
        __syncthreads();
        if (jn > 0) {
            for (int q = sl; q < kAT; q += nsl) {
                double av[4], bv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = As[(4 * ty + i) * kATLd + q];
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = Bs[q * kATLd + 4 * g + j];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < jn) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) append_dot2(av[i], bv[j], s[i][j], c[i][j]);
                    }
            }
        }
    }
    // the slices' sums, [slice][row][column < 4 cgp]: 16 / cgp * 64 * 4 cgp = 4096 doubles in each of the two tiles
    __syncthreads();
    const int wcols = 4 * cgp;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int at = (sl * kAT + 4 * ty + i) * wcols + 4 * g + j;
            As[at] = s[i][j];
            Bs[at] = c[i][j];
        }
    __syncthreads();
    double* B = a.b + (size_t)d * n * kAT;
    for (int idx = threadIdx.x; idx < kAT * kAT; idx += kAThreads) {
        const int row = idx >> 6, col = idx & 63, gr = bi * kAT + row;
        double v = 0.0;
        if (col < wcols) {
            double ss = As[row * wcols + col], cc = Bs[row * wcols + col];
            for (int q = 1; q < nsl; ++q) {
                const int at = (q * kAT + row) * wcols + col;
                append_two_sum(As[at], ss, cc);
                cc += Bs[at];
            }
            v = ss + cc;
        }
        if (gr < n) B[(size_t)gr * kAT + col] = v;
    }
}

// part blockIdx.x of B^T B: the row blocks kAppendPartBlocks p .. of B, in order
template <bool MM = false>
__global__ __launch_bounds__(kAThreads) void append_btb_kernel(typename AppendArg<MM>::type arg) {
    __shared__ double As[kAT * kATLd];
    const auto& a = AppendArg<MM>::entry(arg, blockIdx.y);
    const int d = AppendArg<MM>::output(arg, blockIdx.y), p = blockIdx.x, n = a.n;
    if constexpr (MM) {
        if (p >= a.nparts) return;   // beyond this problem's parts (uniform; before any barrier)
    }
    const int ct = (a.k + 15) >> 4, wave = threadIdx.x >> 6;
    const double* B = a.b + (size_t)d * n * kAT;
    v4d acc[4] = {};
    const int b_end = min(a.nblk, (p + 1) * kAppendPartBlocks);
    for (int bi = p * kAppendPartBlocks; bi < b_end; ++bi) {
        __syncthreads();
        append_load_tile(As, B, kAT, n, kAT, bi * kAT, 0);
        __syncthreads();
        if (wave < ct) append_mma<true>(acc, As, As, ct);   // (uniform per wave; no barrier inside)
    }
    double* out = a.btb + ((size_t)d * a.nparts + p) * kAT * kAT;
    append_for_each(acc, [&](int r, int c, double v) { out[r * kAT + c] = v; });
}

// One workgroup per output: S, its Cholesky factor and the factor's inverse -- the work fit_potrf_diag_kernel does for a
// diagonal block (sx_fit_blocked.hpp), on the leading k x k part of a block padded with the identity: the padding is its
// own factor and inverse, so the k pivots and the k rows of the substitution are all the work there is
template <bool MM = false>
__global__ __launch_bounds__(kAThreads) void append_schur_kernel(typename AppendArg<MM>::type arg) {
    __shared__ double L[kAT * kATLd];
    __shared__ double Wd[kAT * kATLd];
    const auto& a = AppendArg<MM>::entry(arg, blockIdx.x);
    const int d = AppendArg<MM>::output(arg, blockIdx.x), tid = threadIdx.x, n = a.n, k = a.k, n2 = a.n + a.k;
    const double* kcc = a.kcc + (size_t)d * kAT * kAT;
    const double* btb = a.btb + (size_t)d * a.nparts * kAT * kAT;
    for (int idx = tid; idx < kAT * kAT; idx += kAThreads) {
        const int r = idx >> 6, c = idx & 63;
        double s = (r == c) ? 1.0 : 0.0;
        if (r < k && c < k) {
            s = kcc[idx];
            for (int p = 0; p < a.nparts; ++p) s -= btb[(size_t)p * kAT * kAT + idx];
        }
        L[r * kATLd + c] = s;
    }
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < k; ++j) {
        const double ajj = L[j * kATLd + j];
        if (!(ajj > 0.0)) bad = true;
        const double piv = sqrt(ajj);
        __syncthreads();  // everyone has read the pivot
        if (tid >= j && tid < k) L[tid * kATLd + j] = (tid == j) ? piv : L[tid * kATLd + j] / piv;
        __syncthreads();
        // rank-1 update of the trailing lower triangle: rows r > j, columns j < c <= r
        for (int idx = ((j + 1) << 6) + tid; idx < (k << 6); idx += kAThreads) {
            const int r = idx >> 6, c = idx & 63;
            if (c > j && c <= r) L[r * kATLd + c] -= L[r * kATLd + j] * L[c * kATLd + j];
        }
        __syncthreads();
    }
    if (bad && tid == 0) atomicOr(a.status, SX_STATUS_NOT_PD);
    // Wd = L^-1 by forward substitution, thread c solves column c and keeps it in registers (static indices, fully
    // unrolled; the rows >= k are the identity's, behind a uniform branch)
    if (tid < kAT) {
        const int c = tid;
        double w[kAT];
#pragma unroll
        for (int r = 0; r < kAT; ++r) {
            double s = (r == c) ? 1.0 : 0.0;
            if (r < k) {
#pragma unroll
                for (int q = 0; q < r; ++q) s -= L[r * kATLd + q] * w[q];
                s = (r >= c) ? s / L[r * kATLd + r] : 0.0;
            }
            w[r] = s;
            Wd[r * kATLd + c] = s;
        }
    }
    __syncthreads();
    double* W2 = a.w_new + (size_t)d * n2 * n2;
    double* ws = a.ws + (size_t)d * kAT * kAT;
    for (int idx = tid; idx < kAT * kAT; idx += kAThreads) {
        const int r = idx >> 6, c = idx & 63;
        const double v = Wd[r * kATLd + c];
        ws[idx] = v;
        if (r < k && c < k) W2[(size_t)(n + r) * n2 + n + c] = v;
    }
    // the new columns' share of t = W_bot y', and the sum of logs, each in index order
    if (tid < kAT) {
        double t = 0.0;
        if (tid < k)
            for (int c = 0; c <= tid; ++c) t += Wd[tid * kATLd + c] * a.y[(size_t)(n + c) * a.n_s + d];
        a.tpart[((size_t)d * (a.nblk + 1) + a.nblk) * kAT + tid] = t;
    }
    if (tid == 0) {
        double ld = a.logdet_old[d];
        for (int j = 0; j < k; ++j) ld += log(L[j * kATLd + j]);
        a.logdet[d] = ld;
    }
}

// columns 64 blockIdx.x .. of the new rows: -W_s (B^T W), the sum over the row blocks of W at and below the diagonal
template <bool MM = false>
__global__ __launch_bounds__(kAThreads) void append_wbot_kernel(typename AppendArg<MM>::type arg) {
    __shared__ double As[kAT * kATLd];
    __shared__ double Bs[kAT * kATLd];
    const auto& a = AppendArg<MM>::entry(arg, blockIdx.y);
    const int d = AppendArg<MM>::output(arg, blockIdx.y), cj = blockIdx.x, n = a.n, k = a.k, n2 = a.n + a.k;
    if constexpr (MM) {
        if (cj >= a.nblk) return;   // beyond this problem's column blocks (uniform; before any barrier)
    }
    const int rt = (k + 15) >> 4, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const double* W = a.w_old + (size_t)d * n * n;
    const double* B = a.b + (size_t)d * n * kAT;
    v4d acc[4] = {};
    for (int bi = cj; bi < a.nblk; ++bi) {
        __syncthreads();
        append_load_tile(As, B, kAT, n, kAT, bi * kAT, 0);
        append_load_tile(Bs, W, n, n, n, bi * kAT, cj * kAT);
        __syncthreads();
        if (wave < rt) append_mma<true>(acc, As, Bs, 4);
    }
    __syncthreads();
    append_load_tile(As, a.ws + (size_t)d * kAT * kAT, kAT, kAT, kAT, 0, 0);
    append_for_each(acc, [&](int r, int c, double v) { Bs[r * kATLd + c] = v; });
    __syncthreads();
    v4d out[4] = {};
    if (wave < rt) append_mma<false>(out, As, Bs, 4);
    __syncthreads();
    double* W2 = a.w_new + (size_t)d * n2 * n2;
    append_for_each(out, [&](int r, int c, double v) {
        const int gc = cj * kAT + c;
        As[r * kATLd + c] = -v;
        if (r < k && gc < n) W2[(size_t)(n + r) * n2 + gc] = -v;
    });
    __syncthreads();
    if (tid < kAT) {
        double t = 0.0;
        if (tid < k)
            for (int c = 0; c < kAT && cj * kAT + c < n; ++c) t += As[tid * kATLd + c] * a.y[(size_t)(cj * kAT + c) * a.n_s + d];
        a.tpart[((size_t)d * (a.nblk + 1) + cj) * kAT + tid] = t;
    }
}

// The old rows of W into the new stride (k zeros appended; nothing above the diagonal is read), and
// alpha' = [alpha; 0] + W_bot^T t with t the sum of its parts in block order.  Rows and columns are dealt out over the grid.
template <bool MM = false>
__global__ __launch_bounds__(kAThreads) void append_copy_alpha_kernel(typename AppendArg<MM>::type arg) {
    __shared__ double t[kAT];
    const auto& a = AppendArg<MM>::entry(arg, blockIdx.y);
    const int d = AppendArg<MM>::output(arg, blockIdx.y), tid = threadIdx.x, n = a.n, k = a.k, n2 = a.n + a.k;
    // the grid the rows and columns are dealt out over: this problem's own
    const auto grid = [&]() -> unsigned {
        if constexpr (MM)
            return a.copy_grid;
        else
            return gridDim.x;
    };
    if constexpr (MM) {
        if (blockIdx.x >= grid()) return;   // (uniform; before the barrier)
    }
    const double* W = a.w_old + (size_t)d * n * n;
    double* W2 = a.w_new + (size_t)d * n2 * n2;
    if (tid < kAT) {
        double s = 0.0;
        for (int p = 0; p <= a.nblk; ++p) s += a.tpart[((size_t)d * (a.nblk + 1) + p) * kAT + tid];
        t[tid] = s;
    }
    for (int i = blockIdx.x; i < n; i += grid())
        for (int c = tid; c < n2; c += kAThreads) W2[(size_t)i * n2 + c] = (c <= i) ? W[(size_t)i * n + c] : 0.0;
    __syncthreads();
    // (append_schur_kernel wrote the new rows' own block whole, zeros above its diagonal included)
    for (int c = blockIdx.x * kAThreads + tid; c < n2; c += grid() * kAThreads) {
        double s = (c < n) ? a.alpha_old[(size_t)d * n + c] : 0.0;
        for (int r = (c < n) ? 0 : c - n; r < k; ++r) s += W2[(size_t)(n + r) * n2 + c] * t[r];
        a.alpha[(size_t)d * n2 + c] = s;
    }
}

}  // namespace sx
