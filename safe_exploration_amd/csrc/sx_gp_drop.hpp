// sx_gp_drop: the k <= 64 OLDEST rows removed from a fitted exact GP without refactorising the kept ones (DESIGN.md
// section 3.5) -- the other half of sx_gp_append, for a model that slides a window over its data.
//
// Per output, with W = L^-1 of the fit of N rows partitioned after the first k, W = [ W11 0 ; W21 W22 ], m = N - k kept rows:
//   K22 = L22 L22^T + L21 L21^T  (a rank-k UPDATE of the kept rows' own factor, positive sign),
//   L11 = W11^-1,  V = L22^-1 L21 = -W21 L11 [m x k],  W' = chol(I + V V^T)^-1 W22.
// chol(I + V V^T) is a product of k rank-1 factors, and its inverse applies to every column of W22 independently in one pass
// over the rows.  With U = V, t_s = 1 and running sums sV[s][q] = 0, sX[s][c] = 0, for row i = 0 .. m - 1 and stage s = 0 .. k - 1:
//   u = U[i,s];  tn = t_s + u^2;  dinv = sqrt(t_s / tn);  coef = u / sqrt(tn t_s)
//   q > s:   U[i,q] = (U[i,q] - u sV[s][q]) dinv;   sV[s][q] += coef U[i,q]
//   c <= i:  X[i,c] = (X[i,c] - u sX[s][c]) dinv;   sX[s][c] += coef X[i,c]
//   t_s = tn
// X starts as W22 and ends as W'.  alpha' = W'^T (W' y2),  sum log diag L' = -sum log diag W'.
//
// Seven launches, all outputs side by side in the grid:
//   drop_l11_kernel     one workgroup per output: W11 checked (a diagonal that is not > 0, an entry that is not finite), L11
//   drop_v_kernel       V for 64 kept rows per workgroup, its columns >= k zero
//   drop_table_kernel   one wave per output: the scalars (u, dinv, coef) of every (row, stage), the only chain that is serial
//                       in the rows.  Lane s owns stage s (t_s and sV[s][.] in registers) and works on row tick - s: the rows
//                       pass down the stages as a wavefront through a ring in LDS, so the chain is m + k ticks, not m k steps
//   drop_main_kernel    one lane per column of W22, one wave per 64 columns: walks the rows from the diagonal block down with
//                       its running sums in registers and writes the new stride, zeros above the diagonal included
//   drop_t_kernel       t = W' y2, a wave per row
//   drop_alpha_kernel   alpha' = W'^T t, a lane per column
//   drop_logdet_kernel  -sum log diag W'
// The table and the main kernel are compiled for KB = 1, 2, 4, .. 64 stages and run the smallest KB >= k: a stage s >= k meets
// a zero column of V, so u = 0, dinv = 1, coef = 0 and the stage changes nothing, bit for bit; their loops over the stages
// are straight-line code with static register indices.
// Every sum has a fixed order that depends on N and k only; no atomics on doubles; nothing waits across workgroups.
//
// sx_gp_drop_multi: the same seven launches for E problems that share (n_s, k), hence KB, and differ in N (MM = true).  The
// kernels then take the device table of the problems' DropEntry and the grid's output index is e n_s + d: x for
// drop_l11_kernel, drop_table_kernel and drop_logdet_kernel, y for the other four, whose x-extent is the largest problem's.
// A workgroup beyond its own problem's extent (64-row blocks for drop_v_kernel, drop_main_kernel and drop_alpha_kernel,
// 4-row blocks for drop_t_kernel) returns before it touches that problem's memory or reaches a barrier; the test is uniform
// per workgroup.  The contract: no kernel reads gridDim and every loop bound comes from the problem's own n, k, m, so the
// workgroups of problem e that run are exactly those of its single call, with the same block indices and the same
// statements: linv, alpha and logdet of problem e are sx_gp_drop's for that model alone, bit for bit, whatever else shares the
// call and in whatever order.  The status word is the problem's own: one problem that is not positive definite leaves the
// others valid.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"

namespace sx {

constexpr int kDropMaxK = 64;        // the rows one call removes: one lane per stage of the table kernel
constexpr int kDropMaxN = 4096;      // sx_gp_fit's limit (kFitMaxN, sx_fit.hpp)
constexpr int kDT = 64;              // tile edge, and the row stride of V
constexpr int kDTLd = kDT + 1;       // LDS row stride (odd: the lanes of a wave that walk down a column spread over the banks)
constexpr int kDThreads = 256;
constexpr int kDropRing = 96;        // rows of V in flight in the table kernel: 64 stages deep + two chunks of prefetch
constexpr int kDropChunk = 16;       // rows of V the table kernel fetches at a time
// rows of W22 the main kernel loads ahead of the row it works on (fewer where the running sums take the registers)
__host__ __device__ constexpr int drop_rows_ahead(int kb) { return kb >= 64 ? 4 : kb >= 32 ? 8 : 16; }
constexpr int kDropAlphaWaves = 4;   // the row classes (i mod 4) whose partial sums drop_alpha_kernel adds in class order

// the compiled stage count for k dropped rows: the smallest power of two >= k
__host__ __device__ inline int drop_stages(int k) {
    int kb = 1;
    while (kb < k) kb <<= 1;
    return kb;
}

struct DropArgs {
    const double* y;         // [m x n_s]            the kept rows' targets
    const double* w_old;     // [n_s x N x N]
    double* w_new;           // [n_s x m x m]
    double* alpha;           // [n_s x m]
    double* logdet;          // [n_s]
    int* status;
    // the workspace
    double* l11;             // [n_s x 64 x 64]      L11 (rows, columns < k), identity beyond
    double* v;               // [n_s x m x 64]       V, columns >= k zero
    double* tab;             // [n_s x m x KB x 3]   (u, dinv, coef) of row i, stage s; KB = drop_stages(k)
    double* t;               // [n_s x m]            W' y2
    int n, k, m, n_s;
};

// One problem of sx_gp_drop_multi: an entry of the device table sx_gp_drop_table lays out -- the problem's DropArgs (status:
// its own word) and the x-extents of its own launches.
struct DropEntry : DropArgs {
    int blocks;              // 64-row blocks of the kept rows: drop_v_kernel, drop_main_kernel, drop_alpha_kernel
    int blocks4;             // 4-row blocks: drop_t_kernel
};
static_assert(sizeof(DropEntry) == SX_GP_DROP_ENTRY_BYTES, "include/sx_amd.h: SX_GP_DROP_ENTRY_BYTES");

// The argument of the drop kernels, after AppendArg (sx_gp_append.hpp): the DropArgs itself (one model, the grid's output
// index is the output d), or with MM = true the device table of E problems' DropEntry, of which the workgroup binds the
// entry of its problem: the grid's output index is then e n_s + d.  The pointer is restrict-qualified and never written and
// the index is uniform, so the entry is read through the constant address space (scalar loads, and the device pointers it
// holds are taken to be global, as those of a kernel argument are).
// (entry() and output() answer by value, so that the plain mode's statements keep their form and its ISA.)
template <bool MM>
struct DropArg {
    using type = DropArgs;
    __device__ static const DropArgs& entry(const type& a, int) { return a; }
    __device__ static int output(const type&, int idx) { return idx; }
};
template <>
struct DropArg<true> {
    using type = const DropEntry* __restrict__;
    using ConstE = __attribute__((address_space(4))) const DropEntry;
    __device__ static int problem(type table, int idx) { return idx / ((const ConstE*)table)[0].n_s; }
    __device__ static const DropEntry& entry(type table, int idx) {
        return *(const DropEntry*)((const ConstE*)table + problem(table, idx));
    }
    __device__ static int output(type table, int idx) { return idx - problem(table, idx) * ((const ConstE*)table)[0].n_s; }
};

__host__ __device__ inline int drop_blocks(int m) { return (m + kDT - 1) / kDT; }
__host__ __device__ inline int drop_blocks4(int m) { return (m + kDThreads / 64 - 1) / (kDThreads / 64); }

// doubles of the workspace for n_s outputs, m kept rows and k dropped ones
inline int64_t drop_workspace_doubles(int n_s, int m, int k) {
    return (int64_t)n_s * ((int64_t)kDT * kDT + (int64_t)m * kDT + (int64_t)m * drop_stages(k) * 3 + m);
}

// One workgroup per output.  W11 into LDS (padded with the identity), checked; L11 = W11^-1 by forward substitution, thread c
// solves column c and keeps it in registers (static indices, fully unrolled; the rows >= k are the identity's)
template <bool MM = false>
__global__ __launch_bounds__(kDThreads) void drop_l11_kernel(typename DropArg<MM>::type arg) {
    __shared__ double Ws[kDT * kDTLd];
    const auto& a = DropArg<MM>::entry(arg, blockIdx.x);
    const int d = DropArg<MM>::output(arg, blockIdx.x), tid = threadIdx.x, n = a.n, k = a.k;
    const double* W = a.w_old + (size_t)d * n * n;
    bool bad = false;
    for (int idx = tid; idx < kDT * kDT; idx += kDThreads) {
        const int r = idx >> 6, c = idx & 63;
        double v = (r == c) ? 1.0 : 0.0;
        if (r < k && c <= r) {
            v = W[(size_t)r * n + c];
            if (!(v - v == 0.0) || (r == c && !(v > 0.0))) bad = true;
        }
        Ws[r * kDTLd + c] = v;
    }
    if (bad) atomicOr(a.status, SX_STATUS_NOT_PD);
    __syncthreads();
    if (tid < kDT) {
        const int c = tid;
        double w[kDT];
        double* out = a.l11 + (size_t)d * kDT * kDT;
#pragma unroll
        for (int r = 0; r < kDT; ++r) {
            double s = (r == c) ? 1.0 : 0.0;
            if (r < k) {
#pragma unroll
                for (int q = 0; q < r; ++q) s -= Ws[r * kDTLd + q] * w[q];
                s = (r >= c) ? s / Ws[r * kDTLd + r] : 0.0;
            }
            w[r] = s;
            out[r * kDT + c] = s;
        }
    }
}

// V = -W21 L11 for the kept rows 64 blockIdx.x ..: V[i][s] = -sum over q = s .. k - 1 (in that order) of W21[i][q] L11[q][s];
// the columns s >= k are zero
template <bool MM = false>
__global__ __launch_bounds__(kDThreads) void drop_v_kernel(typename DropArg<MM>::type arg) {
    __shared__ double As[kDT * kDTLd];
    __shared__ double Ls[kDT * kDTLd];
    const auto& a = DropArg<MM>::entry(arg, blockIdx.y);
    const int d = DropArg<MM>::output(arg, blockIdx.y), tid = threadIdx.x, n = a.n, k = a.k, m = a.m, i0 = blockIdx.x * kDT;
    if constexpr (MM) {
        if ((int)blockIdx.x >= a.blocks) return;   // beyond this problem's row blocks (uniform; before any barrier)
    }
    const double* W = a.w_old + (size_t)d * n * n;
    const double* l11 = a.l11 + (size_t)d * kDT * kDT;
    for (int idx = tid; idx < kDT * kDT; idx += kDThreads) {
        const int r = idx >> 6, c = idx & 63;
        Ls[r * kDTLd + c] = l11[idx];
        As[r * kDTLd + c] = (i0 + r < m && c < k) ? W[(size_t)(k + i0 + r) * n + c] : 0.0;
    }
    __syncthreads();
    double* V = a.v + (size_t)d * m * kDT;
    const int s = tid & 63;
    for (int r = tid >> 6; r < kDT; r += kDThreads / kDT) {
        if (i0 + r >= m) break;
        double acc = 0.0;
        for (int q = s; q < k; ++q) acc += As[r * kDTLd + q] * Ls[q * kDTLd + s];
        V[(size_t)(i0 + r) * kDT + s] = -acc;
    }
}

// One wave per output, KB stages.  Lane s < KB is stage s: it keeps t_s and the running sums sV[s][q] in registers and at tick T
// works on row i = T - s, which stage s - 1 left in the ring one tick earlier: it takes u = U[i][s], writes the row's
// (u, dinv, coef) into the table and updates the row's columns in place.  (It updates the columns q <= s too, in the ring and
// in its registers, from values nobody reads again: the loop over q is straight-line code without a lane mask.)  The rows
// of V are fetched a chunk at a time, one chunk ahead in registers and one more in the ring; a row lives in the ring from at
// most 2 kDropChunk - 1 ticks before its stage 0 to its last stage: kDropRing slots.
template <int KB, bool MM = false>
__global__ __launch_bounds__(kDT) void drop_table_kernel(typename DropArg<MM>::type arg) {
    static_assert(KB <= kDT && kDropRing >= kDT + 2 * kDropChunk, "a row's slot is reused while a stage still needs it");
    __shared__ double R[kDropRing * kDTLd];
    const auto& a = DropArg<MM>::entry(arg, blockIdx.x);
    const int d = DropArg<MM>::output(arg, blockIdx.x), lane = threadIdx.x, m = a.m;
    const double* V = a.v + (size_t)d * m * kDT;
    double* tab = a.tab + (size_t)d * m * KB * 3;
    double sv[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q) sv[q] = 0.0;
    double t = 1.0;
    bool bad = false;
    double next[kDropChunk];
    // rows 0 .. kDropChunk - 1 into the ring; the tick loop's first fetch (at tick 0) brings the second chunk
#pragma unroll
    for (int j = 0; j < kDropChunk; ++j) R[j * kDTLd + lane] = (j < m) ? V[(size_t)j * kDT + lane] : 0.0;
#pragma unroll
    for (int j = 0; j < kDropChunk; ++j) next[j] = (kDropChunk + j < m) ? V[(size_t)(kDropChunk + j) * kDT + lane] : 0.0;
    const int ticks = m + KB - 1;
    for (int tick = 0; tick < ticks; ++tick) {
        if ((tick & (kDropChunk - 1)) == 0) {
            // rows tick + 16 .. tick + 31 from the registers into the ring, rows tick + 32 .. tick + 47 into the registers
#pragma unroll
            for (int j = 0; j < kDropChunk; ++j) R[((tick + kDropChunk + j) % kDropRing) * kDTLd + lane] = next[j];
#pragma unroll
            for (int j = 0; j < kDropChunk; ++j) {
                const int row = tick + 2 * kDropChunk + j;
                next[j] = (row < m) ? V[(size_t)row * kDT + lane] : 0.0;
            }
        }
        // One wave, whose LDS accesses complete in program order: the ring's writes of the last tick are visible.  (No
        // workgroup barrier: its fence would wait for the table's stores to arrive, a memory round trip per tick.)
        __builtin_amdgcn_wave_barrier();
        const int i = tick - lane;
        if (lane < KB && i >= 0 && i < m) {
            double* row = R + (i % kDropRing) * kDTLd;
            const double u = row[lane];
            const double tn = t + u * u;
            if (!(tn - tn == 0.0)) bad = true;
            const double dinv = sqrt(t / tn), coef = u / sqrt(tn * t);
            t = tn;
            double* out = tab + ((size_t)i * KB + lane) * 3;
            out[0] = u;
            out[1] = dinv;
            out[2] = coef;
#pragma unroll
            for (int q = 1; q < KB; ++q) {
                const double x = (row[q] - u * sv[q]) * dinv;
                sv[q] += coef * x;
                row[q] = x;
            }
        }
    }
    if (bad) atomicOr(a.status, SX_STATUS_NOT_PD);
}

// Columns 64 blockIdx.x .. of W22, one lane per column c, KB stages: rows i = 64 blockIdx.x .. m - 1 in order (above the diagonal
// the lane carries zeros, which the recursion keeps), the running sums sX[s][c] in registers; the row's scalars are the same
// for every lane.  The rows above the block are written as zeros.  The scalars of drop_rows_ahead(KB) rows at a time go through
// LDS, where every lane reads the same word; they are fetched into registers a group ahead, beside the group's rows of W22,
// so that no load waits behind the stores of the rows in work.  (The rows past m of the last group meet zeros for scalars.)
template <int KB, bool MM = false>
__global__ __launch_bounds__(kDT) void drop_main_kernel(typename DropArg<MM>::type arg) {
    constexpr int kDropRowsAhead = drop_rows_ahead(KB);
    constexpr int kGroup = kDropRowsAhead * KB * 3;      // scalars of a group of rows
    constexpr int kPer = (kGroup + kDT - 1) / kDT;       // ... per lane
    __shared__ double T[kPer * kDT];
    const auto& a = DropArg<MM>::entry(arg, blockIdx.y);
    const int d = DropArg<MM>::output(arg, blockIdx.y), lane = threadIdx.x, n = a.n, k = a.k, m = a.m, c0 = blockIdx.x * kDT,
              c = c0 + lane;
    if constexpr (MM) {
        if ((int)blockIdx.x >= a.blocks) return;   // beyond this problem's column blocks (uniform)
    }
    const double* W = a.w_old + (size_t)d * n * n + (size_t)k * n + k;   // W22, leading dimension n
    const double* tab = a.tab + (size_t)d * m * KB * 3;
    double* W2 = a.w_new + (size_t)d * m * m;
    if (c < m)
        for (int i = 0; i < c0; ++i) W2[(size_t)i * m + c] = 0.0;
    double sx[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) sx[s] = 0.0;
    const int64_t tab_end = (int64_t)m * KB * 3;
    double cur[kDropRowsAhead], nxt[kDropRowsAhead], tnx[kPer];
    const auto load = [&](double (&dst)[kDropRowsAhead], int i0) {
#pragma unroll
        for (int j = 0; j < kDropRowsAhead; ++j) {
            const int i = i0 + j;
            dst[j] = (i < m && c <= i) ? W[(size_t)i * n + c] : 0.0;   // (c <= i < m: inside W22)
        }
    };
    const auto load_tab = [&](int i0) {
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int e = lane + u * kDT;
            const int64_t at = (int64_t)i0 * KB * 3 + e;
            tnx[u] = (e < kGroup && at < tab_end) ? tab[at] : 0.0;
        }
    };
    load(cur, c0);
    load_tab(c0);
    for (int i0 = c0; i0 < m; i0 += kDropRowsAhead) {
        __builtin_amdgcn_wave_barrier();   // (one wave: the last group's reads of T are done)
#pragma unroll
        for (int u = 0; u < kPer; ++u) T[lane + u * kDT] = tnx[u];
        __builtin_amdgcn_wave_barrier();
        load(nxt, i0 + kDropRowsAhead);
        load_tab(i0 + kDropRowsAhead);
#pragma unroll
        for (int j = 0; j < kDropRowsAhead; ++j) {
            const int i = i0 + j;
            const double* ti = T + j * KB * 3;
            double x = cur[j];
#pragma unroll
            for (int s = 0; s < KB; ++s) {
                x = (x - ti[3 * s] * sx[s]) * ti[3 * s + 1];
                sx[s] += ti[3 * s + 2] * x;
                // (the scalars of 16 stages at a time: fetched all at once they push the running sums out of the registers)
                if (KB > 16 && (s & 15) == 15) __builtin_amdgcn_sched_barrier(0);
            }
            if (c < m && i < m) W2[(size_t)i * m + c] = (c <= i) ? x : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kDropRowsAhead; ++j) cur[j] = nxt[j];
    }
}

// the wave's sum of v in a fixed order: lanes 32 apart, then 16, .. 1 (every lane ends with the sum)
__device__ __forceinline__ double drop_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// t = W' y2: wave w of workgroup b has row i = 4 b + w; lane l adds the columns l, l + 64, .. <= i in order
template <bool MM = false>
__global__ __launch_bounds__(kDThreads) void drop_t_kernel(typename DropArg<MM>::type arg) {
    const auto& a = DropArg<MM>::entry(arg, blockIdx.y);
    const int d = DropArg<MM>::output(arg, blockIdx.y), lane = threadIdx.x & 63, m = a.m,
              i = blockIdx.x * (kDThreads / 64) + (threadIdx.x >> 6);
    if constexpr (MM) {
        if ((int)blockIdx.x >= a.blocks4) return;   // beyond this problem's rows (uniform per workgroup)
    }
    if (i >= m) return;   // (uniform per wave; no barrier below)
    const double* row = a.w_new + (size_t)d * m * m + (size_t)i * m;
    double s = 0.0;
    for (int c = lane; c <= i; c += 64) s += row[c] * a.y[(size_t)c * a.n_s + d];
    s = drop_wave_sum(s);
    if (lane == 0) {
        a.t[(size_t)d * m + i] = s;
        if (!(s - s == 0.0)) atomicOr(a.status, SX_STATUS_NOT_PD);
    }
}

// alpha' = W'^T t for the columns 64 blockIdx.x ..: lane l of wave w adds the rows i >= c with i mod 4 = w in order, and the
// four classes are added in class order
template <bool MM = false>
__global__ __launch_bounds__(kDThreads) void drop_alpha_kernel(typename DropArg<MM>::type arg) {
    __shared__ double part[kDropAlphaWaves][kDT];
    const auto& a = DropArg<MM>::entry(arg, blockIdx.y);
    const int d = DropArg<MM>::output(arg, blockIdx.y), lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = a.m,
              c0 = blockIdx.x * kDT, c = c0 + lane;
    if constexpr (MM) {
        if ((int)blockIdx.x >= a.blocks) return;   // beyond this problem's column blocks (uniform; before the barrier)
    }
    const double* W2 = a.w_new + (size_t)d * m * m;
    const double* t = a.t + (size_t)d * m;
    double s = 0.0;
    if (c < m) {
        int i = c0 + wave;   // (c0 is a multiple of 4: i mod 4 = wave)
#pragma unroll 8
        for (; i < m; i += kDropAlphaWaves)
            if (i >= c) s += W2[(size_t)i * m + c] * t[i];
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < m) {
        double sum = part[0][lane];
#pragma unroll
        for (int w = 1; w < kDropAlphaWaves; ++w) sum += part[w][lane];
        a.alpha[(size_t)d * m + c] = sum;
    }
}

// logdet' = -sum log diag W': thread t adds the rows t, t + 256, .. in order, then the threads' sums in a fixed tree
template <bool MM = false>
__global__ __launch_bounds__(kDThreads) void drop_logdet_kernel(typename DropArg<MM>::type arg) {
    __shared__ double part[kDThreads];
    const auto& a = DropArg<MM>::entry(arg, blockIdx.x);
    const int d = DropArg<MM>::output(arg, blockIdx.x), tid = threadIdx.x, m = a.m;
    const double* W2 = a.w_new + (size_t)d * m * m;
    double s = 0.0;
    bool bad = false;
    for (int i = tid; i < m; i += kDThreads) {
        const double w = W2[(size_t)i * m + i];
        if (!(w > 0.0) || !(w - w == 0.0)) bad = true;
        s += log(w);
    }
    if (bad) atomicOr(a.status, SX_STATUS_NOT_PD);
    part[tid] = s;
    __syncthreads();
    for (int off = kDThreads / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) a.logdet[d] = -part[0];
}

}  // namespace sx
