// Warm path: sx_gp_select, the max-variance subset of a pool of training inputs (the reference's
// SimpleGPModel.choose_datapoints_maxvar, ssm_gpy/gaussian_process.py:279-344, with a deterministic tie rule).
//
// The greedy rule -- keep the pool point whose predictive variance under the points kept so far, summed over the
// outputs, is largest -- is a jointly pivoted Cholesky factorisation of the n_s matrices K_d + noise_d I.  Per output d:
// the residuals r_d[i] (s_d + noise_d at the start) and the factor columns C_d[j][i].  Step j, pivot p:
//     c = (k_d(x_i, x_p) + noise_d [i = p] - sum_{l<j} C_d[l][i] C_d[l][p]) / sqrt(r_d[p]),   C_d[j][i] = c,  r_d[i] -= c^2
//
// One plain launch per step, grid (ceil(n_max / 64), E): a one-wave workgroup owns 64 pool rows, a lane one row, and
// C_d is stored [m x n_max] with the row index fastest.  Nothing waits across workgroups inside a launch:
//   * every workgroup finds the pivot itself, from the per-workgroup (value, index) partials the previous launch left
//     (double-buffered by step parity), reduced in one total order: value descending, then index ascending;
//   * every lane recomputes r_d[p] from the pivot's own factor column, with the very operations (one fma per earlier
//     step, in step order) that its owner applied to the stored r_d[p], so that no lane reads a residual another
//     workgroup may be updating in the same launch, and all workgroups of a problem see the same bits and take the
//     same decisions (failure included).
// idx, sel_var and status are written by workgroup 0 of each problem.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"

namespace sx {

constexpr int kSelRows = 64;          // pool rows per workgroup: one wave
constexpr int kSelMaxN = 65536;       // pool rows per problem
constexpr int kSelMaxM = 4096;        // rows kept: what sx_gp_fit takes (kFitMaxN, sx_fit.hpp)
constexpr int kSelInitChunk = 8;      // problems whose constants one init launch carries as its argument

// One problem's constants: an entry of the device table at the start of the workspace (written by the init launch).
struct SelectEntry {
    double inv_ls2[SX_MAX_NS * SX_MAX_D];
    double outputscale[SX_MAX_NS];
    double noise[SX_MAX_NS];
    const double* x;   // [n x D] the pool
    int n, pad_;
};
static_assert(sizeof(SelectEntry) % sizeof(double) == 0, "the init launch copies the entry word by word");

// The workspace: the table [E], then per problem r [n_s x n_max], C [n_s x m x n_max], the partials' values
// [2 x nwg] and indices [2 x nwg], the chosen mask [n_max].  (Strides come from n_max, not from the problem's own n:
// a problem's arithmetic does not depend on them.)
struct SelectLayout {
    int64_t r, c, pval, pidx, chosen, per_problem, total;   // bytes (r .. chosen: from the start of a problem's part)
    int nwg;
    __host__ __device__ SelectLayout(int n_s, int E, int n_max, int m) {
        nwg = (n_max + kSelRows - 1) / kSelRows;
        int64_t off = 0;
        r = off;
        off += (int64_t)sizeof(double) * n_s * n_max;
        c = off;
        off += (int64_t)sizeof(double) * n_s * m * n_max;
        pval = off;
        off += (int64_t)sizeof(double) * 2 * nwg;
        pidx = off;
        off += (int64_t)sizeof(int32_t) * 2 * nwg;
        chosen = off;
        off += (int64_t)sizeof(int32_t) * n_max;
        per_problem = (off + 63) / 64 * 64;
        total = ((int64_t)sizeof(SelectEntry) * E + 63) / 64 * 64 + per_problem * E;
    }
    __host__ __device__ int64_t problem(int E, int e) const {
        return ((int64_t)sizeof(SelectEntry) * E + 63) / 64 * 64 + per_problem * e;
    }
};

struct SelectArgs {
    char* ws;                  // the workspace
    const int32_t* seed_idx;   // [E x n_seed] or null
    int32_t* idx;              // [E x m]
    double* sel_var;           // [E x m]
    int32_t* status;           // [E]
    int E, n_s, D, n_max, m, n_seed;
};

struct SelectInitArgs {
    SelectEntry entry[kSelInitChunk];
    int e0;                    // the chunk's first problem
};

// A candidate of the argmax: the summed residual and the row; i < 0: none.  `better` is a total order (value
// descending with NaN last, then index ascending), so the result of a reduction does not depend on its shape.
struct SelCand {
    double v;
    int i;
};
__device__ __forceinline__ bool sel_better(const SelCand& a, const SelCand& b) {   // a before b?
    if (a.i < 0) return false;
    if (b.i < 0) return true;
    const double ka = (a.v != a.v) ? -__builtin_huge_val() : a.v, kb = (b.v != b.v) ? -__builtin_huge_val() : b.v;
    return ka > kb || (ka == kb && a.i < b.i);
}
__device__ __forceinline__ SelCand sel_wave_best(SelCand c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        SelCand o;
        o.v = __shfl_xor(c.v, off);
        o.i = __shfl_xor(c.i, off);
        if (sel_better(o, c)) c = o;
    }
    return c;
}

// the init launch: the table, r = s_d + noise_d, the mask, step 0's partials, idx = -1 and sel_var = NaN
__global__ __launch_bounds__(kSelRows) void gp_select_init_kernel(SelectArgs a, SelectInitArgs ia) {
    const int e = ia.e0 + blockIdx.y, lane = threadIdx.x;
    const SelectEntry& t = ia.entry[blockIdx.y];
    const int n = t.n, base = blockIdx.x * kSelRows;
    if (base >= n) return;
    const SelectLayout lay(a.n_s, a.E, a.n_max, a.m);
    char* ws = a.ws + lay.problem(a.E, e);
    if (blockIdx.x == 0) {
        const double* src = reinterpret_cast<const double*>(&t);
        double* dst = reinterpret_cast<double*>(a.ws + sizeof(SelectEntry) * (size_t)e);
        for (int w = lane; w < (int)(sizeof(SelectEntry) / sizeof(double)); w += kSelRows) dst[w] = src[w];
        for (int j = lane; j < a.m; j += kSelRows) {
            a.idx[(size_t)e * a.m + j] = -1;
            a.sel_var[(size_t)e * a.m + j] = __builtin_nan("");
        }
    }
    const int i = base + lane;
    double* r = reinterpret_cast<double*>(ws + lay.r);
    SelCand c;
    c.v = 0.0;
    c.i = i < n ? i : -1;
    for (int d = 0; d < a.n_s; ++d) {
        const double prior = t.outputscale[d] + t.noise[d];
        if (i < n) r[(size_t)d * a.n_max + i] = prior;
        c.v += prior;
    }
    if (i < n) reinterpret_cast<int32_t*>(ws + lay.chosen)[i] = 0;
    c = sel_wave_best(c);
    if (lane == 0) {
        reinterpret_cast<double*>(ws + lay.pval)[blockIdx.x] = c.v;
        reinterpret_cast<int32_t*>(ws + lay.pidx)[blockIdx.x] = c.i;
    }
}

// step j of every problem
template <int NS>
__global__ __launch_bounds__(kSelRows) void gp_select_step_kernel(SelectArgs a, int j) {
    const int e = blockIdx.y, lane = threadIdx.x;
    const SelectEntry& t = reinterpret_cast<const SelectEntry*>(a.ws)[e];
    const int n = t.n, base = blockIdx.x * kSelRows, D = a.D, m = a.m;
    if (base >= n) return;
    if (a.status[e] & SX_STATUS_NOT_PD) return;
    const SelectLayout lay(NS, a.E, a.n_max, m);
    char* ws = a.ws + lay.problem(a.E, e);
    double* r = reinterpret_cast<double*>(ws + lay.r);
    double* C = reinterpret_cast<double*>(ws + lay.c);
    double* pval = reinterpret_cast<double*>(ws + lay.pval);
    int32_t* pidx = reinterpret_cast<int32_t*>(ws + lay.pidx);
    int32_t* chosen = reinterpret_cast<int32_t*>(ws + lay.chosen);
    const bool writer = blockIdx.x == 0 && lane == 0;

    // the pivot: the caller's seed, or the best of the partials the previous launch left
    int p;
    bool bad = false;
    if (j < a.n_seed) {
        const int32_t* seeds = a.seed_idx + (size_t)e * a.n_seed;
        p = seeds[j];
        bad = p < 0 || p >= n;
        for (int l = lane; l < j; l += kSelRows) bad = bad || seeds[l] == p;   // a repeated seed
        bad = __ballot(bad) != 0;
    } else {
        const int nwg = (n + kSelRows - 1) / kSelRows, par = (j & 1) * lay.nwg;
        SelCand best;
        best.v = 0.0;
        best.i = -1;
        for (int w = lane; w < nwg; w += kSelRows) {
            SelCand c;
            c.v = pval[par + w];
            c.i = pidx[par + w];
            if (sel_better(c, best)) best = c;
        }
        best = sel_wave_best(best);
        p = best.i;
        bad = p < 0 || p >= n;
    }
    p = __builtin_amdgcn_readfirstlane(p);
    if (bad) {
        if (writer) a.status[e] |= SX_STATUS_NOT_PD;
        return;
    }

    // the dot products with the pivot's factor column, and r_d[p] again from that column
    const int i = base + lane, ic = i < n ? i : n - 1;
    const size_t ld = (size_t)a.n_max, ldd = ld * m;
    double acc[NS], rp[NS];
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        acc[d] = 0.0;
        rp[d] = t.outputscale[d] + t.noise[d];
    }
    const double* Ci = C + ic;
    const double* Cp = C + p;
#pragma unroll 4
    for (int l = 0; l < j; ++l) {
#pragma unroll
        for (int d = 0; d < NS; ++d) {
            const double cp = Cp[d * ldd + l * ld], ci = Ci[d * ldd + l * ld];
            acc[d] = fma(ci, cp, acc[d]);
            rp[d] = fma(-cp, cp, rp[d]);
        }
    }
    double sel = 0.0;
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        if (!(rp[d] > 0.0)) bad = true;
        sel += rp[d];
    }
    if (bad) {   // the same bits in every lane of every workgroup of the problem: all leave here
        if (writer) a.status[e] |= SX_STATUS_NOT_PD;
        return;
    }
    if (writer) {
        a.idx[(size_t)e * m + j] = p;
        a.sel_var[(size_t)e * m + j] = sel;
    }

    // the new column, the residuals, the next step's partial
    SelCand cand;
    cand.v = 0.0;
    cand.i = -1;
    if (i < n) {
        const bool taken = chosen[i] != 0 || i == p;
        if (i == p) chosen[i] = 1;
#pragma unroll
        for (int d = 0; d < NS; ++d) {
            const double k = gp_kernel_value(t, d, D, i, p) + (i == p ? t.noise[d] : 0.0);
            const double c = (k - acc[d]) / sqrt(rp[d]);
            C[d * ldd + (size_t)j * ld + i] = c;
            const double rn = fma(-c, c, r[d * ld + i]);
            r[d * ld + i] = rn;
            cand.v += rn;
        }
        if (!taken) cand.i = i;
    }
    cand = sel_wave_best(cand);
    if (lane == 0) {
        const int par = ((j + 1) & 1) * lay.nwg;
        pval[par + blockIdx.x] = cand.v;
        pidx[par + blockIdx.x] = cand.i;
    }
}

}  // namespace sx
