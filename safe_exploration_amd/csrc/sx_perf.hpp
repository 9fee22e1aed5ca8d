// The performance trajectory of the CEM solver (sx_cem_perf_rollout): n_perf chained mean-equivalent steps per particle,
//     mu_{t+1} = a mu_t + b v_t + mean_GP([mu_t, v_t]),      mean_d(z) = sum_i alpha_d[i] s_d exp(-1/2 |z - X_i|^2_{l_d}),
// no variance, no feedback term (reference uncertainty_propagation_casadi.py:152-245 with sigma_x = None).  A step needs
// k* . alpha only -- O(N D) per particle -- where a safety step needs the N x N triangular product.
//
// Layout.  The chain over t is sequential, so the parallelism inside a step comes from the training points: a particle
// owns kPerfLanes = 16 lanes of a wave (4 particles per wave, 16 per 256-thread workgroup), lane j of the particle sums
// the points i = j, j + 16, j + 32, ... (two per trip: 2 n_s exponential chains in flight, exp_tab_f64_n as in the Kstar
// phase of the safety kernels), and an xor butterfly over the 16 lanes (8, 4, 2, 1: a fixed order, the same sum in all 16
// lanes) finishes the mean.  Every lane of the particle then carries mu, the costs and the status redundantly; lane 0
// writes.  The number of lanes per particle is a constant of the kernel, never of the launch: a particle's numbers do
// not depend on P, on the grid or on the workgroup it lands in.
//
// The training inputs (transposed to [D][n_pad]: the 16 lanes of a particle read 128 contiguous bytes, the 4 particles of a
// wave the same ones), alpha [n_s][n_pad] and the 2^(j/256) table live in LDS; n_pad = N rounded up to 32 with zero
// rows, whose alpha is zero too: no remainder loop, no index clamp.  Step t + 1's action is loaded before step t's sum.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"

namespace sx {

constexpr int kPerfLanes = 16;                        // lanes per particle
constexpr int kPerfThreads = 256;
constexpr int kPerfTile = kPerfThreads / kPerfLanes;  // particles per workgroup
constexpr int kPerfUnroll = 2;                        // training points per lane and trip
constexpr int kPerfPad = kPerfLanes * kPerfUnroll;    // n_pad is a multiple of this

// The constants of a step's tail (prior, objective, action box), read once per step: kept in LDS behind the table -- as
// kernel arguments they would sit in SGPRs for the whole kernel, and the (4, n_u) shapes would spill them.
template <int NS, int NU>
struct PerfStepConst {
    double a[NS * NS];
    double b[NS * NU];
    double u_min[NU];
    double u_max[NU];
    double w_abs[NS];
    double target[NS];
    double w_lin[NS];
};

template <int NS, int NU>
struct PerfConst {
    double k_nh_ils2[NS * (NS + NU)];   // -1 / (2 l^2) * 256 / ln 2 (the exponent in the units of exp_tab_f64_n)
    double k_log_os[NS];                // ln(outputscale) * 256 / ln 2
    PerfStepConst<NS, NU> step;
    const double* x_train;              // dev [N x D]
    const double* alpha;                // dev [NS x N]
    int n_train;
    int n_pad;
};

struct PerfPtrs {
    const double* x0;            // [E x NS]
    const double* safe_actions;  // [E x P x H x NU]
    const double* tail_mean;     // [E x T x NU]
    const double* tail_std;
    const double* tail_noise;    // [E x P x T x NU] | NULL: the tail of `rows` is an input
    double* rows;                // [E x P x (H + T) x NU]
    double* obj_cost;            // [E x P] overwritten
    double* con_cost;            // [E x P] added to
    double* perf_traj;           // [E x P x n_perf x NS] | NULL
    int* status;
    int E, P, H, n_perf, r;
};

inline int perf_n_pad(int n_train) { return (n_train + kPerfPad - 1) / kPerfPad * kPerfPad; }
inline size_t perf_lds_bytes(int ns, int nu, int n_train) {
    const size_t step = (size_t)ns * ns + ns * nu + 2 * nu + 3 * ns;   // PerfStepConst
    return ((size_t)(2 * ns + nu) * perf_n_pad(n_train) + kExpTab + step) * sizeof(double);
}

// The training rows i0 + sub and i0 + sub + 16 and their alphas (`xl`, `all`: the LDS arrays at this lane's sub index).
template <int NS, int D>
__device__ __forceinline__ void perf_load_trip(const lds_f64* xl, const lds_f64* all, int n_pad, int i0,
                                               double (&x)[kPerfUnroll][D], double (&a)[kPerfUnroll][NS]) {
#pragma unroll
    for (int h = 0; h < kPerfUnroll; ++h) {
#pragma unroll
        for (int j = 0; j < D; ++j) x[h][j] = xl[j * n_pad + i0 + h * kPerfLanes];
#pragma unroll
        for (int d = 0; d < NS; ++d) a[h][d] = all[d * n_pad + i0 + h * kPerfLanes];
    }
}

// The GP part of PerfConst for one problem of the multi-model launch: an entry of the device table sx_cem_perf_table
// builds (alpha is not part of the packed sx_gp_model, hence a table of its own).
template <int NS, int NU>
struct PerfGpEntry {
    double k_nh_ils2[NS * (NS + NU)];
    double k_log_os[NS];
    const double* x_train;   // dev [N x D]
    const double* alpha;     // dev [NS x N]
    int n_train;
    int n_pad;
};

// The one mean-only kernel: (PerfConst, PerfPtrs), or with MM (table, PerfStepConst, PerfPtrs) -- STEP... is that one middle
// argument, named explicitly by whoever names the kernel.  With MM the grid is problem-aligned, E x ceil(P / kPerfTile)
// workgroups, so that a workgroup stages ONE problem's training inputs and alpha with that problem's n_pad inside the
// launch's allocation for the largest model; a slot past P in a problem's last tile computes on the problem's first
// particle and writes nothing; pp.status holds E words.  The workgroup binds its problem's entry through a pointer into the
// constant address space (the table is restrict-qualified and the kernel never writes it), so every field is a scalar load.
template <int NS, int NU, bool MM = false, class... STEP>
__global__ __launch_bounds__(kPerfThreads) void cem_perf_rollout_kernel(
    const std::conditional_t<MM, const PerfGpEntry<NS, NU>* __restrict__, PerfConst<NS, NU>> model, const STEP... step_arg,
    const PerfPtrs pp) {
    static_assert(sizeof...(STEP) == (MM ? 1 : 0), "STEP... is the multi-model kernel's PerfStepConst<NS, NU>");
    // `pc`, the GP part (k_nh_ils2, k_log_os, x_train, alpha, n_train, n_pad), and `step`, the step constants.  (The
    // spelling is what keeps either mode's instructions: the binding must not take `pp` by reference, and the single-model
    // `pc` must be the argument itself, not a pointer to it; tools/device_code_diff.py is the check.)
    int problem = 0;
    if constexpr (MM) problem = (int)blockIdx.x / ((pp.P + kPerfTile - 1) / kPerfTile);
    const auto& pc = [&]() -> decltype(auto) {
        if constexpr (MM) {
            using ConstE = __attribute__((address_space(4))) const PerfGpEntry<NS, NU>;
            return *(const PerfGpEntry<NS, NU>*)((ConstE*)model + problem);
        } else {
            return (model);
        }
    }();
    const PerfStepConst<NS, NU>& step = [&](const auto&... s) -> const PerfStepConst<NS, NU>& {
        if constexpr (MM) return (s, ...);
        else return pc.step;
    }(step_arg...);
    constexpr int D = NS + NU;
    extern __shared__ __attribute__((aligned(16))) double perf_lds[];
    const int n_pad = pc.n_pad;
    double* xs = perf_lds;                // [D][n_pad]
    double* al = xs + (size_t)D * n_pad;  // [NS][n_pad]
    double* etab = al + (size_t)NS * n_pad;
    for (int idx = threadIdx.x; idx < n_pad * D; idx += kPerfThreads) {
        const int i = idx / D, c = idx - i * D;
        xs[c * n_pad + i] = i < pc.n_train ? pc.x_train[idx] : 0.0;
    }
    for (int idx = threadIdx.x; idx < n_pad * NS; idx += kPerfThreads) {
        const int d = idx / n_pad, i = idx - d * n_pad;
        al[idx] = i < pc.n_train ? pc.alpha[(size_t)d * pc.n_train + i] : 0.0;
    }
    if (threadIdx.x < kExpTab) etab[threadIdx.x] = kExp2Tab[threadIdx.x];
    constexpr int kStepDoubles = (int)(sizeof(PerfStepConst<NS, NU>) / sizeof(double));
    static_assert(kStepDoubles <= kPerfThreads, "one thread per constant");
    if (threadIdx.x < kStepDoubles) etab[kExpTab + threadIdx.x] = reinterpret_cast<const double*>(&step)[threadIdx.x];
    __syncthreads();
    typedef __attribute__((address_space(3))) const PerfStepConst<NS, NU> LdsStep;
    LdsStep& sc = *(LdsStep*)(etab + kExpTab);

    const int sub = (int)threadIdx.x & (kPerfLanes - 1);
    int64_t g, gg;   // the particle of the launch; the one this slot reads through
    bool valid;
    int e;
    if constexpr (MM) {
        const int tiles_per_problem = (pp.P + kPerfTile - 1) / kPerfTile;
        e = (int)blockIdx.x / tiles_per_problem;
        const int c = ((int)blockIdx.x - e * tiles_per_problem) * kPerfTile + ((int)threadIdx.x / kPerfLanes);
        valid = c < pp.P;
        g = (int64_t)e * pp.P + c;
        gg = valid ? g : (int64_t)e * pp.P;   // a slot past P reads through the problem's first particle and writes nothing
    } else {
        const int64_t total = (int64_t)pp.E * pp.P;
        g = (int64_t)blockIdx.x * kPerfTile + ((int)threadIdx.x / kPerfLanes);
        valid = g < total;
        gg = valid ? g : 0;   // a slot past the particles reads through the first one and writes nothing
        e = (int)(gg / pp.P);
    }
    const int H = pp.H, r = pp.r, n_perf = pp.n_perf, T = n_perf - r;
    const int64_t row_len = (int64_t)(H + T) * NU;
    const double* safe = pp.safe_actions + gg * H * NU;
    const double* t_mean = pp.tail_noise ? pp.tail_mean + (int64_t)e * T * NU : nullptr;
    const double* t_std = pp.tail_noise ? pp.tail_std + (int64_t)e * T * NU : nullptr;
    const double* t_noise = pp.tail_noise ? pp.tail_noise + gg * T * NU : nullptr;
    double* row = pp.rows + gg * row_len;

    // the particle's row: the safety actions as the safety rollout wrote them, then the tail
    if (valid) {
        for (int i = sub; i < H * NU; i += kPerfLanes) row[i] = safe[i];
        if (t_noise)
            for (int i = sub; i < T * NU; i += kPerfLanes) row[H * NU + i] = fma(t_std[i], t_noise[i], t_mean[i]);
    }
    // action c of performance step t: shared with the safety trajectory below r, the tail from there (drawn by the
    // same expression as the stored one, so that no lane waits for another lane's store)
    auto action = [&](int t, int c) -> double {
        if (t < r) return safe[t * NU + c];
        const int i = (t - r) * NU + c;
        return t_noise ? fma(t_std[i], t_noise[i], t_mean[i]) : row[H * NU + i];
    };

    double log_os[NS];
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        log_os[d] = pc.k_log_os[d];
        asm volatile("" : "+v"(log_os[d]));
    }
    double mu[NS], v[NU];
#pragma unroll
    for (int i = 0; i < NS; ++i) mu[i] = pp.x0[(int64_t)e * NS + i];
#pragma unroll
    for (int c = 0; c < NU; ++c) v[c] = action(0, c);
    double obj = 0.0, con = 0.0;
    int st = 0;
    const lds_f64* xl = (const lds_f64*)xs + sub;
    const lds_f64* all = (const lds_f64*)al + sub;
    const lds_f64* el = (const lds_f64*)etab;
    const int trips = n_pad / kPerfPad;
    for (int t = 0; t < n_perf; ++t) {
        double vn[NU];   // the next step's action travels while this step's sum runs
#pragma unroll
        for (int c = 0; c < NU; ++c) vn[c] = t + 1 < n_perf ? action(t + 1, c) : 0.0;
        double z[D], acc[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) z[j] = mu[j];
#pragma unroll
        for (int c = 0; c < NU; ++c) z[NS + c] = v[c];
#pragma unroll
        for (int d = 0; d < NS; ++d) acc[d] = 0.0;
        // the operands of trip k + 1 are read while trip k's exponentials run (one wave per SIMD at P = 4096: nobody
        // else hides the LDS latency); the read behind the last trip wraps to the first rows
        double xr[kPerfUnroll][D], ar[kPerfUnroll][NS];
        perf_load_trip<NS, D>(xl, all, n_pad, 0, xr, ar);
        for (int k = 0; k < trips; ++k) {
            double xc[kPerfUnroll][D], ac[kPerfUnroll][NS];
#pragma unroll
            for (int h = 0; h < kPerfUnroll; ++h) {
#pragma unroll
                for (int j = 0; j < D; ++j) xc[h][j] = xr[h][j];
#pragma unroll
                for (int d = 0; d < NS; ++d) ac[h][d] = ar[h][d];
            }
            perf_load_trip<NS, D>(xl, all, n_pad, k + 1 < trips ? (k + 1) * kPerfPad : 0, xr, ar);
            double arg[kPerfUnroll * NS], val[kPerfUnroll * NS];
#pragma unroll
            for (int h = 0; h < kPerfUnroll; ++h) {
                double sq[D];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const double df = z[j] - xc[h][j];
                    sq[j] = df * df;
                }
#pragma unroll
                for (int d = 0; d < NS; ++d) {
                    double a = log_os[d];
#pragma unroll
                    for (int j = 0; j < D; ++j) a = fma(sq[j], pc.k_nh_ils2[d * D + j], a);
                    arg[h * NS + d] = a;
                }
            }
            exp_tab_f64_n<kPerfUnroll * NS>(arg, val, el);
#pragma unroll
            for (int h = 0; h < kPerfUnroll; ++h)
#pragma unroll
                for (int d = 0; d < NS; ++d) acc[d] = fma(val[h * NS + d], ac[h][d], acc[d]);
        }
        // the 16 partial sums of the particle: xor butterfly, every lane ends with the same bits
#pragma unroll
        for (int d = 0; d < NS; ++d)
#pragma unroll
            for (int m = kPerfLanes / 2; m > 0; m >>= 1) acc[d] += __shfl_xor(acc[d], m, kPerfLanes);
        double mu1[NS];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double s = acc[i];
#pragma unroll
            for (int j = 0; j < NS; ++j) s += sc.a[i * NS + j] * mu[j];
#pragma unroll
            for (int c = 0; c < NU; ++c) s += sc.b[i * NU + c] * v[c];
            mu1[i] = s;
            bad = bad || !(__builtin_fabs(s) <= 1.7976931348623157e308);
        }
        if (bad) {
            // (the table exponential drops a NaN argument: a non-finite state stays one by hand)
            st |= SX_STATUS_NAN;
#pragma unroll
            for (int i = 0; i < NS; ++i) mu1[i] = __builtin_nan("");
        }
        double o = 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) o += sc.w_abs[i] * fabs(sc.target[i] - mu1[i]) + sc.w_lin[i] * mu1[i];
        obj += o;
        if (t >= r) {
            bool uviol = false;
#pragma unroll
            for (int c = 0; c < NU; ++c) uviol = uviol || (v[c] < sc.u_min[c]) || (v[c] > sc.u_max[c]);
            if (uviol) con += SX_ACTION_VIOLATION_COST;
        }
        if (valid && sub == 0 && pp.perf_traj) {
#pragma unroll
            for (int i = 0; i < NS; ++i) pp.perf_traj[(g * n_perf + t) * NS + i] = mu1[i];
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) mu[i] = mu1[i];
#pragma unroll
        for (int c = 0; c < NU; ++c) v[c] = vn[c];
    }
    if (valid && sub == 0) {
        pp.obj_cost[g] = obj;
        pp.con_cost[g] += con;
        if (st) atomicOr(pp.status + (MM ? e : 0), st);
    }
}

// Launches cem_perf_rollout_kernel<NS, NU> on `stream`; SX_ERR_UNSUPPORTED where the training set does not fit the LDS
// or the particles exceed a grid.  Instantiated in sx_perf.hip for every shift-0 shape of SX_ROLLOUT_SHAPES.
template <int NS, int NU>
int launch_perf_rollout(const PerfConst<NS, NU>& pc, const PerfPtrs& pp, hipStream_t stream);

// Launches cem_perf_rollout_kernel<NS, NU, true, ...> over pp.E problems with a GP each (`table`: the device array of their
// PerfGpEntry) with `lds` bytes, the largest perf_lds_bytes over the models; pp.status holds E words.  Instantiated in
// sx_perf_multi.hip.
template <int NS, int NU>
int launch_perf_rollout_multi(const PerfGpEntry<NS, NU>* table, const PerfStepConst<NS, NU>& step, const PerfPtrs& pp,
                              size_t lds, hipStream_t stream);

// The step constants of a launch from the sx_env (host)
template <int NS, int NU>
inline void make_perf_step(const sx_env* env, PerfStepConst<NS, NU>& sc) {
    for (int i = 0; i < NS * NS; ++i) sc.a[i] = env->a[i];
    for (int i = 0; i < NS * NU; ++i) sc.b[i] = env->b[i];
    for (int c = 0; c < NU; ++c) {
        sc.u_min[c] = env->u_min[c];
        sc.u_max[c] = env->u_max[c];
    }
    for (int i = 0; i < NS; ++i) {
        sc.w_abs[i] = env->obj_w_abs[i];
        sc.target[i] = env->obj_target[i];
        sc.w_lin[i] = env->obj_w_lin[i];
    }
}

}  // namespace sx
