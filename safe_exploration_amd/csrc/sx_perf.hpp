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

template <int NS, int NU>
__global__ __launch_bounds__(kPerfThreads) void cem_perf_rollout_kernel(const PerfConst<NS, NU> pc, const PerfPtrs pp) {
    constexpr bool MM = false;
    const PerfStepConst<NS, NU>& step = pc.step;
#include "sx_perf_body.inc"
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

// sx_cem_perf_rollout_multi: the workgroup binds its problem's entry through a restrict-qualified pointer into the
// constant address space (the kernel never writes the table), so every field is a scalar load.
template <int NS, int NU>
__global__ __launch_bounds__(kPerfThreads) void cem_perf_rollout_multi_kernel(const PerfGpEntry<NS, NU>* __restrict__ table,
                                                                              const PerfStepConst<NS, NU> step,
                                                                              const PerfPtrs pp) {
    constexpr bool MM = true;
    using ConstE = __attribute__((address_space(4))) const PerfGpEntry<NS, NU>;
    const PerfGpEntry<NS, NU>& pc =
        *(const PerfGpEntry<NS, NU>*)((ConstE*)table + (int)blockIdx.x / ((pp.P + kPerfTile - 1) / kPerfTile));
#include "sx_perf_body.inc"
}

// Launches cem_perf_rollout_kernel<NS, NU> on `stream`; SX_ERR_UNSUPPORTED where the training set does not fit the LDS
// or the particles exceed a grid.  Instantiated in sx_perf.hip for every shift-0 shape of SX_ROLLOUT_SHAPES.
template <int NS, int NU>
int launch_perf_rollout(const PerfConst<NS, NU>& pc, const PerfPtrs& pp, hipStream_t stream);

// Launches cem_perf_rollout_multi_kernel<NS, NU> over pp.E problems with a GP each (`table`: the device array of their
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
