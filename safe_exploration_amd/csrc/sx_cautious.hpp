// The chance-constrained Taylor rollout of Cautious MPC (sx_cem_cautious_rollout): the trajectory of the Taylor form
// (sx_perf_taylor.hpp) on its own -- no safety rollout in front of it, rows of T feed-forward controls k_ff_0 .. k_ff_{T-1}
// -- with the reference's chance constraints on every step (generate_safety_constraints / _generate_control_constraint,
// cautious_mpc.py:337-442, at c_safety = beta).  Per particle, mu_0 = x0, Sigma_0 = 0, K = k_fb:
//     control   t = 0: k_ff_0 outside [u_min, u_max];   t >= 1: k_ff_t[c] +- beta sqrt(K_c Sigma_t K_c^T) against the box
//     (mean_t, var_t, J_t), M, Hm, G_t, mu_{t+1}, Sigma_{t+1}: the Taylor form's, statement by statement
//     state     some row j: h_j . mu_{t+1} + beta sqrt(h_j^T Sigma_{t+1} h_j) - h_vec_j >= 0
// d >= 0 violates and a NaN distance counts as inside (polytope_violated, sx_reach.hpp).  propagate == 0: the GP step starts
// from Sigma_t = 0 (G_t = var_t, Sigma_{t+1} = diag(var_t): one_step_mean_equivalent); the control constraint of step t
// still sees diag(var_{t-1}).
//
// Layout: the Taylor kernel's -- Kstar(t) |sync| MFMA(t) |sync| tail on the 16 owner lanes beside Kstar(t + 1), the step
// constants (the Taylor constants plus beta) in LDS behind the tile's actions -- with a body of its own: the rows are the
// actions (no [safety | tail] split), con_cost is overwritten, and the tail gains the constraint algebra:
// 2 m n_s^2 + 2 n_u n_s^2 FMAs and m + n_u square roots per step on the owner lane.  The covariance step is written as in
// sx_perf_gp_body.inc, fma for fma: with m = 0 and a wide box mu, diag G and Sigma are the Taylor kernel's bits.
// A tile's numbers depend on its 16 particles alone.
// The body is sx_cautious_body.inc, text that cem_cautious_sat_rollout_kernel includes too with its objective section.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_perf_taylor.hpp"   // PerfTaylorConst, PerfVarPtrs, kPerfVarThreads

namespace sx {

template <int NS, int NU>
struct CautiousConst {
    PerfTaylorConst<NS, NU> tc;
    double beta;
};

struct CautiousPtrs {
    PerfPtrs p;          // x0, tail_mean / tail_std / tail_noise (the row's distribution), rows, obj_cost, con_cost
                         // (overwritten), perf_traj, status; H = n_perf = T, r = 0, no safe_actions
    double* sigma;       // [E x P x T x NS] | NULL: diag G_t
    double* cov;         // [E x P x T x NS x NS] | NULL: Sigma_1 .. Sigma_T
    double* margins;     // [E x P x T x 2] | NULL: largest state row distance, largest control distance
    int obj_mode;
    int m;               // polytope rows
    int propagate;       // 0: mean-equivalent GP steps
};

template <int NS, int NU>
constexpr int cautious_const_doubles() {
    return (int)(sizeof(CautiousConst<NS, NU>) / sizeof(double));
}

template <int NS, int NU, bool BYOUT>
__global__ __launch_bounds__(kPerfVarThreads) void cem_cautious_rollout_kernel(const GpConst<NS, NS + NU> gc,
                                                                               const int4* __restrict__ stage_tab,
                                                                               const CautiousConst<NS, NU> cc_arg,
                                                                               const CautiousPtrs cp) {
#include "sx_cautious_body.inc"
}

// sx_cem_cautious_rollout_sat: the same body with the saturating cost (sx_sat_cost.hpp) as the objective; the cost's
// constants ride behind the step constants in one kernel argument and stay there (scalar loads on the owner lanes), so
// the LDS plan is the parent's.
template <int NS, int NU>
struct CautiousSatConst {
    CautiousConst<NS, NU> cc;
    SatConst<NS> sat;
};

template <int NS, int NU, bool BYOUT>
__global__ __launch_bounds__(kPerfVarThreads) void cem_cautious_sat_rollout_kernel(const GpConst<NS, NS + NU> gc,
                                                                                   const int4* __restrict__ stage_tab,
                                                                                   const CautiousSatConst<NS, NU> arg,
                                                                                   const CautiousPtrs cp) {
    const CautiousConst<NS, NU>& cc_arg = arg.cc;
    const SatConst<NS>& sat = arg.sat;
#define SX_CAUTIOUS_SAT
#include "sx_cautious_body.inc"
#undef SX_CAUTIOUS_SAT
}

}  // namespace sx
