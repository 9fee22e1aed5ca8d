// The performance trajectory of the CEM solver with first-order (Taylor) uncertainty propagation
// (sx_cem_perf_rollout_taylor): the variance form (sx_perf_var.hpp) with the state covariance carried from step to step
// under the fixed feedback K = k_fb of the safety rollout.  Per particle, Sigma_0 = 0:
//     (mean_t, var_t, J_t) = GP posterior and mean Jacobian at [mu_t, v_t],   J_t = [J_x | J_u]
//     M = J_x + J_u K,   H = (a + b K) + M
//     G_t = diag(var_t) + M Sigma_t M^T           (the objective and perf_sigma see diag G_t)
//     mu_{t+1} = a mu_t + b v_t + mean_t,         Sigma_{t+1} = H Sigma_t H^T + diag(var_t)
// (reference uncertainty_propagation_casadi.py:11-149 multiplied out; DESIGN.md 3.9 "Taylor form").  Optionally the
// ellipsoid (mu_s, Sigma_s), s = H + 2, is checked against the safe polytope (safempc_simple.py:471-479).
//
// Layout: the variance kernel's, statement by statement -- Kstar(t) |sync| MFMA(t) |sync| tail on the 16 owner lanes beside
// Kstar(t + 1) -- with three changes: gp_collect assembles the Jacobian rows the stage stream carries anyway, the owner lane
// holds Sigma (n_s x n_s, both triangles: the upper one is computed and mirrored) next to mu, and the tail does the
// 4 n_s^3 + O(n_s^2 n_u) FMAs above.  The mean recursion is the variance kernel's fma chain: mu is bit-identical to it.
// The constants of a step (prior, a + b K, K, action box, objective, polytope: 64 .. 128 doubles) sit in LDS behind the
// tile's actions; as kernel arguments they would stay in SGPRs for the whole kernel, which already spills its arguments.
// A tile's numbers depend on its 16 particles alone.
// The kernel is cem_perf_gp_rollout_kernel (sx_perf_var.hpp) of kind PerfTaylorKind: the variance kernels' body with its
// Taylor sections, single-model and multi-model (sx_cem_perf_rollout_taylor_multi: a GP per problem) alike.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_perf_var.hpp"   // PerfVarPtrs, kPerfVarThreads
#include "sx_reach.hpp"      // polytope_violated
#include "sx_sat_cost.hpp"   // SatConst, sat_loss

namespace sx {

template <int NS, int NU>
struct PerfTaylorConst {
    PerfStepConst<NS, NU> step;
    double abk[NS * NS];             // a + b K
    double k_fb[NU * NS];
    double h_mat[SX_MAX_M * NS];
    double h_vec[SX_MAX_M];
};

struct PerfTaylorPtrs : PerfVarPtrs {   // perf_sigma: diag G_t
    double* perf_cov;    // [E x P x n_perf x NS x NS] | NULL: Sigma_1 .. Sigma_{n_perf}
    int m;               // polytope rows
    int safety_step;     // t whose (mu_{t+1}, Sigma_{t+1}) is checked against the polytope (H + 1), or -1
};

// The same kernels with the saturating cost (sx_sat_cost.hpp) as the objective (sx_cem_perf_rollout_taylor_sat[_multi]).
// The cost's constants ride behind the step constants in one kernel argument and stay there: the owner lanes read them by
// scalar loads, and the LDS plan is the same.
template <int NS, int NU>
struct PerfTaylorSatConst {
    PerfTaylorConst<NS, NU> tc;
    SatConst<NS> sat;
};

// (the launcher of the multi-model kernel over the device table, instantiated beside it in sx_perf_taylor_sat_multi.hip, as
// sx_perf_launch.hpp declares the parents')
template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const PerfTaylorSatConst<NS, NU>& c, const PerfTaylorPtrs& tp,
                         bool byout, unsigned blocks, size_t lds, hipStream_t stream);

// The Taylor kinds of cem_perf_gp_rollout_kernel (sx_perf_var.hpp): its Taylor sections, and with SAT the saturating cost
template <bool SAT_>
struct PerfTaylorKind {
    static constexpr bool TAYLOR = true, SAT = SAT_;
    template <int NS, int NU>
    using Const = std::conditional_t<SAT_, PerfTaylorSatConst<NS, NU>, PerfTaylorConst<NS, NU>>;
    using Ptrs = PerfTaylorPtrs;
};

}  // namespace sx
