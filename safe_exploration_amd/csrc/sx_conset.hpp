// The SafeMPC constraint set of a safety rollout (sx_con_set, include/sx_amd.h): the feedback
// bounds on the control ellipsoid (k_ff_t, K Q_t K^T) and the obstacle polytope on the intermediate safety ellipsoids.
// The two device functions the eval kernel (sx_conset_eval) and the _cons rollouts share, the constants and how the host
// fills and checks them.  Restates (in our own form) _generate_control_constraint and the obstacle rows of
// safempc_simple.py:325-396,492-536 of the reference as penalties; checked against tests/conset_oracle.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sx_amd.h"
#include "sx_reach.hpp"

namespace sx {

template <int NS>
struct ConConst {
    double h_mat_obs[SX_MAX_M * NS];   // rows past m_obs zero
    double h_obs[SX_MAX_M];
    int m_obs, ctrl_ellipsoid;
};

// m_obs, ctrl_ellipsoid and the constants of the rows in use as the entries answer SX_ERR_ARG for them
inline bool con_set_ok(const sx_con_set* cons, int ns) {
    if (!cons || ns < 1 || ns > SX_MAX_NS) return false;
    if (cons->m_obs < 0 || cons->m_obs > SX_MAX_M) return false;
    if (cons->ctrl_ellipsoid != 0 && cons->ctrl_ellipsoid != 1) return false;
    for (int i = 0; i < cons->m_obs * ns; ++i)
        if (!std::isfinite(cons->h_mat_obs[i])) return false;
    for (int r = 0; r < cons->m_obs; ++r)
        if (!std::isfinite(cons->h_obs[r])) return false;
    return true;
}

// (sx_con_set keeps its rows n_s apart, as sx_env keeps h_mat)
template <int NS>
void make_con_const(const sx_con_set* cons, ConConst<NS>& k) {
    k = ConConst<NS>{};
    k.m_obs = cons->m_obs;
    k.ctrl_ellipsoid = cons->ctrl_ellipsoid;
    for (int i = 0; i < cons->m_obs * NS; ++i) k.h_mat_obs[i] = cons->h_mat_obs[i];
    for (int r = 0; r < cons->m_obs; ++r) k.h_obs[r] = cons->h_obs[r];
}

// Is the control ellipsoid (u, Q_u = K Q K^T) of a step that starts from the ellipsoid (., Q) NOT certified inside the box?
// polytope_violated of (u, Q_u) over h = [I; -I], h_vec = [u_max; -u_min], c_safety = 1, spelled out so that the 2 n_u
// rows unroll: some +-u_c + sqrt(Q_u[c][c]) -+ bound_c >= 0; a NaN distance is not a violation.  n_u n_s (n_s + n_u) FMAs.
template <int NS, int NU>
__device__ __forceinline__ bool ctrl_ellipsoid_violated(const double* kfb, const double* u_min, const double* u_max,
                                                        const double (&u)[NU], const double (&Q)[NS][NS]) {
    double KQ[NU][NS], Qu[NU][NU];
#pragma unroll
    for (int c = 0; c < NU; ++c)
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < NS; ++i) s = fma(kfb[c * NS + i], Q[i][j], s);
            KQ[c][j] = s;
        }
#pragma unroll
    for (int c = 0; c < NU; ++c)
#pragma unroll
        for (int d = 0; d < NU; ++d) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) s = fma(KQ[c][j], kfb[d * NS + j], s);
            Qu[c][d] = s;
        }
    bool viol = false;
#pragma unroll
    for (int r = 0; r < 2 * NU; ++r) {
        // row r of [I; -I]: sign e_c
        const int c = r < NU ? r : r - NU;
        const double sign = r < NU ? 1.0 : -1.0;
        double hc = 0.0, hq = 0.0;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const double hi = (i == c) ? sign : 0.0;
            hc += hi * u[i];
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NU; ++j) s += Qu[i][j] * ((j == c) ? sign : 0.0);
            hq += hi * s;
        }
        const double d = hc + sqrt(hq) - (r < NU ? u_max[c] : -u_min[c]);
        viol = viol || (d >= 0.0);
    }
    return viol;
}

// The strict box test of the rollouts' action cost
template <int NU>
__device__ __forceinline__ bool action_box_violated(const double* u_min, const double* u_max, const double (&u)[NU]) {
    bool uviol = false;
#pragma unroll
    for (int c = 0; c < NU; ++c) uviol = uviol || (u[c] < u_min[c]) || (u[c] > u_max[c]);
    return uviol;
}

// One particle per lane: con_step[p] = the action cost of a step with action u[p] that starts from the ellipsoid
// (., q_start[p]) (a point where q_start is NULL) + the obstacle cost of the ellipsoid (p_next[p], q_next[p]) it reaches
template <int NS, int NU>
__global__ __launch_bounds__(256) void conset_eval_kernel(const ReachConst<NS, NU> rc, const CostConst<SX_MAX_M, NS, NU> cc,
                                                          const ConConst<NS> cons, int P, const double* __restrict__ u,
                                                          const double* __restrict__ q_start,
                                                          const double* __restrict__ p_next,
                                                          const double* __restrict__ q_next, int check_obstacle,
                                                          double* __restrict__ con_step) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double a[NU];
#pragma unroll
    for (int c = 0; c < NU; ++c) a[c] = u[p * NU + c];
    bool aviol = action_box_violated<NU>(cc.u_min, cc.u_max, a);
    if (cons.ctrl_ellipsoid && q_start) {
        double Q[NS][NS];
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) Q[i][j] = q_start[(p * NS + i) * NS + j];
        aviol = ctrl_ellipsoid_violated<NS, NU>(rc.kfb, cc.u_min, cc.u_max, a, Q) || aviol;
    }
    double con = aviol ? SX_ACTION_VIOLATION_COST : 0.0;
    if (check_obstacle && cons.m_obs > 0) {
        double p1[NS], Q1[NS][NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            p1[i] = p_next[p * NS + i];
#pragma unroll
            for (int j = 0; j < NS; ++j) Q1[i][j] = q_next[(p * NS + i) * NS + j];
        }
        if (polytope_violated<SX_MAX_M, NS>(cons.h_mat_obs, cons.h_obs, cons.m_obs, 1.0, p1, Q1, nullptr))
            con += SX_STATE_VIOLATION_COST;
    }
    con_step[p] = con;
}

}  // namespace sx
