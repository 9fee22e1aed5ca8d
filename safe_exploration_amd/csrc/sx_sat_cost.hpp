// The PILCO saturating cost of a state Gaussian (sx_sat_cost, include/sx_amd.h): the device function the eval kernel
// (sx_sat_cost_eval) and the three _sat rollouts share, its constants and how the host fills and checks them.
//     loss = 1 - exp(-q / 2) / prod diag L,   L = chol(I_k + V^T S~ V),   q = |L^-1 V^T (m~ - z)|^2
// over the trigonometric augmentation (m~, S~) of (mu, Sigma) at the angle index i.  S~ is never formed.  With
// J [n_a x n_s] the Jacobian of the augmentation at the moments (the rows of the kept states, c e_i^T for sin, -s e_i^T
// for cos; s = e0 sin mu_i, c = e0 cos mu_i),
//     S~ = J Sigma J^T + Delta,   Delta on the (sin, cos) block only:
//     D_ss = V_ss - c^2 Sigma_ii,   D_sc = V_sc + s c Sigma_ii,   D_cc = V_cc - s^2 Sigma_ii
// (Cov(x, sin) = Sigma[:, i] c and Cov(x, cos) = -Sigma[:, i] s are J Sigma J^T's own), so
//     V^T S~ V = Wm^T Sigma Wm + [vs vc] Delta [vs vc]^T,   Wm = J^T V [n_s x k]: the state rows of V, row i = c vs - s vc.
// The host lays V out by state (SatConst) with n_s + 1 columns, those past the rank zero: they leave their rows of S at the
// identity and their y at 0 -- no rank is needed for the value; the rank only skips their square roots and divisions.
// (Skipping them in the column sweep too made a full-rank launch 2 - 4 % slower: DESIGN.md 3.12.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "../../include/sx_amd.h"

namespace sx {

template <int NS>
struct SatConst {
    double zx[NS];            // target of state j (0 at the angle)
    double zs, zc;            // target of sin, cos
    double vx[NS][NS + 1];    // row of V of state j (zeros at the angle), columns past the rank zero
    double vs[NS + 1];        // row of V of sin
    double vc[NS + 1];        // row of V of cos
    int trig_idx, rank;
};

// trig_idx, rank and the constants as the entries answer SX_ERR_ARG for them
inline bool sat_cost_ok(const sx_sat_cost* cost, int ns) {
    if (!cost || ns < 1 || ns > SX_MAX_NS) return false;
    if (cost->trig_idx < -1 || cost->trig_idx >= ns) return false;
    const int na = cost->trig_idx < 0 ? ns : ns + 1;
    if (cost->rank < 1 || cost->rank > na) return false;
    for (int i = 0; i < na; ++i)
        if (!std::isfinite(cost->target[i])) return false;
    for (int i = 0; i < na * cost->rank; ++i)
        if (!std::isfinite(cost->v[i])) return false;
    return true;
}

template <int NS>
void make_sat_const(const sx_sat_cost* cost, SatConst<NS>& k) {
    k = SatConst<NS>{};
    const int ti = cost->trig_idx, rank = cost->rank;
    k.trig_idx = ti;
    k.rank = rank;
    int row = 0;   // row of m~: the states but the angle in order, then sin, cos
    for (int j = 0; j < NS; ++j) {
        if (j == ti) continue;
        k.zx[j] = cost->target[row];
        for (int a = 0; a < rank; ++a) k.vx[j][a] = cost->v[row * rank + a];
        ++row;
    }
    if (ti >= 0) {
        k.zs = cost->target[row];
        k.zc = cost->target[row + 1];
        for (int a = 0; a < rank; ++a) {
            k.vs[a] = cost->v[row * rank + a];
            k.vc[a] = cost->v[(row + 1) * rank + a];
        }
    }
}

// How the cost reaches F::make_const(env, c) through perf_gp_rollout (sx_perf_launch.hpp), which hands a form the sx_env
// alone: the _sat entries pass &SatEnv::env -- their copy of the caller's, with an obj_mode the parent's checks accept,
// since the entries do not read the caller's -- and the form steps back to the SatEnv around it (its first member).
struct SatEnv {
    sx_env env;
    const sx_sat_cost* cost;
};
static_assert(offsetof(SatEnv, env) == 0, "sat_cost_of steps from the env to the SatEnv around it");
inline SatEnv make_sat_env(const sx_env* env, const sx_sat_cost* cost) {
    SatEnv se{*env, cost};
    se.env.obj_mode = SX_OBJ_AFFINE_ABS;
    return se;
}
inline const sx_sat_cost* sat_cost_of(const sx_env* env) { return reinterpret_cast<const SatEnv*>(env)->cost; }

// loss(mu, Sigma); Sigma with both triangles.  `k` is uniform (a kernel argument: scalar loads).  About
// n_a (n_s^2 + n_s n_a / 2 + n_a^2 / 6) FMAs, one sincos, two exp, `rank` square roots and divisions.
template <int NS>
__device__ __forceinline__ double sat_loss(const SatConst<NS>& k, const double (&mu)[NS], const double (&S)[NS][NS]) {
    constexpr int K = NS + 1;
    const int ti = k.trig_idx;
    double s = 0.0, c = 0.0, dss = 0.0, dsc = 0.0, dcc = 0.0;
    if (ti >= 0) {
        double m = 0.0, v = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j == ti) {
                m = mu[j];
                v = S[j][j];
            }
        double s0, c0;
        sincos(m, &s0, &c0);
        const double e0 = exp(-0.5 * v);
        double e1 = e0 * e0;
        e1 *= e1;   // exp(-2 v)
        s = e0 * s0;
        c = e0 * c0;
        const double cos2 = (c0 - s0) * (c0 + s0), sin2 = 2.0 * s0 * c0;
        dss = (0.5 * (1.0 - e1 * cos2) - s * s) - c * c * v;
        dcc = (0.5 * (1.0 + e1 * cos2) - c * c) - s * s * v;
        dsc = (0.5 * e1 * sin2 - s * c) + s * c * v;
    }
    // y = V^T d and the upper triangle of A = I + V^T S~ V, column block by column block
    double y[K], A[K][K], wi[K];   // wi: row i of Wm
#pragma unroll
    for (int a = 0; a < K; ++a) wi[a] = c * k.vs[a] - s * k.vc[a];
    auto wm = [&](int j, int a) { return j == ti ? wi[a] : k.vx[j][a]; };
#pragma unroll
    for (int a = 0; a < K; ++a) {
        double ya = k.vs[a] * (s - k.zs) + k.vc[a] * (c - k.zc);
#pragma unroll
        for (int j = 0; j < NS; ++j) ya = fma(k.vx[j][a], mu[j] - k.zx[j], ya);
        y[a] = ya;
        double u[NS];   // Sigma Wm[:, a]
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) t = fma(S[i][j], wm(j, a), t);
            u[i] = t;
        }
        const double ts = dss * k.vs[a] + dsc * k.vc[a], tc = dsc * k.vs[a] + dcc * k.vc[a];
#pragma unroll
        for (int b = a; b < K; ++b) {
            double t = fma(ts, k.vs[b], tc * k.vc[b]);
#pragma unroll
            for (int i = 0; i < NS; ++i) t = fma(u[i], wm(i, b), t);
            A[a][b] = (b == a) ? 1.0 + t : t;
        }
    }
    // L^T in the upper triangle (row a: L[b][a], b >= a), q = |L^-1 y|^2 and the product of the diagonal on the way
    double q = 0.0, det = 1.0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        if (a < k.rank) {
            double d = A[a][a], ya = y[a];
#pragma unroll
            for (int p = 0; p < a; ++p) {
                d = fma(-A[p][a], A[p][a], d);
                ya = fma(-A[p][a], y[p], ya);
            }
            const double l = sqrt(d), inv = 1.0 / l;
            det *= l;
            ya *= inv;
            y[a] = ya;
            q = fma(ya, ya, q);
#pragma unroll
            for (int b = a + 1; b < K; ++b) {
                double t = A[a][b];
#pragma unroll
                for (int p = 0; p < a; ++p) t = fma(-A[p][a], A[p][b], t);
                A[a][b] = t * inv;
            }
        }
    }
    return 1.0 - exp(-0.5 * q) / det;
}

// One particle per lane: loss[p] = sat_loss(mu[p], cov[p])
template <int NS>
__global__ __launch_bounds__(256) void sat_cost_eval_kernel(const SatConst<NS> k, int P, const double* __restrict__ mu,
                                                            const double* __restrict__ cov, double* __restrict__ loss,
                                                            int32_t* __restrict__ status) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double m[NS], S[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        m[i] = mu[p * NS + i];
#pragma unroll
        for (int j = 0; j < NS; ++j) S[i][j] = cov[(p * NS + i) * NS + j];
    }
    double l = sat_loss<NS>(k, m, S);
    if (!(__builtin_fabs(l) <= 1.7976931348623157e308)) {
        l = __builtin_nan("");
        atomicOr(status, SX_STATUS_NAN);
    }
    loss[p] = l;
}

}  // namespace sx
