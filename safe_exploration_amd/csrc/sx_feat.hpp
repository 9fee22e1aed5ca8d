// Exact GPs with a DEGENERATE kernel  k_d(x, x') = c_d phi(x) . phi(x')  -- the reference's 'linear' kernel (phi = identity)
// and 'nn' kernel (phi = a small fully connected network, min/max-normalised per point), ssm_cem/gp_ssm_cem.py:45-57,140-185.
//
// MI355X-first form: such a GP is Bayesian linear regression on F features, so nothing about it scales with N_train at
// prediction time.  With  A_d = Phi^T Phi + (noise_d / c_d) I  (F x F),  M_d = chol(A_d)^-1,  wbar_d = A_d^-1 Phi^T y_d:
//     mean_d(z) = wbar_d . phi(z)          var_d(z) = noise_d (|M_d phi(z)|^2 + 1)      (likelihood noise included)
//     d mean_d / dz = (d phi / dz)^T wbar_d                                          (reverse sweep through the network)
// -- identical to the kernel-space posterior (Woodbury), which is how the oracle computes it.  A particle-step is a few
// thousand flops on F <= 32 features: one particle per LANE for the whole rollout, weights and M_d read through the scalar
// cache (their indices are wave-uniform), per-lane activations in LDS ([unit][lane]: conflict-free).  No matrix cores: there
// is no N x N operand to contract.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_reach.hpp"
#include "sx_step.hpp"

namespace sx {

constexpr int kFeatWave = 64;                            // one wave per workgroup, one particle per lane
// LDS doubles per workgroup: pre-activations of every layer + features + two scratch vectors of the reverse sweep, [unit][lane]
constexpr int kFeatLdsDoubles = (SX_FEAT_MAX_LAYERS + 3) * SX_FEAT_MAX_WIDTH * kFeatWave;

struct FeatConst {
    int n_layers, n_feat, normalise, d_in;
    int width[SX_FEAT_MAX_LAYERS + 1];
    double prelu;
    double noise[SX_MAX_NS];
    const double* net;
    const double* wbar;
    const double* minv;
};

// phi(z) for this lane's point.  pre[l] (LDS, [unit][lane]) keeps layer l's pre-activations for the reverse sweep;
// `feat` receives phi.  Returns argmin / argmax / min / max of the un-normalised features through the references.
template <int D>
__device__ __forceinline__ void feat_forward(const FeatConst& fc, const double (&z)[D], double* lds, int lane, int& amin,
                                             int& amax, double& fmin, double& fmax) {
    double* feat = lds + (SX_FEAT_MAX_LAYERS) * SX_FEAT_MAX_WIDTH * kFeatWave;
    const int F = fc.n_feat;
    if (fc.n_layers == 0) {   // linear kernel: phi = z
#pragma unroll
        for (int j = 0; j < D; ++j) feat[j * kFeatWave + lane] = z[j];
        amin = amax = 0;
        fmin = fmax = 0.0;
        return;
    }
    const double* w = fc.net;
    for (int l = 1; l <= fc.n_layers; ++l) {
        const int win = fc.width[l - 1], wout = fc.width[l];
        double* out = lds + (l - 1) * SX_FEAT_MAX_WIDTH * kFeatWave;
        const double* in = lds + (l - 2) * SX_FEAT_MAX_WIDTH * kFeatWave;   // (l == 1 reads z instead)
        const double* bias = w + (size_t)wout * win;
        for (int k = 0; k < wout; ++k) {
            double s = bias[k];
            if (l == 1) {
#pragma unroll
                for (int i = 0; i < D; ++i) s = fma(w[k * D + i], z[i], s);
            } else {
                for (int i = 0; i < win; ++i) {
                    const double a = in[i * kFeatWave + lane];
                    s = fma(w[k * win + i], a > 0.0 ? a : 0.0, s);           // ReLU between the layers
                }
            }
            out[k * kFeatWave + lane] = s;
        }
        w = bias + wout;
    }
    // PReLU after the last layer, then the reference's per-point normalisation (gp_ssm_cem.py:176-181):
    //   phi = 2 (f - min f) / max f - 1        (max of the UN-shifted features, as the reference writes it)
    const double* last = lds + (fc.n_layers - 1) * SX_FEAT_MAX_WIDTH * kFeatWave;
    fmin = 0.0;
    fmax = 0.0;
    amin = amax = 0;
    for (int k = 0; k < F; ++k) {
        const double p = last[k * kFeatWave + lane];
        const double f = p > 0.0 ? p : fc.prelu * p;
        feat[k * kFeatWave + lane] = f;
        if (k == 0 || f < fmin) { fmin = f; amin = k; }
        if (k == 0 || f > fmax) { fmax = f; amax = k; }
    }
    if (fc.normalise) {
        for (int k = 0; k < F; ++k) feat[k * kFeatWave + lane] = 2.0 * ((feat[k * kFeatWave + lane] - fmin) / fmax) - 1.0;
    }
}

// mean, variance (noise included) and, with WITH_JAC, the mean Jacobian [NS][D] of this lane's point.
template <int NS, int D, bool WITH_JAC>
__device__ __forceinline__ void feat_gp_predict(const FeatConst& fc, const double (&z)[D], double* lds, int lane,
                                                double (&mean)[NS], double (&var)[NS], double (&jac)[NS][D]) {
    int amin, amax;
    double fmin, fmax;
    feat_forward<D>(fc, z, lds, lane, amin, amax, fmin, fmax);
    const int F = fc.n_feat;
    const double* feat = lds + (SX_FEAT_MAX_LAYERS) * SX_FEAT_MAX_WIDTH * kFeatWave;
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        double* grad = lds + (SX_FEAT_MAX_LAYERS + 1) * SX_FEAT_MAX_WIDTH * kFeatWave;   // scratch of the reverse sweep
        const double* wb = fc.wbar + (size_t)d * F;
        const double* M = fc.minv + (size_t)d * F * F;
        double m = 0.0, q = 0.0;
        for (int r = 0; r < F; ++r) {
            const double ph = feat[r * kFeatWave + lane];
            m = fma(wb[r], ph, m);
            double t = 0.0;
            for (int k = 0; k <= r; ++k) t = fma(M[r * F + k], feat[k * kFeatWave + lane], t);
            q = fma(t, t, q);
        }
        mean[d] = m;
        var[d] = fc.noise[d] * q + fc.noise[d];
        if constexpr (WITH_JAC) {
            if (fc.n_layers == 0) {
#pragma unroll
                for (int j = 0; j < D; ++j) jac[d][j] = wb[j];
                continue;
            }
            // reverse sweep: g_phi = wbar_d -> normalisation -> PReLU -> layers
            double gsum = 0.0, gdot = 0.0;
            const double* last = lds + (fc.n_layers - 1) * SX_FEAT_MAX_WIDTH * kFeatWave;
            if (fc.normalise) {
                for (int k = 0; k < F; ++k) {
                    gsum += wb[k];
                    // f_k - min f recovered from phi: (phi + 1) max f / 2
                    gdot = fma(wb[k], (feat[k * kFeatWave + lane] + 1.0) * 0.5 * fmax, gdot);
                }
            }
            for (int k = 0; k < F; ++k) {
                double g = wb[k];
                if (fc.normalise) {
                    g = 2.0 / fmax * g;
                    if (k == amin) g -= 2.0 / fmax * gsum;
                    if (k == amax) g -= 2.0 / (fmax * fmax) * gdot;
                }
                const double p = last[k * kFeatWave + lane];
                grad[k * kFeatWave + lane] = g * (p > 0.0 ? 1.0 : fc.prelu);
            }
            // layers L .. 1; the weights of layer l start at offset off[l]
            int off[SX_FEAT_MAX_LAYERS + 1];
            off[1] = 0;
            for (int l = 1; l < fc.n_layers; ++l) off[l + 1] = off[l] + fc.width[l] * fc.width[l - 1] + fc.width[l];
            for (int l = fc.n_layers; l >= 1; --l) {
                const int win = fc.width[l - 1], wout = fc.width[l];
                const double* w = fc.net + off[l];
                if (l == 1) {
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        double s = 0.0;
                        for (int k = 0; k < wout; ++k) s = fma(w[k * D + i], grad[k * kFeatWave + lane], s);
                        jac[d][i] = s;
                    }
                } else {
                    const double* pre = lds + (l - 2) * SX_FEAT_MAX_WIDTH * kFeatWave;
                    // (every input unit reads ALL of the layer's output gradients: the new gradient goes to a second
                    // scratch vector and the two swap roles)
                    double* next = lds + (SX_FEAT_MAX_LAYERS + 1 + ((fc.n_layers - l) & 1 ? 0 : 1)) * SX_FEAT_MAX_WIDTH * kFeatWave;
                    for (int i = 0; i < win; ++i) {
                        double s = 0.0;
                        for (int k = 0; k < wout; ++k) s = fma(w[k * win + i], grad[k * kFeatWave + lane], s);
                        next[i * kFeatWave + lane] = (pre[i * kFeatWave + lane] > 0.0) ? s : 0.0;
                    }
                    grad = next;
                }
            }
        }
    }
}

inline FeatConst make_feat_const(const sx_feat_model* m) {
    FeatConst fc;
    fc.n_layers = m->n_layers;
    fc.n_feat = m->n_feat;
    fc.normalise = m->normalise;
    fc.d_in = m->n_s + m->n_u;
    for (int l = 0; l <= SX_FEAT_MAX_LAYERS; ++l) fc.width[l] = m->width[l];
    fc.prelu = m->prelu;
    for (int d = 0; d < SX_MAX_NS; ++d) fc.noise[d] = m->noise[d];
    fc.net = m->net;
    fc.wbar = m->wbar;
    fc.minv = m->minv;
    return fc;
}

// ---- sx_feat_features: Phi = phi(X) for N points ---------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kFeatWave) void feat_features_kernel(FeatConst fc, const double* __restrict__ x, int n,
                                                                  double* __restrict__ phi) {
    extern __shared__ __attribute__((aligned(16))) double feat_smem[];
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x * (int64_t)kFeatWave + lane;
    double z[D];
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = (g < n) ? x[g * D + j] : 0.0;
    int amin, amax;
    double fmin, fmax;
    feat_forward<D>(fc, z, feat_smem, lane, amin, amax, fmin, fmax);
    const double* feat = feat_smem + (SX_FEAT_MAX_LAYERS) * SX_FEAT_MAX_WIDTH * kFeatWave;
    if (g < n)
        for (int k = 0; k < fc.n_feat; ++k) phi[g * fc.n_feat + k] = feat[k * kFeatWave + lane];
}

// ---- sx_feat_predict ---------------------------------------------------------------------------------------------------
template <int NS, int NU>
__global__ __launch_bounds__(kFeatWave) void feat_predict_kernel(FeatConst fc, const double* __restrict__ zin, int P,
                                                                 double* __restrict__ mean, double* __restrict__ var,
                                                                 double* __restrict__ jac) {
    constexpr int D = NS + NU;
    extern __shared__ __attribute__((aligned(16))) double feat_smem[];
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x * (int64_t)kFeatWave + lane;
    double z[D], m[NS], v[NS], jc[NS][D];
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = (g < P) ? zin[g * D + j] : 0.0;
    if (jac)
        feat_gp_predict<NS, D, true>(fc, z, feat_smem, lane, m, v, jc);
    else
        feat_gp_predict<NS, D, false>(fc, z, feat_smem, lane, m, v, jc);
    if (g >= P) return;
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        mean[g * NS + d] = m[d];
        var[g * NS + d] = v[d];
        if (jac) {
#pragma unroll
            for (int j = 0; j < D; ++j) jac[(g * NS + d) * D + j] = jc[d][j];
        }
    }
}

// ---- sx_cem_rollout_feat: the CEM particle rollout over a feature-space GP, one particle per lane for all H steps ----------
// (cem_rollout_lanes, sx_step.hpp, with the GP's prediction; the modes SH and MM are described there)
template <int NS, int NU, int SH = 0, bool MM = false>
__global__ __launch_bounds__(kFeatWave) void cem_rollout_feat_kernel(typename ModelArg<FeatConst, MM>::type fc_arg,
                                                                     ReachConst<NS, NU> rc, CostConst<SX_MAX_M, NS, NU> cc,
                                                                     FeatRolloutPtrs rp) {
    constexpr int D = NS + NU + SH;
    extern __shared__ __attribute__((aligned(16))) double feat_smem[];
    cem_rollout_lanes<NS, NU, SH, MM, kFeatWave, FeatConst>(
        fc_arg, rc, cc, rp,
        [&](auto with_jac, const FeatConst& fc, const double (&z)[D], int lane, double (&mean)[NS], double (&var)[NS],
            double (&jac)[NS][D]) { feat_gp_predict<NS, D, decltype(with_jac)::value>(fc, z, feat_smem, lane, mean, var, jac); });
}

}  // namespace sx
