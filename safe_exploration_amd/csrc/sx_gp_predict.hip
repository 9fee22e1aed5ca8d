// The exact-GP posterior and the one-step reachability outside a rollout: gp_predict_kernel, the reach and polytope
// kernels, and the entries sx_gp_predict[_workspace_bytes], sx_onestep_reach and sx_polytope_distance.  Training sets beyond
// the LDS budget take the large-N path (sx_big_launch.hpp).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/sx_amd.h"
#include "sx_big.hpp"   // big_ws_layout
#include "sx_big_launch.hpp"
#include "sx_gp.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_reach.hpp"
#include "sx_stream_launch.hpp"   // SX_DISPATCH

namespace sx {

// ---------------------------------------------------------------------------------------------------------------
// sx_gp_predict: one 16-point tile per workgroup
// ---------------------------------------------------------------------------------------------------------------
// (BYOUT: one output's Kstar in LDS at a time, as in the rollout kernel)
template <int NS, int NU, bool BYOUT = false>
__global__ __launch_bounds__(kPredictThreads) void gp_predict_kernel(GpConst<NS, NS + NU> gc,
                                                                     const int4* __restrict__ stage_tab,
                                                                     const double* __restrict__ z, int P,
                                                                     double* __restrict__ mean, double* __restrict__ var,
                                                                     double* __restrict__ jac) {
    constexpr int D = NS + NU;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    GpTileLds<NS, D> lds;
    const int nw = blockDim.x >> 6;
    lds.carve(smem, gc.n_train, gc.n_pad, nw, BYOUT ? 1 : NS);
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    gp_load_xs(gc, lds);
    const MfmaHead head = gp_mfma_head(gc, stage_tab, wave, nw, lane, gc.stage_cap);
    const int4* __restrict__ const tab_one = stage_tab + (size_t)nw * (1 + gc.stage_cap);
    for (int tile = blockIdx.x; tile * SX_TILE < P; tile += gridDim.x) {
        const int g0 = tile * SX_TILE;
        if (tid < SX_TILE * D) {
            const int c = tid / D, j = tid - c * D;
            lds.zs[tid] = (g0 + c < P) ? z[(int64_t)(g0 + c) * D + j] : 0.0;
        }
        __syncthreads();
        int qb, qe;
        kstar_pair_range(gc.n_pad >> 3, wave, 1, nw, qb, qe);
        double zq[D];
#pragma unroll
        for (int j = 0; j < D; ++j) zq[j] = lds.zs[(lane & 15) * D + j];
        if constexpr (BYOUT) {
            auto one_output = [&](auto dtag) {
                constexpr int DD = decltype(dtag)::value;
                if constexpr (DD < NS) {
                    const int4* __restrict__ tab_d = tab_one + (size_t)DD * nw * (1 + gc.stage_cap_one);
                    const MfmaHead head_d = gp_mfma_head(gc, tab_d, wave, nw, lane, gc.stage_cap_one);
                    gp_kstar_phase_one<NS, D, DD>(gc, lds, qb, qe, zq);
                    __syncthreads();
                    gp_mfma_phase<NS, D, 1>(gc, tab_d, lds, wave, nw, lane, head_d, gc.stage_cap_one, DD);
                    __syncthreads();
                }
            };
            one_output(std::integral_constant<int, 0>{});
            one_output(std::integral_constant<int, 1>{});
            one_output(std::integral_constant<int, 2>{});
            one_output(std::integral_constant<int, 3>{});
        } else {
            gp_kstar_phase(gc, lds, qb, qe, zq);
            __syncthreads();
            gp_mfma_phase(gc, stage_tab, lds, wave, nw, lane, head, gc.stage_cap);
            __syncthreads();
        }
        if (tid < SX_TILE && g0 + tid < P) {
            double zz[D], m[NS], v[NS], jc[NS][D];
#pragma unroll
            for (int j = 0; j < D; ++j) zz[j] = lds.zs[tid * D + j];
            if (jac) {
                gp_collect<NS, D, true>(gc, lds, nw, tid, zz, m, v, jc);
            } else {
                gp_collect<NS, D, false>(gc, lds, nw, tid, zz, m, v, jc);
            }
            const int64_t g = g0 + tid;
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
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// sx_onestep_reach / sx_polytope_distance: one particle per lane
// ---------------------------------------------------------------------------------------------------------------
// Pre-pass of sx_onestep_reach: does the variance batch hold an exact zero (gp_reachability_pytorch.py:238)?  ONE
// workgroup, so it is the only writer of the scratch bit: it clears the bit a previous call may have left and sets it
// again if this batch has a zero.  The main kernel reads the bit; both run on the caller's stream, in order.
constexpr int kStatusScratchBatchZero = 0x10000;
__global__ __launch_bounds__(1024) void batch_zero_flag_kernel(const double* __restrict__ var, int64_t n, int* __restrict__ status) {
    int any = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) any |= (var[i] == 0.0) ? 1 : 0;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        atomicAnd(status, ~kStatusScratchBatchZero);
        if (any) atomicOr(status, kStatusScratchBatchZero);
    }
}

template <int NS, int NU>
__global__ void onestep_reach_kernel(ReachConst<NS, NU> rc, int P, const double* __restrict__ p_in,
                                     const double* __restrict__ q_in, const double* __restrict__ u_in,
                                     const double* __restrict__ mean_in, const double* __restrict__ var_in,
                                     const double* __restrict__ jac_in, double* __restrict__ p_out,
                                     double* __restrict__ q_out, double* __restrict__ sig_out, int* __restrict__ status) {
    constexpr int D = NS + NU;
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (g >= P) return;
    double p[NS], u[NU], mean[NS], var[NS], p1[NS], Q1[NS][NS];
    int st = 0;
    // the whole-batch rule of _fix_zeros_nans: with an exact zero anywhere in the batch, every var <= 0 is lifted
    const bool batch_zero = (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kStatusScratchBatchZero) != 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        p[i] = p_in[g * NS + i];
        mean[i] = mean_in[g * NS + i];
        var[i] = var_in[g * NS + i];
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) u[c] = u_in[g * NU + c];
    if (q_in == nullptr) {
        reach_point<NS, NU>(rc, p, u, mean, var, p1, Q1, st, batch_zero);
    } else {
        double Q[NS][NS], jac[NS][D];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
#pragma unroll
            for (int j = 0; j < NS; ++j) Q[i][j] = q_in[(g * NS + i) * NS + j];
#pragma unroll
            for (int j = 0; j < D; ++j) jac[i][j] = jac_in[(g * NS + i) * D + j];
        }
        reach_ellipsoid<NS, NU>(rc, p, Q, u, mean, var, jac, p1, Q1, st, batch_zero);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        p_out[g * NS + i] = p1[i];
        sig_out[g * NS + i] = var[i];
#pragma unroll
        for (int j = 0; j < NS; ++j) q_out[(g * NS + i) * NS + j] = Q1[i][j];
    }
    if (st) atomicOr(status, st);
}

template <int NS>
struct PolyArgs {
    double h_mat[SX_MAX_M * NS];
    double h_vec[SX_MAX_M];
    int m;
};

template <int NS>
__global__ void polytope_kernel(PolyArgs<NS> pa, int P, double c_safety, const double* __restrict__ p_in,
                                const double* __restrict__ q_in, double* __restrict__ d_out,
                                uint8_t* __restrict__ inside) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (g >= P) return;
    double p[NS], Q[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        p[i] = p_in[g * NS + i];
#pragma unroll
        for (int j = 0; j < NS; ++j) Q[i][j] = q_in[(g * NS + i) * NS + j];
    }
    double d[SX_MAX_M];
    const bool viol = polytope_violated<SX_MAX_M, NS>(pa.h_mat, pa.h_vec, pa.m, c_safety, p, Q, d);
    for (int r = 0; r < pa.m; ++r) d_out[g * pa.m + r] = d[r];
    if (inside) inside[g] = viol ? 0 : 1;
}

static bool predict_fits(int ns, int nu, int n_train, int n_pad, int ns_lds = -1) {
    const int nw = kPredictThreads / 64;
    return gp_tile_lds_doubles(ns, ns + nu, n_train, n_pad, nw, ns_lds) * sizeof(double) <= kMaxLdsBytes && n_pad <= 1024;
}

template <int NS, int NU>
static int launch_predict(const sx_gp_model* m, const double* z, int P, double* mean, double* var, double* jac,
                          double* workspace, int64_t workspace_bytes, hipStream_t stream) {
    const bool all_at_once = predict_fits(NS, NU, m->n_train, m->n_pad);
    if (!all_at_once && !(NS > 1 && predict_fits(NS, NU, m->n_train, m->n_pad, 1)))
        return launch_predict_big<NS, NU>(m, z, P, mean, var, jac, workspace, workspace_bytes, stream);
    const int nw = kPredictThreads / 64;
    auto gc = make_gp_const<NS, NU>(m, nw);
    const size_t lds = gp_tile_lds_doubles(NS, NS + NU, m->n_train, m->n_pad, nw, all_at_once ? NS : 1) * sizeof(double);
    const int tiles = (P + SX_TILE - 1) / SX_TILE;
    const int grid = tiles < 4096 ? tiles : 4096;
    if (all_at_once) {
        if (int rc = allow_lds(gp_predict_kernel<NS, NU, false>, lds)) return rc;
        hipLaunchKernelGGL((gp_predict_kernel<NS, NU, false>), dim3(grid), dim3(kPredictThreads), lds, stream, gc,
                           gc.stage_tab, z, P, mean, var, jac);
    } else {
        if (int rc = allow_lds(gp_predict_kernel<NS, NU, true>, lds)) return rc;
        hipLaunchKernelGGL((gp_predict_kernel<NS, NU, true>), dim3(grid), dim3(kPredictThreads), lds, stream, gc,
                           gc.stage_tab, z, P, mean, var, jac);
    }
    return check_launch();
}

template <int NS, int NU>
static int launch_reach(const sx_env* env, int P, const double* p, const double* Q, const double* u, const double* mean,
                        const double* var, const double* jac, double* p1, double* Q1, double* sigma, int* status,
                        hipStream_t stream) {
    ReachConst<NS, NU> rc;
    if (!make_reach_const<NS, NU>(env, rc)) return SX_ERR_ARG;
    const int threads = 64;
    hipLaunchKernelGGL(batch_zero_flag_kernel, dim3(1), dim3(1024), 0, stream, var, (int64_t)P * NS, status);
    hipLaunchKernelGGL((onestep_reach_kernel<NS, NU>), dim3((P + threads - 1) / threads), dim3(threads), 0, stream, rc,
                       P, p, Q, u, mean, var, jac, p1, Q1, sigma, status);
    hipLaunchKernelGGL(batch_zero_flag_kernel, dim3(1), dim3(64), 0, stream, var, (int64_t)0, status);  // clears the scratch bit
    return check_launch();
}

template <int NS>
static int launch_polytope(const sx_env* env, int P, const double* p, const double* Q, double c_safety, double* d,
                           uint8_t* inside, hipStream_t stream) {
    PolyArgs<NS> pa;
    std::memset(&pa, 0, sizeof(pa));
    for (int r = 0; r < env->m; ++r) {
        for (int i = 0; i < NS; ++i) pa.h_mat[r * NS + i] = env->h_mat[r * NS + i];
        pa.h_vec[r] = env->h_vec[r];
    }
    pa.m = env->m;
    const int threads = 64;
    hipLaunchKernelGGL((polytope_kernel<NS>), dim3((P + threads - 1) / threads), dim3(threads), 0, stream, pa, P,
                       c_safety, p, Q, d, inside);
    return check_launch();
}

}  // namespace sx

extern "C" {

int64_t sx_gp_predict_workspace_bytes(const sx_gp_model* model, int P) {
    if (!model || P < 0) return -1;
    if (sx::predict_fits(model->n_s, model->n_u, model->n_train, model->n_pad)) return 0;
    if (model->n_s > 1 && sx::predict_fits(model->n_s, model->n_u, model->n_train, model->n_pad, 1)) return 0;
    return sx::big_ws_layout(nullptr, model->n_s, model->n_s + model->n_u, model->n_pad, P).total * (int64_t)sizeof(double);
}

int sx_gp_predict(const sx_gp_model* model, const double* z, int P, double* mean, double* var, double* jac,
                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (!model || P < 0) return SX_ERR_ARG;
    if (P == 0) return SX_OK;   // an empty batch is not an error (its pointers may be NULL)
    if (!z || !mean || !var) return SX_ERR_ARG;
#define CALL(NS, NU) \
    sx::launch_predict<NS, NU>(model, z, P, mean, var, jac, (double*)workspace, workspace_bytes, (hipStream_t)stream)
    SX_DISPATCH(model->n_s, model->n_u, CALL);
#undef CALL
}

int sx_onestep_reach(const sx_env* env, int P, const double* p, const double* Q, const double* u, const double* mean,
                     const double* var, const double* jac, double* p1, double* Q1, double* sigma, int32_t* status,
                     void* stream) {
    if (!env || !p || !u || !mean || !var || !p1 || !Q1 || !sigma || !status || P < 0) return SX_ERR_ARG;
    if (Q && !jac) return SX_ERR_ARG;
    if (P == 0) return SX_OK;
#define CALL(NS, NU) \
    sx::launch_reach<NS, NU>(env, P, p, Q, u, mean, var, jac, p1, Q1, sigma, status, (hipStream_t)stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

int sx_polytope_distance(const sx_env* env, int P, const double* p, const double* Q, double c_safety, double* d,
                         uint8_t* inside, void* stream) {
    if (!env || !p || !Q || !d || P < 0) return SX_ERR_ARG;
    if (env->m <= 0 || env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    if (P == 0) return SX_OK;
    switch (env->n_s) {
        case 1: return sx::launch_polytope<1>(env, P, p, Q, c_safety, d, inside, (hipStream_t)stream);
        case 2: return sx::launch_polytope<2>(env, P, p, Q, c_safety, d, inside, (hipStream_t)stream);
        case 3: return sx::launch_polytope<3>(env, P, p, Q, c_safety, d, inside, (hipStream_t)stream);
        case 4: return sx::launch_polytope<4>(env, P, p, Q, c_safety, d, inside, (hipStream_t)stream);
        default: return SX_ERR_UNSUPPORTED;
    }
}

}  // extern "C"
