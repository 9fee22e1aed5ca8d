// The large-N path: the kernels of sx_big.hpp and the two predict helpers, launch_predict_big and launch_rollout_big
// (sx_big_launch.hpp) for every shift-0 shape of SX_ROLLOUT_SHAPES, and sx_gp_big_tiling, which reports the tiling they launch.
#include <cstdlib>

#include "sx_big.hpp"
#include "sx_big_launch.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES

namespace sx {

// trmm_reduce_kernel variants, selectable for A/B measurements (tools/cfg4_probe.py), read once per process:
//   SX_TRMM_ORDER   = tile order bits: 16 paired tiles (default for small grids), 8 longest-first (default otherwise),
//                     1 XCD-contiguous with the row tile fastest, 0 plain;
//                     + 2 / + 4: timing-only diagnostics (every workgroup reads the same Kstar / W tile: no fabric traffic)
//   SX_TRMM_VARIANT = <pairs per chunk><LDS buffers>: 13 (default), 12, 22, 23
//   SX_TRMM_PT      = particle tiles per workgroup: 8 | 4 (default: 4 where 8 would leave a compute unit with at most two
//                     workgroups, see plan_big_tiling in sx_big_launch.hpp)
// Measured at config 4 (N = 2000, 16 384 particles), per launch: plain order 7.2 ms, XCD-contiguous 4.73 ms, longest-first
// 3.92 ms -- whatever the variant, and the same with the fabric traffic removed (order + 6): the kernel was never
// memory-bound, its tiles differ 16-fold in work and the tail of the launch was what it lost.
static const TrmmOverride& trmm_override() {
    static const TrmmOverride o = [] {
        const char *order = std::getenv("SX_TRMM_ORDER"), *variant = std::getenv("SX_TRMM_VARIANT"), *pt = std::getenv("SX_TRMM_PT");
        return TrmmOverride{order ? std::atoi(order) : -1, variant ? std::atoi(variant) : 13, pt ? std::atoi(pt) : 0};
    }();
    return o;
}

template <int NS, int D, int PPC, int NBUF, int PT>
static void launch_trmm_v(int kind, const GpConst<NS, D>& gc, const BigWs& ws, int64_t p128, const BigTiling& t, hipStream_t stream) {
    constexpr int lds = big_lds_bytes<PPC, NBUF, PT>();
    (void)allow_lds(trmm_reduce_kernel<NS, D, PPC, NBUF, PT>, lds);
    const dim3 grid((unsigned)t.grid);
    if (kind >= 0)
        launch(kind, trmm_reduce_kernel<NS, D, PPC, NBUF, PT>, grid, dim3(kBigThreads), lds, stream, gc, ws, p128, t.row_tiles, t.order);
    else
        hipLaunchKernelGGL((trmm_reduce_kernel<NS, D, PPC, NBUF, PT>), grid, dim3(kBigThreads), lds, stream, gc, ws, p128, t.row_tiles,
                           t.order);
}

// trmm_reduce_kernel in the tiling plan_big_tiling (sx_big_launch.hpp) picks for the shape and the process's SX_TRMM_* settings
template <int NS, int D>
static void launch_trmm(int kind, const GpConst<NS, D>& gc, const BigWs& ws, int64_t p128, hipStream_t stream) {
    const BigTiling t = plan_big_tiling(NS, gc.n_pad, p128, trmm_override());
    if (t.pt == 4) return launch_trmm_v<NS, D, 1, 3, 4>(kind, gc, ws, p128, t, stream);
    switch (t.variant()) {
        case 12: return launch_trmm_v<NS, D, 1, 2, 8>(kind, gc, ws, p128, t, stream);
        case 22: return launch_trmm_v<NS, D, 2, 2, 8>(kind, gc, ws, p128, t, stream);
        case 23: return launch_trmm_v<NS, D, 2, 3, 8>(kind, gc, ws, p128, t, stream);
        default: return launch_trmm_v<NS, D, 1, 3, 8>(kind, gc, ws, p128, t, stream);
    }
}

// ---- sx_gp_predict for training sets beyond the LDS budget: the same Kstar / triangular-product kernels, then collect ----
template <int NS, int D>
__global__ void predict_init_big_kernel(const double* __restrict__ z, int64_t P, int64_t p128, BigWs ws) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= p128 * D) return;
    ws.zs[i] = (i < P * D) ? z[i] : 0.0;
}

template <int NS, int D>
__global__ void predict_collect_big_kernel(GpConst<NS, D> gc, BigWs ws, int64_t P, int64_t p128, int row_parts,
                                           double* __restrict__ mean, double* __restrict__ var, double* __restrict__ jac) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (g >= P) return;
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        double q = 0.0;
        for (int r = 0; r < row_parts; ++r) q += ws.part[((int64_t)d * row_parts + r) * p128 + g];
        var[g * NS + d] = (gc.outputscale[d] - q) + gc.noise[d];
        const double m = ws.mj[((int64_t)d * (D + 1)) * p128 + g];
        mean[g * NS + d] = m;
        if (jac) {
#pragma unroll
            for (int j = 0; j < D; ++j)
                jac[(g * NS + d) * D + j] =
                    ws.mj[((int64_t)d * (D + 1) + 1 + j) * p128 + g] - ws.zs[g * D + j] * gc.inv_ls2[d * D + j] * m;
        }
    }
}

template <int NS, int NU>
int launch_predict_big(const sx_gp_model* m, const double* z, int P, double* mean, double* var, double* jac,
                       double* workspace, int64_t workspace_bytes, hipStream_t stream) {
    constexpr int D = NS + NU;
    auto gc = make_gp_const<NS, NU>(m, kPredictThreads / 64);
    const int64_t p128 = ((int64_t)P + kBigTile - 1) / kBigTile * kBigTile;
    BigWs ws = big_ws_layout(workspace, NS, D, m->n_pad, P);
    if (!workspace || workspace_bytes < ws.total * (int64_t)sizeof(double)) return SX_ERR_ARG;
    const int row_tiles = (m->n_pad + kBigTile - 1) / kBigTile;
    hipLaunchKernelGGL((predict_init_big_kernel<NS, D>), dim3((unsigned)((p128 * D + 255) / 256)), dim3(256), 0, stream, z,
                       (int64_t)P, p128, ws);
    hipLaunchKernelGGL((kstar_big_kernel<NS, D>), dim3((unsigned)(p128 / 16), (unsigned)((m->n_pad + 255) / 256)), dim3(256),
                       0, stream, gc, ws);
    launch_trmm<NS, D>(-1, gc, ws, p128, stream);
    hipLaunchKernelGGL((predict_collect_big_kernel<NS, D>), dim3((unsigned)((P + 63) / 64)), dim3(64), 0, stream, gc, ws,
                       (int64_t)P, p128, row_tiles * 2, mean, var, jac);
    return check_launch();
}

template <int NS, int NU>
int launch_rollout_big(const sx_gp_model* m, const sx_env* env, const RolloutPtrs& rp, double* workspace,
                       int64_t workspace_bytes, hipStream_t stream) {
    constexpr int D = NS + NU;
    auto gc = make_gp_const<NS, NU>(m, kRolloutThreads / 64);
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if (int r = env_consts<NS, NU>(env, rc, cc)) return r;
    const int64_t total = (int64_t)rp.E * rp.P;
    const int64_t p128 = (total + kBigTile - 1) / kBigTile * kBigTile;
    BigWs ws = big_ws_layout(workspace, NS, D, m->n_pad, total);
    if (!workspace || workspace_bytes < ws.total * (int64_t)sizeof(double)) return SX_ERR_ARG;
    const int row_tiles = (m->n_pad + kBigTile - 1) / kBigTile;
    BigInit bi{rp.x0, rp.q0, rp.mean, rp.std, rp.noise, rp.actions, rp.obj_cost, rp.con_cost, rp.P, rp.H};
    hipLaunchKernelGGL((init_big_kernel<NS, NU>), dim3((unsigned)((p128 + 255) / 256)), dim3(256), 0, stream, bi, ws, total,
                       p128);
    for (int t = 0; t < rp.H; ++t) {
        launch(SX_PROF_KSTAR_BIG, kstar_big_kernel<NS, D>, dim3((unsigned)(p128 / 16), (unsigned)((m->n_pad + 255) / 256)),
               dim3(256), 0, stream, gc, ws);
        launch_trmm<NS, D>(SX_PROF_TRMM_BIG, gc, ws, p128, stream);
        BigStep bs{rp.actions, rp.traj, rp.sigma, rp.obj_cost, rp.con_cost, rp.status, rp.H, t, row_tiles * 2,
                   (t > 0 || rp.q0 != nullptr) ? 1 : 0};
        launch(SX_PROF_STEP_BIG, step_big_kernel<NS, NU>, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, stream, gc, rc, cc,
               bs, ws, total, p128);
    }
    return check_launch();
}

}  // namespace sx

#define SX_BIG_INSTANTIATE(NS, NU)                                                                                      \
    template int sx::launch_predict_big<NS, NU>(const sx_gp_model*, const double*, int, double*, double*, double*,     \
                                                double*, int64_t, hipStream_t);                                        \
    template int sx::launch_rollout_big<NS, NU>(const sx_gp_model*, const sx_env*, const sx::RolloutPtrs&, double*,    \
                                                int64_t, hipStream_t);
#define SX_BIG_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_BIG_INSTANTIATE(NS, NU))
SX_ROLLOUT_SHAPES(SX_BIG_ONE, 0)

extern "C" int sx_gp_big_tiling(const sx_gp_model* model, int64_t particles, int* pt, int* order, int* variant, int64_t* grid) {
    if (!model || !pt || !order || !variant || !grid || particles < 0 || model->n_s <= 0 || model->n_pad <= 0) return SX_ERR_ARG;
    const int64_t p128 = (particles + sx::kBigTile - 1) / sx::kBigTile * sx::kBigTile;
    const sx::BigTiling t = sx::plan_big_tiling(model->n_s, model->n_pad, p128, sx::trmm_override());
    *pt = t.pt;
    *order = t.order;
    *variant = t.variant();
    *grid = t.grid;
    return SX_OK;
}
