// The feature-GP and MC-dropout rollout kernels in the multi-model mode (sx_cem_rollout_feat_multi /
// sx_cem_rollout_mlp_multi): every shift-0 shape of SX_ROLLOUT_SHAPES.
#include <climits>

#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES
#include "sx_feat.hpp"
#include "sx_mlp.hpp"
#include "sx_mlp_mfma.hpp"
#include "sx_model_multi.hpp"

namespace sx {

// E problems x ceil(P / tile) workgroups (0: more than a grid holds)
static unsigned multi_grid(const FeatRolloutPtrs& rp, int tile) {
    const int64_t n = (int64_t)rp.E * ((rp.P + tile - 1) / tile);
    return n > INT_MAX ? 0u : (unsigned)n;
}

template <int NS, int NU>
int launch_rollout_feat_multi(const FeatConst* table, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                              const FeatRolloutPtrs& rp, hipStream_t stream) {
    const unsigned grid = multi_grid(rp, kFeatWave);
    if (grid == 0) return SX_ERR_UNSUPPORTED;
    const size_t lds = kFeatLdsDoubles * sizeof(double);
    if (int r = allow_lds(cem_rollout_feat_kernel<NS, NU, 0, true>, lds)) return r;
    launch(SX_PROF_ROLLOUT_FEAT, cem_rollout_feat_kernel<NS, NU, 0, true>, dim3(grid), dim3(kFeatWave), lds, stream, table,
           rc, cc, rp);
    return check_launch();
}

template <int NS, int NU, int L, bool FULL>
static int launch_rollout_mlp_mfma_multi(const MlpConst* table, const ReachConst<NS, NU>& rc,
                                         const CostConst<SX_MAX_M, NS, NU>& cc, const FeatRolloutPtrs& rp,
                                         hipStream_t stream) {
    const unsigned grid = multi_grid(rp, kMmTile);
    if (grid == 0) return SX_ERR_UNSUPPORTED;
    const size_t lds = (size_t)MmLds<NS, NS + NU>::total * sizeof(double);
    if (int r = allow_lds(cem_rollout_mlp_mfma_kernel<NS, NU, L, FULL, 0, true>, lds)) return r;
    launch(SX_PROF_ROLLOUT_MLP, cem_rollout_mlp_mfma_kernel<NS, NU, L, FULL, 0, true>, dim3(grid), dim3(kMmThreads), lds,
           stream, table, rc, cc, rp);
    return check_launch();
}

template <int NS, int NU>
int launch_rollout_mlp_multi(const MlpConst* table, const MlpConst& arch, bool mfma, const ReachConst<NS, NU>& rc,
                             const CostConst<SX_MAX_M, NS, NU>& cc, const FeatRolloutPtrs& rp, hipStream_t stream) {
    if (mfma) {
        return mlp_mfma_form(arch, [&](auto l, auto full) {
            return launch_rollout_mlp_mfma_multi<NS, NU, decltype(l)::value, decltype(full)::value>(table, rc, cc, rp, stream);
        });
    }
    const unsigned grid = multi_grid(rp, kMlpLanes);
    if (grid == 0) return SX_ERR_UNSUPPORTED;
    const size_t lds = mlp_lds_doubles(arch.n_hidden, arch.wmax) * sizeof(double);
    if (int r = allow_lds(cem_rollout_mlp_kernel<NS, NU, 0, true>, lds)) return r;
    launch(SX_PROF_ROLLOUT_MLP, cem_rollout_mlp_kernel<NS, NU, 0, true>, dim3(grid), dim3(kMlpLanes), lds, stream, table, rc,
           cc, rp);
    return check_launch();
}

}  // namespace sx

#define SX_MODEL_MULTI_INSTANTIATE(NS, NU)                                                                              \
    template int sx::launch_rollout_feat_multi<NS, NU>(const sx::FeatConst*, const sx::ReachConst<NS, NU>&,            \
                                                       const sx::CostConst<SX_MAX_M, NS, NU>&,                         \
                                                       const sx::FeatRolloutPtrs&, hipStream_t);                       \
    template int sx::launch_rollout_mlp_multi<NS, NU>(const sx::MlpConst*, const sx::MlpConst&, bool,                  \
                                                      const sx::ReachConst<NS, NU>&,                                   \
                                                      const sx::CostConst<SX_MAX_M, NS, NU>&,                          \
                                                      const sx::FeatRolloutPtrs&, hipStream_t);
#define SX_MODEL_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_MODEL_MULTI_INSTANTIATE(NS, NU))
SX_ROLLOUT_SHAPES(SX_MODEL_MULTI_ONE, 0)
