// Launchers of the feature-GP and MC-dropout rollout kernels in the multi-model mode (MM = true: a model per problem,
// sx_cem_rollout_feat_multi / sx_cem_rollout_mlp_multi).  Their instantiations are compiled in a translation unit of
// their own (sx_model_multi.hip, every shift-0 shape of SX_ROLLOUT_SHAPES); sx_feat.hip and sx_mlp.hip see the declarations.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_feat.hpp"
#include "sx_mlp.hpp"
#include "sx_reach.hpp"

namespace sx {

// Launches cem_rollout_feat_kernel<NS, NU, 0, true> over E problems with a feature GP each: `table` is the device array
// of their FeatConst (sx_feat_model_table).  rp.status holds E words.
template <int NS, int NU>
int launch_rollout_feat_multi(const FeatConst* table, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                              const FeatRolloutPtrs& rp, hipStream_t stream);

// Launches the MC-dropout rollout over E problems with an ensemble each (`table`: the device array of their MlpConst,
// sx_mlp_model_table).  `arch` is any one of the models: they share the architecture, hence the kernel -- the matrix-core
// kernel for (n_hidden, every layer 64 wide) where `mfma`, the one-particle-per-lane kernel else -- and the LDS size.
template <int NS, int NU>
int launch_rollout_mlp_multi(const MlpConst* table, const MlpConst& arch, bool mfma, const ReachConst<NS, NU>& rc,
                             const CostConst<SX_MAX_M, NS, NU>& cc, const FeatRolloutPtrs& rp, hipStream_t stream);

}  // namespace sx
