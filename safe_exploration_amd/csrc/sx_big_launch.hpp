// Launchers of the large-N path (sx_big.hpp: Kstar in HBM, for training sets beyond the LDS budget of the single-launch
// kernels), which sx_gp_predict and sx_cem_rollout share.  Their instantiations -- every shift-0 shape of
// SX_ROLLOUT_SHAPES -- are compiled in a translation unit of their own (sx_big.hip), so that each of its kernels exists
// once; sx_gp_predict.hip and sx_gp_rollout.hip see the declarations.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_rollout.hpp"

namespace sx {

// sx_gp_predict over `workspace` (big_ws_layout doubles for P points; SX_ERR_ARG if absent or too small)
template <int NS, int NU>
int launch_predict_big(const sx_gp_model* m, const double* z, int P, double* mean, double* var, double* jac,
                       double* workspace, int64_t workspace_bytes, hipStream_t stream);

// sx_cem_rollout over `workspace` (big_ws_layout doubles for E P particles): three launches per step
template <int NS, int NU>
int launch_rollout_big(const sx_gp_model* m, const sx_env* env, const RolloutPtrs& rp, double* workspace,
                       int64_t workspace_bytes, hipStream_t stream);

}  // namespace sx
