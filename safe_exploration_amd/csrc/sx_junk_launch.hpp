// Launcher of the query-shifted streaming rollout (cem_rollout_kernel<NS, NU, BYOUT, SH>, SH > 0: sx_cem_rollout_junk).
// Its instantiations are compiled in translation units of their own (sx_junk_ns12.hip, sx_junk_ns34.hip, built in
// parallel with the rest); sx_kernels.hip sees the declaration.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_reach.hpp"
#include "sx_rollout.hpp"

namespace sx {

// Launches cem_rollout_kernel<NS, NU, !all_at_once, SH> with `lds` bytes of dynamic LDS on `stream`.  The caller has
// checked the LDS budget (fused_fits with the GP width NS + NU + SH).
template <int NS, int NU, int SH>
int launch_rollout_shifted(const GpConst<NS, NS + NU + SH>& gc, const ReachConst<NS, NU>& rc,
                           const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool all_at_once, size_t lds,
                           hipStream_t stream);

}  // namespace sx
