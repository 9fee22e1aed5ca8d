// Streaming rollout kernels with the saturating cost on the safety ellipsoids in the multi-model mode
// (sx_cem_rollout_sat_multi, sx_cem_rollout_elites_sat_multi; cem_rollout_kernel<StreamSat<true>, ...>): every shift-0
// shape of SX_ROLLOUT_SHAPES in both forms.
#include "sx_stream_impl.hpp"

#define SX_SAT_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamSat<true>))
SX_ROLLOUT_SHAPES(SX_SAT_MULTI_ONE, 0)
