// Streaming rollout kernels with the saturating cost on the safety ellipsoids as the objective (sx_cem_rollout_sat,
// sx_cem_rollout_elites_sat; cem_rollout_kernel<StreamSat<false>, ...>): every shift-0 shape of SX_ROLLOUT_SHAPES in both
// forms.  A translation unit of its own: nothing the other objects compile changes with it.
#include "sx_stream_impl.hpp"

#define SX_SAT_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamSat<false>))
SX_ROLLOUT_SHAPES(SX_SAT_ONE, 0)
