// Streaming rollout kernels with a feedback gain per particle and step (sx_cem_rollout_gains;
// cem_rollout_kernel<StreamGains, ...>): every shift-0 shape of SX_ROLLOUT_SHAPES in both forms.  A translation unit of its
// own, compiled beside the others.
#include "sx_stream_impl.hpp"

#define SX_GAINS_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamGains))
SX_ROLLOUT_SHAPES(SX_GAINS_ONE, 0)
