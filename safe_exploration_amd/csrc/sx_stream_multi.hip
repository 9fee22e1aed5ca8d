// Streaming rollout kernels in the multi-model mode (sx_cem_rollout_multi): every shift-0 shape of SX_ROLLOUT_SHAPES.
#include "sx_stream_impl.hpp"

#define SX_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamPlain<0, true>))
SX_ROLLOUT_SHAPES(SX_MULTI_ONE, 0)
