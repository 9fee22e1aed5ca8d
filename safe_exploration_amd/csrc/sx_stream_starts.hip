// Streaming rollout kernels with a start state per particle (sx_cem_rollout_starts): every shift-0 shape of
// SX_ROLLOUT_SHAPES.
#include "sx_stream_impl.hpp"

#define SX_STARTS_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamStarts))
SX_ROLLOUT_SHAPES(SX_STARTS_ONE, 0)
