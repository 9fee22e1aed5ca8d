// Streaming rollout kernels with a start state per particle in the multi-model mode (sx_cem_rollout_starts_multi;
// cem_rollout_kernel<StreamStartsMulti, ...>): every shift-0 shape of SX_ROLLOUT_SHAPES in both forms.  A translation
// unit of its own: nothing the other objects compile changes with it.
#include "sx_stream_impl.hpp"

#define SX_STARTS_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamStartsMulti))
SX_ROLLOUT_SHAPES(SX_STARTS_MULTI_ONE, 0)
