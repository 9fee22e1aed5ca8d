// Streaming rollout kernels with a start state per particle and the SafeMPC constraint set in the multi-model mode
// (sx_cem_rollout_starts_cons_multi; cem_rollout_kernel<StreamStartsConsMulti, ...>): every shift-0 shape of
// SX_ROLLOUT_SHAPES in both forms.  The set is one argument shared by all problems.
#include "sx_stream_impl.hpp"

#define SX_STARTS_CONS_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamStartsConsMulti))
SX_ROLLOUT_SHAPES(SX_STARTS_CONS_MULTI_ONE, 0)
