// Streaming rollout kernels with the SafeMPC constraint set in finish() in the multi-model mode (sx_cem_rollout_cons_multi,
// sx_cem_rollout_elites_cons_multi without a cost; cem_rollout_kernel<StreamCons<false, true>, ...>): every shift-0
// shape of SX_ROLLOUT_SHAPES in both forms.  The set is one argument shared by all problems.
#include "sx_stream_impl.hpp"

#define SX_CONS_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamCons<false, true>))
SX_ROLLOUT_SHAPES(SX_CONS_MULTI_ONE, 0)
