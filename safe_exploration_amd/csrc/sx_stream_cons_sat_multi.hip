// Streaming rollout kernels with the SafeMPC constraint set in finish() and the saturating cost on the safety ellipsoids
// as the objective, in the multi-model mode (sx_cem_rollout_cons_multi, sx_cem_rollout_elites_cons_multi with a cost;
// cem_rollout_kernel<StreamCons<true, true>, ...>): every shift-0 shape of SX_ROLLOUT_SHAPES in both forms.  A
// translation unit of its own, beside sx_stream_cons_multi.hip, so that the two build in parallel.
#include "sx_stream_impl.hpp"

#define SX_CONS_SAT_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamCons<true, true>))
SX_ROLLOUT_SHAPES(SX_CONS_SAT_MULTI_ONE, 0)
