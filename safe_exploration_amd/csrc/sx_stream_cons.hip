// Streaming rollout kernels with the SafeMPC constraint set in finish() and the objective of env->obj_mode
// (sx_cem_rollout_cons, sx_cem_rollout_elites_cons with cost == NULL; cem_rollout_kernel<StreamCons<false>, ...>): every
// shift-0 shape of SX_ROLLOUT_SHAPES in both forms.  A translation unit of its own: nothing the other objects compile
// changes with it.
#include "sx_stream_impl.hpp"

#define SX_CONS_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_STREAM_INSTANTIATE(NS, NU, StreamCons<false>))
SX_ROLLOUT_SHAPES(SX_CONS_ONE, 0)
