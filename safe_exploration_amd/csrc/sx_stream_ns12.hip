// Streaming rollout kernels (sx_cem_rollout, sx_cem_rollout_junk) for state dimensions 1 and 2.
#include "sx_stream_impl.hpp"

SX_STREAM_INSTANTIATE(1, 1, 0)
SX_STREAM_INSTANTIATE(2, 1, 0)
SX_STREAM_INSTANTIATE(2, 2, 0)
SX_STREAM_INSTANTIATE(1, 1, 1)
SX_STREAM_INSTANTIATE(2, 1, 1)
SX_STREAM_INSTANTIATE(2, 2, 1)
SX_STREAM_INSTANTIATE(2, 2, 2)
