// Streaming rollout kernels (sx_cem_rollout, sx_cem_rollout_junk) for state dimensions 3 and 4.
#include "sx_stream_impl.hpp"

SX_STREAM_INSTANTIATE(3, 1, StreamPlain<0>)
SX_STREAM_INSTANTIATE(4, 1, StreamPlain<0>)
SX_STREAM_INSTANTIATE(4, 2, StreamPlain<0>)
SX_STREAM_INSTANTIATE(3, 1, StreamPlain<1>)
SX_STREAM_INSTANTIATE(3, 2, StreamPlain<1>)
SX_STREAM_INSTANTIATE(4, 1, StreamPlain<1>)
