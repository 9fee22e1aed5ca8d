// Streaming rollout kernels (sx_cem_rollout, sx_cem_rollout_junk) for state dimensions 1 and 2.
#include "sx_stream_impl.hpp"

SX_STREAM_INSTANTIATE(1, 1, StreamPlain<0>)
SX_STREAM_INSTANTIATE(2, 1, StreamPlain<0>)
SX_STREAM_INSTANTIATE(2, 2, StreamPlain<0>)
SX_STREAM_INSTANTIATE(1, 1, StreamPlain<1>)
SX_STREAM_INSTANTIATE(2, 1, StreamPlain<1>)
SX_STREAM_INSTANTIATE(2, 2, StreamPlain<1>)
SX_STREAM_INSTANTIATE(2, 2, StreamPlain<2>)
