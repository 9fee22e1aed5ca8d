// Query-shifted streaming rollout kernels (sx_cem_rollout_junk) for state dimensions 1 and 2.
#include "sx_junk_impl.hpp"

SX_JUNK_INSTANTIATE(1, 1, 1)
SX_JUNK_INSTANTIATE(2, 1, 1)
SX_JUNK_INSTANTIATE(2, 2, 1)
SX_JUNK_INSTANTIATE(2, 2, 2)
