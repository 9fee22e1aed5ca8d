// Query-shifted streaming rollout kernels (sx_cem_rollout_junk) for state dimensions 3 and 4.
#include "sx_junk_impl.hpp"

SX_JUNK_INSTANTIATE(3, 1, 1)
SX_JUNK_INSTANTIATE(3, 2, 1)
SX_JUNK_INSTANTIATE(4, 1, 1)
