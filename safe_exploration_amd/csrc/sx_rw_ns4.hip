// Register-resident rollout kernels (sx_rollout_rw.hpp, sx_rollout_rh.hpp) for state dimension 4: every n_pad / 16 that fits.
#include "sx_rw_impl.hpp"

namespace sx {
SX_RW_INSTANTIATE(4, 1)
SX_RW_INSTANTIATE(4, 2)
}  // namespace sx
