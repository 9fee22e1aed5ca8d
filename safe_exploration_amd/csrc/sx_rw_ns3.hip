// Register-resident rollout kernels (sx_rollout_rw.hpp, sx_rollout_rh.hpp) for state dimension 3: every n_pad / 16 that fits.
#include "sx_rw_impl.hpp"

namespace sx {
SX_RW_INSTANTIATE(3, 1)
}  // namespace sx
