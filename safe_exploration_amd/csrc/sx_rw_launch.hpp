// Launcher of the register-resident rollout kernels (sx_rollout_rw.hpp).  Its instantiations are compiled in translation
// units of their own (sx_rw_ns{1..4}.hip: one per state dimension, built in parallel); sx_gp_rollout.hip sees the declaration.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_reach.hpp"
#include "sx_rollout.hpp"

namespace sx {

constexpr int kRwWaves = 4;   // one wave per SIMD, 512 registers each

// largest n_pad / 16 whose W fits the register budget next to the step's working set, i.e. that compiles without a
// scratch spill (checked over all instantiations with tools/kernel_resources.py after every change of the kernel)
constexpr int rw_max_nrb(int ns, int nu) {
    return ns == 1 ? 18 : ns == 2 ? (nu == 1 ? 13 : 12) : ns == 3 ? 8 : (nu == 1 ? 6 : 5);
}


// cem_rollout_rh_kernel (eight waves of 256 registers): instantiated where finish() and the Kstar phase leave room for the
// resident pairs without a scratch spill -- n_s <= 2; at n_s >= 3 their working sets (Jacobi sweeps on 3 x 3 / 4 x 4
// matrices, 2 n_s exponential chains) do not (tools/kernel_resources.py: (2, 2, 10) and every n_s >= 3 instantiation spill)
constexpr int rh_max_nrb(int ns, int nu) { return ns == 1 ? 18 : ns == 2 ? (nu == 1 ? 13 : 8) : 0; }

// Dynamic LDS bytes of cem_rollout_rh_kernel / cem_rollout_rw_kernel<NS, NU, n_pad / 16>; ~0 where n_pad / 16 has no
// instantiation.  No HIP call.
template <int NS, int NU>
size_t rollout_rh_lds_bytes(int n_train, int n_pad, int H);
template <int NS, int NU>
size_t rollout_rw_lds_bytes(int n_train, int n_pad, int H);

// Launch cem_rollout_rh_kernel (sx_rollout_rh.hpp: eight waves, W partly resident) / cem_rollout_rw_kernel
// (sx_rollout_rw.hpp: four waves, W in the register file) for nrb = n_pad / 16 with `lds` bytes (rollout_*_lds_bytes) of
// dynamic LDS on `stream`.
template <int NS, int NU>
int launch_rollout_rh(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                      const RolloutPtrs& rp, int nrb, size_t lds, hipStream_t stream);
template <int NS, int NU>
int launch_rollout_rw(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                      const RolloutPtrs& rp, int nrb, size_t lds, hipStream_t stream);

}  // namespace sx
