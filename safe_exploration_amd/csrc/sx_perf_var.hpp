// The performance trajectory of the CEM solver WITH the GP's posterior variance (sx_cem_perf_rollout_var): n_perf chained
// mean-equivalent steps per particle,
//     (mean_t, var_t) = GP posterior at [mu_t, v_t],      mu_{t+1} = a mu_t + b v_t + mean_t,
// no feedback term, no variance propagation (sigma_x = None), and var_t = s + noise - || W k* ||^2 per output: the N x N
// triangular product of the safety kernels on the f64 matrix cores, where the mean-only kernel (sx_perf.hpp) needs k* . alpha.
//
// Layout: the skeleton of the streaming safety kernel (sx_rollout.hpp) without its finish().  One workgroup of SX_WAVES
// waves owns a tile of 16 particles of one problem for all n_perf steps; the packed model is the safety rollout's (W
// fragments, the mean / Jacobian rows, the stage table of sx_gp_pack).  Step t:
//     Kstar(t) on all waves, equal shares  |sync|  MFMA(t)  |sync|  gp_collect + the step's tail on the 16 owner lanes
// Every Kstar thread derives its query point of step t + 1 from z_t and the posterior means MFMA(t) left in LDS (the
// next_centre fma chain of the safety kernel), so the owner lanes' tail -- next centre, objective, action box, stores --
// runs beside the start of Kstar(t + 1) and costs no third barrier.  z lives in two LDS buffers, as in the safety kernel:
// the owner writes z_{t+1} into buffer (t + 1) & 1 for the threads of step t + 2.
// The stage stream carries the folded Jacobian rows R_d[1 .. D], which this kernel computes and ignores: they ride in the
// row-blocks that hold the mean row and the zero padding anyway, so no MFMA is issued for them alone.
//
// BYOUT = true: output by output (Kstar_d | MFMA_d for d = 0 .. n_s - 1, 2 n_s barriers per step), for training sets whose
// n_s Kstar buffers do not fit in LDS together -- the same per-output stage streams as the safety kernel's.
// A tile's numbers depend on its 16 particles alone: not on P, the grid or the workgroup it lands in.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_perf.hpp"   // PerfStepConst, PerfPtrs

namespace sx {

constexpr int kPerfVarThreads = 64 * SX_WAVES;

struct PerfVarPtrs {
    PerfPtrs p;
    double* perf_sigma;   // [E x P x n_perf x NS] | NULL: var_0 .. var_{n_perf - 1}
    int obj_mode;         // SX_OBJ_NEG_VARIANCE | SX_OBJ_AFFINE_ABS
};

template <int NS, int NU, bool BYOUT>
__global__ __launch_bounds__(kPerfVarThreads) void cem_perf_var_rollout_kernel(const GpConst<NS, NS + NU> gc,
                                                                               const int4* __restrict__ stage_tab,
                                                                               const PerfStepConst<NS, NU> sc,
                                                                               const PerfVarPtrs vp) {
    constexpr bool MM = false;
#define SX_PERF_TAYLOR 0
#include "sx_perf_gp_body.inc"
#undef SX_PERF_TAYLOR
}

// sx_cem_perf_rollout_var_multi: a GP per problem.  The workgroup binds its problem's GpConst through a restrict-qualified
// pointer into the constant address space (scalar loads; the kernel never writes the table).
template <int NS, int NU, bool BYOUT>
__global__ __launch_bounds__(kPerfVarThreads) void cem_perf_var_rollout_multi_kernel(
    const GpConst<NS, NS + NU>* __restrict__ table, const PerfStepConst<NS, NU> sc, const PerfVarPtrs vp) {
    constexpr bool MM = true;
    using ConstG = __attribute__((address_space(4))) const GpConst<NS, NS + NU>;
    const int problem = blockIdx.x / ((vp.p.P + SX_TILE - 1) / SX_TILE);
    const GpConst<NS, NS + NU>& gc = *(const GpConst<NS, NS + NU>*)((ConstG*)table + problem);
    const int4* __restrict__ const stage_tab = gc.stage_tab;
#define SX_PERF_TAYLOR 0
#include "sx_perf_gp_body.inc"
#undef SX_PERF_TAYLOR
}

}  // namespace sx
