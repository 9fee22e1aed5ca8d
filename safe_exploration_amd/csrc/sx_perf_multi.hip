// The performance-trajectory kernels in the multi-model mode (sx_cem_perf_rollout_multi, sx_cem_perf_rollout_var_multi):
// every shift-0 shape of SX_ROLLOUT_SHAPES, and their launchers.  A translation unit of its own: nothing the other
// objects compile changes with it.
#include <climits>

#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES
#include "sx_perf.hpp"
#include "sx_perf_launch.hpp"

namespace sx {

template <int NS, int NU>
int launch_perf_rollout_multi(const PerfGpEntry<NS, NU>* table, const PerfStepConst<NS, NU>& step, const PerfPtrs& pp,
                              size_t lds, hipStream_t stream) {
    const int64_t blocks = (int64_t)pp.E * ((pp.P + kPerfTile - 1) / kPerfTile);
    if (blocks > INT_MAX || lds > kMaxLdsBytes) return SX_ERR_UNSUPPORTED;
    const auto kernel = cem_perf_rollout_kernel<NS, NU, true, PerfStepConst<NS, NU>>;
    if (int r = allow_lds(kernel, lds)) return r;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kPerfThreads), lds, stream, table, step, pp);
    return check_launch();
}

template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const PerfStepConst<NS, NU>& sc, const PerfVarPtrs& vp,
                          bool byout, unsigned blocks, size_t lds, hipStream_t stream) {
    return launch_perf_gp_forms<PerfVarKind, NS, NU>(byout, blocks, lds, stream, table, sc, vp);
}

}  // namespace sx

#define SX_PERF_MULTI_INSTANTIATE(NS, NU)                                                                              \
    template int sx::launch_perf_rollout_multi<NS, NU>(const sx::PerfGpEntry<NS, NU>*, const sx::PerfStepConst<NS, NU>&, \
                                                       const sx::PerfPtrs&, size_t, hipStream_t);                      \
    template int sx::launch_perf_gp_multi<NS, NU>(const sx::GpConst<NS, NS + NU>*, const sx::PerfStepConst<NS, NU>&,  \
                                                   const sx::PerfVarPtrs&, bool, unsigned, size_t,  \
                                                   hipStream_t);
#define SX_PERF_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_PERF_MULTI_INSTANTIATE(NS, NU))
SX_ROLLOUT_SHAPES(SX_PERF_MULTI_ONE, 0)
