// The Taylor performance-trajectory kernel in the multi-model mode (sx_cem_perf_rollout_taylor_multi): every shift-0 shape
// of SX_ROLLOUT_SHAPES in both forms, and its launcher.  A translation unit of its own: nothing the other objects compile
// changes with it.
#include <climits>

#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES
#include "sx_perf_launch.hpp"
#include "sx_perf_taylor.hpp"

namespace sx {

static_assert(kPerfVarThreads == kRolloutThreads, "the stage table of sx_gp_pack is cut for the safety kernel's waves");

template <int NS, int NU, bool BYOUT>
static int launch_perf_taylor_multi_form(const GpConst<NS, NS + NU>* table, const PerfTaylorConst<NS, NU>& tc,
                                         const PerfTaylorPtrs& tp, unsigned blocks, size_t lds, hipStream_t stream) {
    if (int r = allow_lds(cem_perf_taylor_rollout_multi_kernel<NS, NU, BYOUT>, lds)) return r;
    hipLaunchKernelGGL((cem_perf_taylor_rollout_multi_kernel<NS, NU, BYOUT>), dim3(blocks), dim3(kPerfVarThreads), lds,
                       stream, table, tc, tp);
    return check_launch();
}

template <int NS, int NU>
int launch_perf_taylor_multi(const GpConst<NS, NS + NU>* table, const PerfTaylorConst<NS, NU>& tc, const PerfTaylorPtrs& tp,
                             bool byout, size_t lds, hipStream_t stream) {
    const int64_t blocks = (int64_t)tp.v.p.E * ((tp.v.p.P + SX_TILE - 1) / SX_TILE);
    if (blocks > INT_MAX || lds > kMaxLdsBytes) return SX_ERR_UNSUPPORTED;
    if constexpr (NS > 1) {
        if (byout) return launch_perf_taylor_multi_form<NS, NU, true>(table, tc, tp, (unsigned)blocks, lds, stream);
    }
    return launch_perf_taylor_multi_form<NS, NU, false>(table, tc, tp, (unsigned)blocks, lds, stream);
}

}  // namespace sx

#define SX_PERF_TAYLOR_MULTI_INSTANTIATE(NS, NU)                                                                        \
    template int sx::launch_perf_taylor_multi<NS, NU>(const sx::GpConst<NS, NS + NU>*, const sx::PerfTaylorConst<NS, NU>&, \
                                                      const sx::PerfTaylorPtrs&, bool, size_t, hipStream_t);
#define SX_PERF_TAYLOR_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_PERF_TAYLOR_MULTI_INSTANTIATE(NS, NU))
SX_ROLLOUT_SHAPES(SX_PERF_TAYLOR_MULTI_ONE, 0)
