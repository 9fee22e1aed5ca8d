// The Taylor performance-trajectory kernel in the multi-model mode (sx_cem_perf_rollout_taylor_multi): every shift-0 shape
// of SX_ROLLOUT_SHAPES in both forms, and its launcher.  A translation unit of its own: nothing the other objects compile
// changes with it.
#include <climits>

#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES
#include "sx_perf_launch.hpp"
#include "sx_perf_taylor.hpp"

namespace sx {

template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const PerfTaylorConst<NS, NU>& tc, const PerfTaylorPtrs& tp,
                             bool byout, unsigned blocks, size_t lds, hipStream_t stream) {
    return launch_perf_gp_forms<PerfTaylorKind<false>, NS, NU>(byout, blocks, lds, stream, table, tc, tp);
}

}  // namespace sx

#define SX_TAYLOR_MULTI_INSTANTIATE(NS, NU)                                                                        \
    template int sx::launch_perf_gp_multi<NS, NU>(const sx::GpConst<NS, NS + NU>*, const sx::PerfTaylorConst<NS, NU>&, \
                                                      const sx::PerfTaylorPtrs&, bool, unsigned, size_t, hipStream_t);
#define SX_TAYLOR_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_TAYLOR_MULTI_INSTANTIATE(NS, NU))
SX_ROLLOUT_SHAPES(SX_TAYLOR_MULTI_ONE, 0)
