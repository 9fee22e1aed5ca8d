// The Taylor performance kernel with the saturating cost in the multi-model mode (sx_cem_perf_rollout_taylor_sat_multi):
// every shift-0 shape of SX_ROLLOUT_SHAPES in both forms, and its launcher.  A translation unit of its own: nothing the
// other objects compile changes with it.
#include <climits>

#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES
#include "sx_perf_launch.hpp"
#include "sx_perf_taylor.hpp"

namespace sx {

template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const PerfTaylorSatConst<NS, NU>& c, const PerfTaylorPtrs& tp,
                         bool byout, unsigned blocks, size_t lds, hipStream_t stream) {
    return launch_perf_gp_forms<PerfTaylorKind<true>, NS, NU>(byout, blocks, lds, stream, table, c, tp);
}

}  // namespace sx

#define SX_TAYLOR_SAT_MULTI_INSTANTIATE(NS, NU)                                                                       \
    template int sx::launch_perf_gp_multi<NS, NU>(const sx::GpConst<NS, NS + NU>*, const sx::PerfTaylorSatConst<NS, NU>&, \
                                                  const sx::PerfTaylorPtrs&, bool, unsigned, size_t, hipStream_t);
#define SX_TAYLOR_SAT_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_TAYLOR_SAT_MULTI_INSTANTIATE(NS, NU))
SX_ROLLOUT_SHAPES(SX_TAYLOR_SAT_MULTI_ONE, 0)
