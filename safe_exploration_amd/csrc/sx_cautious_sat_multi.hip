// The cautious rollout kernel with the saturating cost in the multi-model mode (sx_cem_cautious_rollout_sat_multi):
// cem_cautious_rollout_kernel<..., SAT = true, MM = true> (sx_cautious.hpp) for every shift-0 shape of SX_ROLLOUT_SHAPES in
// both forms, and its launcher.  A translation unit of its own: nothing the other objects compile changes with it.
#include "sx_cautious_host.hpp"   // launch_cautious_forms

namespace sx {

template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const CautiousSatConst<NS, NU>& c, const CautiousPtrs& cp,
                         bool byout, unsigned blocks, size_t lds, hipStream_t stream) {
    return launch_cautious_forms<true, NS, NU>(byout, blocks, lds, stream, table, c, cp);
}

}  // namespace sx

#define SX_CAUTIOUS_SAT_MULTI_INSTANTIATE(NS, NU)                                                                       \
    template int sx::launch_perf_gp_multi<NS, NU>(const sx::GpConst<NS, NS + NU>*, const sx::CautiousSatConst<NS, NU>&, \
                                                  const sx::CautiousPtrs&, bool, unsigned, size_t, hipStream_t);
#define SX_CAUTIOUS_SAT_MULTI_ONE(NS, NU, SH, unused) SX_SHIFT0_##SH(SX_CAUTIOUS_SAT_MULTI_INSTANTIATE(NS, NU))
SX_ROLLOUT_SHAPES(SX_CAUTIOUS_SAT_MULTI_ONE, 0)
