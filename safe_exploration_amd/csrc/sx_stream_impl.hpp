// Body of launch_stream<V, NS, NU> (sx_stream_launch.hpp), the one launcher of the streaming rollout kernels; included by
// sx_stream_ns*.hip, sx_stream_multi.hip, sx_stream_starts.hip, sx_stream_sat.hip, sx_stream_sat_multi.hip,
// sx_stream_cons.hip, sx_stream_cons_sat.hip, sx_stream_cons_multi.hip, sx_stream_cons_sat_multi.hip,
// sx_stream_starts_cons.hip, sx_stream_starts_multi.hip, sx_stream_starts_cons_multi.hip and sx_stream_gains.hip, which instantiate it for their variant V and so compile that variant's kernels.
#pragma once
#include <climits>
#include <tuple>
#include <type_traits>

#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"

namespace sx {

// a trailing kernel argument the variant has, *p, as a tuple of one; none for one it has not
template <bool HAVE, class T>
auto stream_extra(const T* p) {
    if constexpr (HAVE) return std::tie(*p);
    else return std::tuple<>();
}

template <class V, int NS, int NU>
int launch_stream(const StreamGpArg<V, NS, NU>& gp, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                  const RolloutPtrs& rp, const SatConst<NS>* sat, bool byout, size_t lds, hipStream_t stream,
                  const ConConst<NS>* cons, const GainConst* gains) {
    static_assert(V::SH >= 0 && V::SH <= NU && NS + NU + V::SH <= SX_MAX_D, "query shift outside the junk-dimension shapes");
#ifdef SX_STAMPS
    if constexpr (!V::MM && !V::PS && !V::SAT && !V::CONS) {
        // this translation unit's copy of the stamp buffer pointer (sx_debug_set_stamps hands it over in rp.stamps)
        static unsigned long long* stamps = nullptr;
        if (rp.stamps != stamps && hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &rp.stamps, sizeof(rp.stamps)) == hipSuccess)
            stamps = rp.stamps;
    }
#endif
    const int64_t grid = (int64_t)rp.E * ((rp.P + SX_TILE - 1) / SX_TILE);
    if (grid > INT_MAX) return SX_ERR_UNSUPPORTED;
    // (the table's entries carry a stage table each)
    const int4* stage_tab = nullptr;
    if constexpr (!V::MM) stage_tab = gp.stage_tab;
    // the trailing arguments [*cons][, *sat] | *gains of V, and its kernel over them
    return std::apply(
        [&](const auto&... extras) {
            const auto kernel = byout ? cem_rollout_kernel<V, NS, NU, true, std::decay_t<decltype(extras)>...>
                                      : cem_rollout_kernel<V, NS, NU, false, std::decay_t<decltype(extras)>...>;
            if (int r = allow_lds(kernel, lds)) return r;
            launch(SX_PROF_ROLLOUT_FUSED, kernel, dim3((unsigned)grid), dim3(kRolloutThreads), lds, stream, gp, stage_tab, rc,
                   cc, rp, extras...);
            return check_launch();
        },
        std::tuple_cat(stream_extra<V::CONS>(cons), stream_extra<V::SAT>(sat), stream_extra<V::KF>(gains)));
}

}  // namespace sx

// launch_stream of variant V (the trailing argument: StreamPlain<SH>, StreamPlain<0, true>, StreamStarts, StreamSat<MM>,
// StreamCons<SAT, MM>, StreamStartsCons, StreamStartsMulti, StreamStartsConsMulti, StreamGains)
#define SX_STREAM_INSTANTIATE(NS, NU, ...)                                                                            \
    template int sx::launch_stream<sx::__VA_ARGS__, NS, NU>(                                                          \
        const sx::StreamGpArg<sx::__VA_ARGS__, NS, NU>&, const sx::ReachConst<NS, NU>&,                               \
        const sx::CostConst<SX_MAX_M, NS, NU>&, const sx::RolloutPtrs&, const sx::SatConst<NS>*, bool, size_t, hipStream_t, \
        const sx::ConConst<NS>*, const sx::GainConst*);
