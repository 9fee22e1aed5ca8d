// Bodies of launch_rollout_stream<NS, NU, SH>, launch_rollout_stream_multi<NS, NU>, launch_rollout_starts<NS, NU>,
// launch_rollout_sat<NS, NU> and launch_rollout_sat_multi<NS, NU>; included by sx_stream_ns*.hip, sx_stream_multi.hip,
// sx_stream_starts.hip, sx_stream_sat.hip and sx_stream_sat_multi.hip, which instantiate them.
#pragma once
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"

namespace sx {

template <int NS, int NU, int SH>
int launch_rollout_stream(const GpConst<NS, NS + NU + SH>& gc, const ReachConst<NS, NU>& rc,
                          const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool byout, size_t lds,
                          hipStream_t stream) {
    static_assert(SH >= 0 && SH <= NU && NS + NU + SH <= SX_MAX_D, "query shift outside the junk-dimension shapes");
#ifdef SX_STAMPS
    // this translation unit's copy of the stamp buffer pointer (sx_debug_set_stamps hands it over in rp.stamps)
    static unsigned long long* stamps = nullptr;
    if (rp.stamps != stamps && hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &rp.stamps, sizeof(rp.stamps)) == hipSuccess)
        stamps = rp.stamps;
#endif
    const int tiles = (rp.P + SX_TILE - 1) / SX_TILE;
    if (byout) {
        if (int r = allow_lds(cem_rollout_kernel<NS, NU, true, SH>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_kernel<NS, NU, true, SH>, dim3(rp.E * tiles), dim3(kRolloutThreads), lds,
               stream, gc, gc.stage_tab, rc, cc, rp);
    } else {
        if (int r = allow_lds(cem_rollout_kernel<NS, NU, false, SH>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_kernel<NS, NU, false, SH>, dim3(rp.E * tiles), dim3(kRolloutThreads), lds,
               stream, gc, gc.stage_tab, rc, cc, rp);
    }
    return check_launch();
}

template <int NS, int NU>
int launch_rollout_stream_multi(const GpConst<NS, NS + NU>* table, const ReachConst<NS, NU>& rc,
                                const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool byout, size_t lds,
                                hipStream_t stream) {
    const int tiles = (rp.P + SX_TILE - 1) / SX_TILE;
    if (byout) {
        if (int r = allow_lds(cem_rollout_kernel<NS, NU, true, 0, true>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_kernel<NS, NU, true, 0, true>, dim3(rp.E * tiles), dim3(kRolloutThreads),
               lds, stream, table, (const int4*)nullptr, rc, cc, rp);
    } else {
        if (int r = allow_lds(cem_rollout_kernel<NS, NU, false, 0, true>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_kernel<NS, NU, false, 0, true>, dim3(rp.E * tiles), dim3(kRolloutThreads),
               lds, stream, table, (const int4*)nullptr, rc, cc, rp);
    }
    return check_launch();
}

template <int NS, int NU>
int launch_rollout_starts(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc,
                          const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool byout, size_t lds,
                          hipStream_t stream) {
    const int tiles = (rp.P + SX_TILE - 1) / SX_TILE;
    if (byout) {
        if (int r = allow_lds(cem_rollout_starts_kernel<NS, NU, true>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_starts_kernel<NS, NU, true>, dim3(rp.E * tiles), dim3(kRolloutThreads),
               lds, stream, gc, gc.stage_tab, rc, cc, rp);
    } else {
        if (int r = allow_lds(cem_rollout_starts_kernel<NS, NU, false>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_starts_kernel<NS, NU, false>, dim3(rp.E * tiles), dim3(kRolloutThreads),
               lds, stream, gc, gc.stage_tab, rc, cc, rp);
    }
    return check_launch();
}

template <int NS, int NU>
int launch_rollout_sat(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                       const RolloutPtrs& rp, const SatConst<NS>& sat, bool byout, size_t lds, hipStream_t stream) {
    const int tiles = (rp.P + SX_TILE - 1) / SX_TILE;
    if (byout) {
        if (int r = allow_lds(cem_rollout_sat_kernel<NS, NU, true, false>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_sat_kernel<NS, NU, true, false>, dim3(rp.E * tiles),
               dim3(kRolloutThreads), lds, stream, gc, gc.stage_tab, rc, cc, rp, sat);
    } else {
        if (int r = allow_lds(cem_rollout_sat_kernel<NS, NU, false, false>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_sat_kernel<NS, NU, false, false>, dim3(rp.E * tiles),
               dim3(kRolloutThreads), lds, stream, gc, gc.stage_tab, rc, cc, rp, sat);
    }
    return check_launch();
}

template <int NS, int NU>
int launch_rollout_sat_multi(const GpConst<NS, NS + NU>* table, const ReachConst<NS, NU>& rc,
                             const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, const SatConst<NS>& sat,
                             bool byout, size_t lds, hipStream_t stream) {
    const int tiles = (rp.P + SX_TILE - 1) / SX_TILE;
    if (byout) {
        if (int r = allow_lds(cem_rollout_sat_kernel<NS, NU, true, true>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_sat_kernel<NS, NU, true, true>, dim3(rp.E * tiles), dim3(kRolloutThreads),
               lds, stream, table, (const int4*)nullptr, rc, cc, rp, sat);
    } else {
        if (int r = allow_lds(cem_rollout_sat_kernel<NS, NU, false, true>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_sat_kernel<NS, NU, false, true>, dim3(rp.E * tiles), dim3(kRolloutThreads),
               lds, stream, table, (const int4*)nullptr, rc, cc, rp, sat);
    }
    return check_launch();
}

}  // namespace sx

#define SX_STREAM_SAT_INSTANTIATE(NS, NU)                                                                             \
    template int sx::launch_rollout_sat<NS, NU>(                                                                      \
        const sx::GpConst<NS, NS + NU>&, const sx::ReachConst<NS, NU>&, const sx::CostConst<SX_MAX_M, NS, NU>&,      \
        const sx::RolloutPtrs&, const sx::SatConst<NS>&, bool, size_t, hipStream_t);

#define SX_STREAM_SAT_MULTI_INSTANTIATE(NS, NU)                                                                       \
    template int sx::launch_rollout_sat_multi<NS, NU>(                                                                \
        const sx::GpConst<NS, NS + NU>*, const sx::ReachConst<NS, NU>&, const sx::CostConst<SX_MAX_M, NS, NU>&,      \
        const sx::RolloutPtrs&, const sx::SatConst<NS>&, bool, size_t, hipStream_t);

#define SX_STREAM_STARTS_INSTANTIATE(NS, NU)                                                                         \
    template int sx::launch_rollout_starts<NS, NU>(                                                                   \
        const sx::GpConst<NS, NS + NU>&, const sx::ReachConst<NS, NU>&, const sx::CostConst<SX_MAX_M, NS, NU>&,      \
        const sx::RolloutPtrs&, bool, size_t, hipStream_t);

#define SX_STREAM_MULTI_INSTANTIATE(NS, NU)                                                                             \
    template int sx::launch_rollout_stream_multi<NS, NU>(                                                              \
        const sx::GpConst<NS, NS + NU>*, const sx::ReachConst<NS, NU>&, const sx::CostConst<SX_MAX_M, NS, NU>&,       \
        const sx::RolloutPtrs&, bool, size_t, hipStream_t);

#define SX_STREAM_INSTANTIATE(NS, NU, SH)                                                                            \
    template int sx::launch_rollout_stream<NS, NU, SH>(                                                               \
        const sx::GpConst<NS, NS + NU + SH>&, const sx::ReachConst<NS, NU>&, const sx::CostConst<SX_MAX_M, NS, NU>&, \
        const sx::RolloutPtrs&, bool, size_t, hipStream_t);
