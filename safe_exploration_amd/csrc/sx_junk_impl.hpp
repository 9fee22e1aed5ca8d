// Body of launch_rollout_shifted<NS, NU, SH>; included by sx_junk_ns*.hip, which instantiate it.
#pragma once
#include "sx_junk_launch.hpp"
#include "sx_launch.hpp"

namespace sx {

template <int NS, int NU, int SH>
int launch_rollout_shifted(const GpConst<NS, NS + NU + SH>& gc, const ReachConst<NS, NU>& rc,
                           const CostConst<SX_MAX_M, NS, NU>& cc, const RolloutPtrs& rp, bool all_at_once, size_t lds,
                           hipStream_t stream) {
    static_assert(SH >= 1 && SH <= NU && NS + NU + SH <= SX_MAX_D, "query shift outside the junk-dimension shapes");
    const int tiles = (rp.P + SX_TILE - 1) / SX_TILE;
    if (all_at_once) {
        if (int r = allow_lds(cem_rollout_kernel<NS, NU, false, SH>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_kernel<NS, NU, false, SH>, dim3(rp.E * tiles), dim3(kRolloutThreads), lds,
               stream, gc, gc.stage_tab, rc, cc, rp);
    } else {
        if (int r = allow_lds(cem_rollout_kernel<NS, NU, true, SH>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_kernel<NS, NU, true, SH>, dim3(rp.E * tiles), dim3(kRolloutThreads), lds,
               stream, gc, gc.stage_tab, rc, cc, rp);
    }
    return check_launch();
}

}  // namespace sx

#define SX_JUNK_INSTANTIATE(NS, NU, SH)                                                                             \
    template int sx::launch_rollout_shifted<NS, NU, SH>(                                                              \
        const sx::GpConst<NS, NS + NU + SH>&, const sx::ReachConst<NS, NU>&, const sx::CostConst<SX_MAX_M, NS, NU>&, \
        const sx::RolloutPtrs&, bool, size_t, hipStream_t);
