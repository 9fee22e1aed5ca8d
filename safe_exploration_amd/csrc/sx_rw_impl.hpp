// Bodies of the register-resident launchers (sx_rw_launch.hpp); included by sx_rw_ns*.hip, which instantiate them.
#pragma once
#include <type_traits>

#include "sx_launch.hpp"
#include "sx_rollout_rh.hpp"
#include "sx_rollout_rw.hpp"
#include "sx_rw_launch.hpp"

namespace sx {

// f(std::integral_constant<int, nrb>{}) for 1 <= nrb <= MAX; `none` for any other nrb
template <int MAX, typename R, typename F>
static R with_nrb(int nrb, R none, F&& f) {
    if constexpr (MAX == 0) {
        return none;
    } else {
        if (nrb == MAX) return f(std::integral_constant<int, MAX>{});
        return with_nrb<MAX - 1>(nrb, none, f);
    }
}

template <int NS, int NU>
size_t rollout_rh_lds_bytes(int n_train, int n_pad, int H) {
    return with_nrb<rh_max_nrb(NS, NU)>(n_pad >> 4, ~(size_t)0, [&](auto nrb_c) {
        return rh_lds_doubles<NS, NU, decltype(nrb_c)::value>(n_train, n_pad, H) * sizeof(double) + sizeof(RwConst<NS, NU>);
    });
}

template <int NS, int NU>
size_t rollout_rw_lds_bytes(int n_train, int n_pad, int H) {
    const int nrb = n_pad >> 4;
    if (nrb < 1 || nrb > rw_max_nrb(NS, NU)) return ~(size_t)0;
    return (gp_tile_lds_doubles(NS, NS + NU, n_train, n_pad, kRwWaves, NS) + (((size_t)SX_TILE * H * NU + 1) & ~(size_t)1) +
            (((size_t)SX_TILE * (NS + NS * NS + 3) + 1) & ~(size_t)1) + RwKstarLds<NS, NS + NU>::doubles(n_pad)) *
               sizeof(double) +
           sizeof(RwConst<NS, NU>);
}

// rw_kstar_phase's table is 2^(j/2048): the exponent constants in units of ln 2 / 2048 (a factor of 8: exact)
template <int NS, int D>
static GpConst<NS, D> in_exp2_2048_units(const GpConst<NS, D>& gc) {
    GpConst<NS, D> g8 = gc;
    for (int i = 0; i < NS * D; ++i) g8.k_nh_ils2[i] *= 8.0;
    for (int d = 0; d < NS; ++d) g8.k_log_os[d] *= 8.0;
    return g8;
}

// one workgroup fills a compute unit: a persistent grid, W loaded once per workgroup
static int resident_grid(const RolloutPtrs& rp) {
    const int tiles = rp.E * ((rp.P + SX_TILE - 1) / SX_TILE);
    return tiles < device_cus() ? tiles : device_cus();
}

template <int NS, int NU>
int launch_rollout_rh(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                      const RolloutPtrs& rp, int nrb, size_t lds, hipStream_t stream) {
    const GpConst<NS, NS + NU> g8 = in_exp2_2048_units(gc);
    return with_nrb<rh_max_nrb(NS, NU)>(nrb, (int)SX_ERR_UNSUPPORTED, [&](auto nrb_c) {
        constexpr int NRB = decltype(nrb_c)::value;
        if (int r = allow_lds(cem_rollout_rh_kernel<NS, NU, NRB>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_rh_kernel<NS, NU, NRB>, dim3(resident_grid(rp)), dim3(kRhThreads), lds, stream,
               g8, rc, cc, rp);
        return check_launch();
    });
}

template <int NS, int NU>
int launch_rollout_rw(const GpConst<NS, NS + NU>& gc, const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                      const RolloutPtrs& rp, int nrb, size_t lds, hipStream_t stream) {
    const GpConst<NS, NS + NU> g8 = in_exp2_2048_units(gc);
    return with_nrb<rw_max_nrb(NS, NU)>(nrb, (int)SX_ERR_UNSUPPORTED, [&](auto nrb_c) {
        constexpr int NRB = decltype(nrb_c)::value;
        static_assert(rw_fits<NS, NRB>(), "rw_max_nrb promises more than the register budget holds");
        if (int r = allow_lds(cem_rollout_rw_kernel<NS, NU, NRB>, lds)) return r;
        launch(SX_PROF_ROLLOUT_FUSED, cem_rollout_rw_kernel<NS, NU, NRB>, dim3(resident_grid(rp)), dim3(kRwThreads), lds, stream,
               g8, rc, cc, rp);
        return check_launch();
    });
}

}  // namespace sx

#define SX_RW_INSTANTIATE(NS, NU)                                                                                         \
    template size_t rollout_rh_lds_bytes<NS, NU>(int, int, int);                                                          \
    template size_t rollout_rw_lds_bytes<NS, NU>(int, int, int);                                                          \
    template int launch_rollout_rh<NS, NU>(const GpConst<NS, NS + NU>&, const ReachConst<NS, NU>&,                        \
                                           const CostConst<SX_MAX_M, NS, NU>&, const RolloutPtrs&, int, size_t, hipStream_t); \
    template int launch_rollout_rw<NS, NU>(const GpConst<NS, NS + NU>&, const ReachConst<NS, NU>&,                        \
                                           const CostConst<SX_MAX_M, NS, NU>&, const RolloutPtrs&, int, size_t, hipStream_t);
