// Host side of the Taylor performance rollouts, shared by sx_perf_taylor.hip (the parent entries) and
// sx_perf_taylor_sat.hip (the entries with the saturating cost): the form for perf_gp_rollout and what the entries do
// behind check_perf_entry.  The cautious form (sx_cautious_host.hpp) fills its Taylor constants through
// PerfTaylorForm::make_const too.  Host code only.
#pragma once
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // SX_ROLLOUT_SHAPES, SX_DISPATCH
#include "sx_perf_launch.hpp"
#include "sx_perf_taylor.hpp"

namespace sx {

// The Taylor form for perf_gp_rollout (sx_perf_launch.hpp): the variance form's plan with the step constants behind the
// tile's actions
struct PerfTaylorForm {
    template <int NS, int NU>
    using Const = PerfTaylorConst<NS, NU>;
    using Ptrs = PerfTaylorPtrs;
    static const PerfPtrs& base(const Ptrs& tp) { return tp.p; }
    static size_t extra_bytes(int ns, int nu) { return perf_taylor_extra_bytes(ns, nu); }
    template <int NS, int NU>
    static void make_const(const sx_env* env, Const<NS, NU>& tc) {
        static_assert(sizeof(PerfTaylorConst<NS, NU>) ==
                          (2 * NS * NS + 2 * NS * NU + 2 * NU + 3 * NS + SX_MAX_M * NS + SX_MAX_M) * sizeof(double),
                      "perf_taylor_extra_bytes counts the fields of PerfTaylorConst");
        make_perf_step<NS, NU>(env, tc.step);
        for (int i = 0; i < NS; ++i)
            for (int j = 0; j < NS; ++j) {
                double s = env->a[i * NS + j];
                for (int c = 0; c < NU; ++c) s += env->b[i * NU + c] * env->k_fb[c * NS + j];
                tc.abk[i * NS + j] = s;
            }
        for (int i = 0; i < NU * NS; ++i) tc.k_fb[i] = env->k_fb[i];
        for (int i = 0; i < env->m * NS; ++i) tc.h_mat[i] = env->h_mat[i];
        for (int i = 0; i < env->m; ++i) tc.h_vec[i] = env->h_vec[i];
    }
    template <int NS, int NU, bool BYOUT>
    static auto kernel() {
        return cem_perf_gp_rollout_kernel<PerfTaylorKind<false>, NS, NU, BYOUT, false, const int4* __restrict__>;
    }
};

// What the Taylor entries do behind check_perf_entry: terminal_safety, then the polytope rows, then the launch of form F
// (PerfTaylorForm | PerfTaylorSatForm, sx_perf_taylor_sat.hip)
template <class F = PerfTaylorForm>
int perf_taylor_launch(const sx_gp_model* models, const void* table, const sx_env* env, const PerfPtrs& pp,
                              double* perf_sigma, double* perf_cov, int terminal_safety, void* stream) {
    if (terminal_safety && (pp.n_perf < pp.H + 2 || env->m <= 0)) return SX_ERR_ARG;
    if (env->m < 0) return SX_ERR_ARG;
    if (env->m > SX_MAX_M) return SX_ERR_UNSUPPORTED;
    const PerfTaylorPtrs tp{{pp, perf_sigma, env->obj_mode}, perf_cov, env->m, terminal_safety ? pp.H + 1 : -1};
    return perf_gp_dispatch<F>(models, table, env, tp, (hipStream_t)stream);
}

}  // namespace sx
