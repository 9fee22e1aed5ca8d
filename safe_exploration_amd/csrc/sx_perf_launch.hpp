// Host side of the performance rollouts, shared by their five translation units: the argument checks of the six rollout
// entries, the form of a GP-product rollout (variance | Taylor; the streaming plan of sx_stream_launch.hpp over their LDS
// -- the entries launch it, the four _form queries report it), the one path from plan to launch of those two forms, and the launchers of their multi-model kernels,
// whose instantiations are compiled in sx_perf_multi.hip and sx_perf_taylor_multi.hip.  Host code only.
#pragma once
#include <climits>
#include <cstring>

#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_stream_launch.hpp"   // plan_stream_multi, SX_DISPATCH
#include "sx_perf_var.hpp"

namespace sx {

static_assert(kPerfVarThreads == kRolloutThreads, "the stage table of sx_gp_pack is cut for the safety kernel's waves");

inline PerfPtrs make_perf_ptrs(const double* x0, const double* safe_actions, const double* tail_mean,
                               const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                               double* con_cost, double* perf_traj, int32_t* status, int E, int P, int H, int n_perf, int r) {
    return {x0, safe_actions, tail_mean, tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj, status,
            E, P, H, n_perf, r};
}

inline bool perf_model_has_data(const sx_gp_model& m) { return m.x_train && m.n_train > 0; }

// The packed model of sx_gp_pack: W fragments, the stage table, and the padding that holds the mean / Jacobian rows
inline bool perf_var_model_ok(const sx_gp_model& m) {
    if (!perf_model_has_data(m) || !m.a_pack || !m.stage_tab) return false;
    return m.n_pad % 16 == 0 && m.n_pad > m.n_train + m.n_s + m.n_u;
}

// (n_s, n_u) within the arrays of sx_gp_model / sx_env
inline bool perf_shape_ok(const sx_gp_model& m) {
    return m.n_s > 0 && m.n_s <= SX_MAX_NS && m.n_u > 0 && m.n_u <= SX_MAX_NU;
}

// n models of one (n_s, n_u), `model_ok` (perf_model_has_data | perf_var_model_ok) each
inline bool perf_models_ok(const sx_gp_model* models, int n, bool (*model_ok)(const sx_gp_model&)) {
    if (!models || n <= 0) return false;
    for (int i = 0; i < n; ++i)
        if (models[i].n_s != models[0].n_s || models[i].n_u != models[0].n_u || !model_ok(models[i])) return false;
    return true;
}

// What the six rollout entries check alike before anything touches the device, in the order they answer: pointers (`head`:
// the entry's own leading ones are all there), sizes, the drawn tail, the `n` models (`bounded`: perf_shape_ok too -- the
// single-model mean-only and variance entries leave a shape past SX_MAX_NS / SX_MAX_NU to the dispatch) against env, and
// the objective: a mean-only entry (`variance` false) answers SX_ERR_UNSUPPORTED for SX_OBJ_NEG_VARIANCE.
inline int check_perf_entry(bool head, const sx_gp_model* models, int n, bool bounded, bool (*model_ok)(const sx_gp_model&),
                            const sx_env* env, const PerfPtrs& pp, bool variance) {
    if (!head || !models || !env || !pp.x0 || !pp.safe_actions || !pp.rows || !pp.obj_cost || !pp.con_cost || !pp.status)
        return SX_ERR_ARG;
    if (pp.E <= 0 || pp.P <= 0 || pp.H <= 0 || pp.r < 1 || pp.r > pp.H || pp.n_perf <= pp.r) return SX_ERR_ARG;
    if (pp.tail_noise && (!pp.tail_mean || !pp.tail_std)) return SX_ERR_ARG;
    if ((bounded && !perf_shape_ok(models[0])) || !perf_models_ok(models, n, model_ok)) return SX_ERR_ARG;
    if (models[0].n_s != env->n_s || models[0].n_u != env->n_u) return SX_ERR_ARG;
    if (env->obj_mode == SX_OBJ_NEG_VARIANCE) return variance ? SX_OK : SX_ERR_UNSUPPORTED;
    return env->obj_mode == SX_OBJ_AFFINE_ABS ? SX_OK : SX_ERR_ARG;
}

// bytes of the step constants (PerfTaylorConst, sx_perf_taylor.hpp) the Taylor kernels keep in LDS behind the tile's actions
inline size_t perf_taylor_extra_bytes(int ns, int nu) {
    return ((size_t)2 * ns * ns + 2 * ns * nu + 2 * nu + 3 * ns + (size_t)SX_MAX_M * ns + SX_MAX_M) * sizeof(double);
}

// What the four _form queries answer for `n` models: the form of the launch by the streaming plan the safety kernel takes
// (plan_stream_multi, sx_stream_launch.hpp: n_perf actions in the tile, the Taylor form's step constants behind them;
// there is no resident-W form and no workspace path here), -1 where an entry would refuse the models or has no form for them.
inline int perf_gp_form(const sx_gp_model* models, int n, int n_perf, bool taylor) {
    if (n_perf <= 1 || !perf_models_ok(models, n, perf_var_model_ok) || !perf_shape_ok(models[0])) return -1;
    const size_t extra = taylor ? perf_taylor_extra_bytes(models[0].n_s, models[0].n_u) : 0;
    return plan_stream_multi(models, n, n_perf, extra).form;
}

// One launch of a GP-product kernel with `lds` bytes: `args` are the kernel's own
template <class Kernel, class... Args>
int launch_perf_gp(Kernel kernel, unsigned blocks, size_t lds, hipStream_t stream, const Args&... args) {
    if (int r = allow_lds(kernel, lds)) return r;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kPerfVarThreads), lds, stream, args...);
    return check_launch();
}

// The multi-model kernel of kind K (PerfVarKind | PerfTaylorKind<SAT>); one output has no output-by-output kernel.
template <class K, int NS, int NU, class... Args>
int launch_perf_gp_forms(bool byout, unsigned blocks, size_t lds, hipStream_t stream, const Args&... args) {
    if constexpr (NS > 1) {
        if (byout) return launch_perf_gp(cem_perf_gp_rollout_kernel<K, NS, NU, true, true>, blocks, lds, stream, args...);
    }
    return launch_perf_gp(cem_perf_gp_rollout_kernel<K, NS, NU, false, true>, blocks, lds, stream, args...);
}

// The launchers of the multi-model kernels over `table` (sx_gp_model_table's; the status holds a word per problem),
// instantiated for every shape beside the kernels: launch_perf_gp_forms over cem_perf_gp_rollout_kernel<..., MM = true> of
// kind PerfVarKind (sx_perf_multi.hip) and of kind PerfTaylorKind<false> (sx_perf_taylor_multi.hip)
template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const PerfStepConst<NS, NU>& sc, const PerfVarPtrs& vp,
                         bool byout, unsigned blocks, size_t lds, hipStream_t stream);
template <int NS, int NU>
struct PerfTaylorConst;
struct PerfTaylorPtrs;
template <int NS, int NU>
int launch_perf_gp_multi(const GpConst<NS, NS + NU>* table, const PerfTaylorConst<NS, NU>& tc, const PerfTaylorPtrs& tp,
                         bool byout, unsigned blocks, size_t lds, hipStream_t stream);

// The path of both GP-product forms from the checked arguments to the launch, for one model (`table` NULL) or pp.E of them
// behind their device table: plan, blocks, step constants, then the kernel of the form the plan picked.  `F` names the form:
//     F::Const<NS, NU>, F::make_const<NS, NU>(env, c)   the step constants and how sx_env fills them
//     F::Ptrs, F::base(ptrs)                            the kernel's pointers and the PerfPtrs in them
//     F::extra_bytes(ns, nu)                            what the kernel keeps in LDS behind the actions
//     F::kernel<NS, NU, BYOUT>()                        the single-model kernel
template <class F, int NS, int NU>
int perf_gp_rollout(const sx_gp_model* models, const void* table, const sx_env* env, const typename F::Ptrs& ptrs,
                    hipStream_t stream) {
    const PerfPtrs& pp = F::base(ptrs);
    const StreamPlan plan = plan_stream_multi(models, table ? pp.E : 1, pp.n_perf, F::extra_bytes(NS, NU));
    const int64_t blocks = (int64_t)pp.E * ((pp.P + SX_TILE - 1) / SX_TILE);
    if (plan.form < 0 || blocks > INT_MAX) return SX_ERR_UNSUPPORTED;
    typename F::template Const<NS, NU> c;
    std::memset(&c, 0, sizeof(c));
    F::template make_const<NS, NU>(env, c);
    const bool byout = plan.form == SX_FORM_BYOUT;
    if (table)
        return launch_perf_gp_multi<NS, NU>(static_cast<const GpConst<NS, NS + NU>*>(table), c, ptrs, byout,
                                            (unsigned)blocks, plan.lds, stream);
    const GpConst<NS, NS + NU> gc = make_gp_const<NS, NU>(models, kPerfVarThreads / 64);
    const auto kernel = byout ? F::template kernel<NS, NU, true>() : F::template kernel<NS, NU, false>();
    return launch_perf_gp(kernel, (unsigned)blocks, plan.lds, stream, gc, gc.stage_tab, c, ptrs);
}

template <class F>
int perf_gp_dispatch(const sx_gp_model* models, const void* table, const sx_env* env, const typename F::Ptrs& ptrs,
                     hipStream_t stream) {
#define CALL(NS, NU) perf_gp_rollout<F, NS, NU>(models, table, env, ptrs, stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

}  // namespace sx
