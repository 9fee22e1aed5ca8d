// The exact-GP rollout entries: which form a model's rollout takes (plan_rollout over the streaming plan of
// sx_stream_launch.hpp), the launch in that form through the launchers of sx_rw_launch.hpp,
// sx_stream_launch.hpp and sx_big_launch.hpp (launch_rollout), the one host path of the entries that have the streaming
// kernel only (stream_rollout), the GP model table, and sx_cem_rollout[_elites][_junk], sx_cem_rollout[_elites]_multi,
// sx_cem_rollout_starts[_cons][_multi], sx_cem_rollout_gains, sx_cem_rollout_gains_form, sx_cem_rollout_starts_multi_form, sx_cem_rollout_form, sx_cem_rollout_multi_form, sx_cem_rollout_starts_form,
// sx_cem_rollout_workspace_bytes, and the entries with the saturating cost on the safety ellipsoids,
// sx_cem_rollout[_elites]_sat[_multi], sx_cem_rollout_sat_form, and those with the SafeMPC constraint set in the step,
// sx_cem_rollout[_elites]_cons[_multi], sx_cem_rollout_cons_form, sx_cem_rollout_cons_multi_form.  No kernel is compiled here.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/sx_amd.h"
#include "sx_big.hpp"   // big_ws_layout
#include "sx_big_launch.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_rw_launch.hpp"
#include "sx_stream_launch.hpp"

namespace sx {

#ifdef SX_STAMPS
extern unsigned long long* g_stamp_host;   // diagnostic build: the phase-stamp buffer (sx_debug_set_stamps, sx_rank.hip)
#endif

// The rollout form of a model, decided here only: sx_cem_rollout[_elites][_junk] launch it,
// sx_cem_rollout_form reports it, sx_cem_rollout_workspace_bytes sizes the workspace path by it.  No HIP call.
struct RolloutPlan {
    int form;     // SX_FORM_*
    bool ok;      // false: sx_cem_rollout answers SX_ERR_UNSUPPORTED
    size_t lds;   // dynamic LDS bytes of the form's kernel (not SX_FORM_BIG)
    int nrb;      // SX_FORM_RH / SX_FORM_RW: n_pad / 16, the kernel's instantiation
};

// SX_ROLLOUT=rh|rw|stream forces one form of the single-launch kernel (A/B runs); where it does not apply the rollout
// takes the streaming kernel, or answers SX_ERR_UNSUPPORTED with SX_ROLLOUT_STRICT set (so that a run knows what it timed).
struct FormOverride {
    int form;   // SX_FORM_RH / SX_FORM_RW / SX_FORM_STREAM, or -1: none
    bool strict;
    bool refuses() const { return strict && form >= 0; }
};
static const FormOverride& form_override() {
    static const FormOverride o = [] {
        const char* e = std::getenv("SX_ROLLOUT");
        const int form = !e                            ? -1
                         : std::strcmp(e, "stream") == 0 ? SX_FORM_STREAM
                         : std::strcmp(e, "rw") == 0     ? SX_FORM_RW
                         : std::strcmp(e, "rh") == 0     ? SX_FORM_RH
                                                         : -1;
        return FormOverride{form, std::getenv("SX_ROLLOUT_STRICT") != nullptr};
    }();
    return o;
}

template <int NS, int NU>
static int resident_lds_bytes(int n_train, int n_pad, int H, size_t* rh, size_t* rw) {
    *rh = rollout_rh_lds_bytes<NS, NU>(n_train, n_pad, H);
    *rw = rollout_rw_lds_bytes<NS, NU>(n_train, n_pad, H);
    return SX_OK;
}
// LDS bytes of the 8-wave and the 4-wave form for a plain rollout of a compiled shape (~0: that form has no instantiation)
static int resident_lds_bytes(int ns, int nu, int n_train, int n_pad, int H, size_t* rh, size_t* rw) {
#define CALL(NS, NU) resident_lds_bytes<NS, NU>(n_train, n_pad, H, rh, rw)
    SX_DISPATCH(ns, nu, CALL);
#undef CALL
}

// The refit prologue of the elite-row form keeps 2 H n_u doubles in the Kstar / mean-row buffers: at least 256 + 256 n_s
// of them
static bool elite_rows_fit(int ns, int nu, int H) { return 2 * H * nu <= 256 + 256 * ns; }

// `m` is the GP over ns + nu + sh columns (m->n_u = nu + sh), sh the query shift of sx_cem_rollout_junk.  The streaming
// answer is plan_stream's (sx_stream_launch.hpp); what is decided here is the workspace path, the elite-row bound, the
// override and the resident forms.
static RolloutPlan plan_rollout(const sx_gp_model* m, int sh, int H, bool elites) {
    const int ns = m->n_s, nu = m->n_u - sh, n_train = m->n_train, n_pad = m->n_pad;
    const StreamPlan s = plan_stream(ns, nu, sh, n_train, n_pad, H);
    bool ok = rollout_compiled(ns, nu, sh);
    // Kstar in HBM: plain rollouts only, without elite rows (the refit prologue belongs to the single-launch kernel)
    if (s.form < 0) return {SX_FORM_BIG, ok && sh == 0 && !elites, 0, 0};
    if (elites && !elite_rows_fit(ns, nu, H)) ok = false;
    if (s.form == SX_FORM_BYOUT) return {SX_FORM_BYOUT, ok, s.lds, 0};
    const RolloutPlan stream{SX_FORM_STREAM, ok, s.lds, 0};
    const FormOverride& o = form_override();
    if (!ok || sh > 0 || o.form == SX_FORM_STREAM) return stream;
    // W partly resident on 8 waves (n_s <= 2), then all of W in the registers of 4 waves (smaller N), then W streamed from
    // L2: the 4-wave form loses to the streaming kernel only where the 8-wave form exists (n_s = 2, n_u = 1: 126.6
    // against 125.7 us at config 2), and beats it by 7 - 16 % on the shapes the 8-wave form does not cover (n_s = 3, 4;
    // n_s = n_u = 2 beyond N = 128).
    size_t rh, rw;
    resident_lds_bytes(ns, nu, n_train, n_pad, H, &rh, &rw);
    if (o.form != SX_FORM_RW && rh <= kMaxLdsBytes) return {SX_FORM_RH, true, rh, n_pad >> 4};
    if (o.form != SX_FORM_RH && rw <= kMaxLdsBytes) return {SX_FORM_RW, true, rw, n_pad >> 4};
    return {SX_FORM_STREAM, !o.refuses(), stream.lds, 0};
}

// The rollout of a GP over NS + NU + SH columns (SH: the query shift of sx_cem_rollout_junk) in the form plan_rollout picks.
template <int NS, int NU, int SH>
static int launch_rollout(const sx_gp_model* m, const sx_env* env, const RolloutPtrs& rp, double* workspace,
                          int64_t workspace_bytes, hipStream_t stream) {
    RolloutPlan plan = plan_rollout(m, SH, rp.H, rp.elite_rows != nullptr);
    if (!plan.ok) return SX_ERR_UNSUPPORTED;
    if constexpr (SH == 0) {
        if (plan.form == SX_FORM_BIG) return launch_rollout_big<NS, NU>(m, env, rp, workspace, workspace_bytes, stream);
    }
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if (int r = env_consts<NS, NU>(env, rc, cc)) return r;
    RolloutPtrs rps = rp;
#ifdef SX_STAMPS
    rps.stamps = g_stamp_host;
#endif
    if constexpr (SH == 0) {
        if (plan.form == SX_FORM_RH || plan.form == SX_FORM_RW) {
            const int r = plan.form == SX_FORM_RH
                              ? launch_rollout_rh<NS, NU>(make_gp_const<NS, NU>(m, 8), rc, cc, rps, plan.nrb, plan.lds, stream)
                              : launch_rollout_rw<NS, NU>(make_gp_const<NS, NU>(m, kRwWaves), rc, cc, rps, plan.nrb, plan.lds,
                                                          stream);
            if (r != SX_ERR_UNSUPPORTED || form_override().refuses()) return r;
            plan = {SX_FORM_STREAM, true, rollout_stream_lds_bytes(NS, NU, SH, m->n_train, m->n_pad, rp.H, false), 0};
        }
    }
    return launch_stream<StreamPlain<SH>, NS, NU>(make_gp_const<NS, NU + SH>(m, kRolloutThreads / 64), rc, cc, rps, nullptr,
                                                  plan.form == SX_FORM_BYOUT, plan.lds, stream);
}

// The entries that have the streaming kernel only -- the multi-model rollouts, the per-particle starts, the saturating
// cost on the safety ellipsoids -- from their checked arguments to the launch of variant V, for one model or (V::MM) rp.E
// of them behind their device `table`: the streaming plan with the elite-row bound (no workspace path, no resident form,
// no override), the constants of `env`, those of `cost` (V::SAT) and of `cons` (V::CONS), the device `gains` (V::KF), the GP
// argument, the launcher.
template <class V, int NS, int NU>
static int stream_rollout(const sx_gp_model* models, const void* table, const sx_env* env, const sx_sat_cost* cost,
                          const sx_con_set* cons, const double* gains, const RolloutPtrs& rp, hipStream_t stream) {
    const StreamPlan plan = plan_stream_multi(models, V::MM ? rp.E : 1, rp.H);
    if (plan.form < 0 || (rp.elite_rows && !elite_rows_fit(NS, NU, rp.H))) return SX_ERR_UNSUPPORTED;
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if constexpr (V::KF) {
        // env->k_fb is not read: the constants are those of a zero gain, and no lane of the variant reads rc.kfb / rc.cholB
        sx_env no_gain = *env;
        for (double& k : no_gain.k_fb) k = 0.0;
        if (int r = env_consts<NS, NU>(&no_gain, rc, cc)) return r;
    } else {
        if (int r = env_consts<NS, NU>(env, rc, cc)) return r;
    }
    SatConst<NS> sat;
    if constexpr (V::SAT) make_sat_const<NS>(cost, sat);
    const SatConst<NS>* satp = V::SAT ? &sat : nullptr;
    ConConst<NS> con;
    if constexpr (V::CONS) make_con_const<NS>(cons, con);
    const ConConst<NS>* conp = V::CONS ? &con : nullptr;
    const GainConst kf{gains};
    const GainConst* kfp = V::KF ? &kf : nullptr;
    const bool byout = plan.form == SX_FORM_BYOUT;
    if constexpr (V::MM)
        return launch_stream<V, NS, NU>(static_cast<const GpConst<NS, NS + NU>*>(table), rc, cc, rp, satp, byout, plan.lds,
                                        stream, conp, kfp);
    else
        return launch_stream<V, NS, NU>(make_gp_const<NS, NU>(models, kRolloutThreads / 64), rc, cc, rp, satp, byout,
                                        plan.lds, stream, conp, kfp);
}

template <class V>
static int stream_dispatch(const sx_gp_model* models, const void* table, const sx_env* env, const sx_sat_cost* cost,
                           const RolloutPtrs& rp, void* stream, const sx_con_set* cons = nullptr,
                           const double* gains = nullptr) {
#define CALL(NS, NU) stream_rollout<V, NS, NU>(models, table, env, cost, cons, gains, rp, (hipStream_t)stream)
    SX_DISPATCH(env->n_s, env->n_u, CALL);
#undef CALL
}

// Bytes of one sx_gp_model_table entry: the GpConst the streaming kernel takes (SX_ERR_UNSUPPORTED for a shape without
// a rollout kernel)
template <int NS, int NU>
static int64_t gp_table_entry_bytes() {
    return (int64_t)sizeof(GpConst<NS, NS + NU>);
}
static int64_t gp_table_entry_bytes(int ns, int nu) {
#define CALL(NS, NU) gp_table_entry_bytes<NS, NU>()
    SX_DISPATCH(ns, nu, CALL);
#undef CALL
}

template <int NS, int NU>
static int build_gp_table(const sx_gp_model* models, int E, void* table, hipStream_t stream) {
    std::vector<GpConst<NS, NS + NU>> host(E);
    for (int i = 0; i < E; ++i) host[i] = make_gp_const<NS, NU>(&models[i], kRolloutThreads / 64);
    return copy_model_table(host, table, stream);
}

// The elite-row form of a rollout's actions: the refit prologue derives the sampling distribution from k sorted elite
// rows and, where mean_out and std_out are given, writes it out
static RolloutPtrs with_elites(RolloutPtrs rp, const double* elite_rows, int k, double* mean_out, double* std_out) {
    rp.elite_rows = elite_rows;
    rp.elite_k = k;
    rp.mean_out = mean_out;
    rp.std_out = std_out;
    return rp;
}

// The objective of a safety rollout: env's own, or (`sat`) the saturating cost `cost` on the safety ellipsoids (DESIGN.md
// section 3.13; env->obj_mode is then not read), which has the streaming kernel only
struct Objective {
    bool sat;
    const sx_sat_cost* cost;
};
constexpr Objective kEnvObjective{false, nullptr};

// (model, env, query_shift) of the rollout entries: checked before anything touches the device
static bool rollout_shapes_ok(const sx_gp_model* model, const sx_env* env, int query_shift) {
    return model->n_s == env->n_s && query_shift >= 0 && query_shift <= env->n_u && model->n_u == env->n_u + query_shift;
}

// E models of one (n_s, n_u) with a training set each: checked before anything touches the device
static bool multi_models_ok(const sx_gp_model* models, int E) {
    if (!models || E <= 0) return false;
    const int ns = models[0].n_s, nu = models[0].n_u;
    if (ns <= 0 || ns > SX_MAX_NS || nu <= 0 || nu > SX_MAX_NU) return false;
    for (int i = 0; i < E; ++i)
        if (models[i].n_s != ns || models[i].n_u != nu || models[i].n_train <= 0 || models[i].n_pad <= 0) return false;
    return true;
}

// The entries over one model, behind their RolloutPtrs (`elites`: with_elites'): the argument checks, the cost's after
// them, then the launch -- launch_rollout's full plan, or the streaming kernel priced by the cost.
static int cem_rollout_single(const sx_gp_model* model, const sx_env* env, int query_shift, Objective obj, bool elites,
                              const RolloutPtrs& rp, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!model || (elites && !rp.elite_rows) || !rollout_args_ok(env, rp) || !rollout_shapes_ok(model, env, query_shift))
        return SX_ERR_ARG;
    if (obj.sat) {
        if (!sat_cost_ok(obj.cost, env->n_s)) return SX_ERR_ARG;
        return stream_dispatch<StreamSat<false>>(model, nullptr, env, obj.cost, rp, stream);
    }
#define CALL(NS, NU, SH) launch_rollout<NS, NU, SH>(model, env, rp, (double*)workspace, workspace_bytes, (hipStream_t)stream)
    SX_ROLLOUT_DISPATCH(env->n_s, env->n_u, query_shift, CALL);
#undef CALL
}

// sx_cem_rollout[_elites]_cons: cem_rollout_single's checks, the set's and the cost's after them, then the streaming kernel
// with the set in its step, priced by env's objective (cost == NULL) or by the cost
static int cem_rollout_cons(const sx_gp_model* model, const sx_env* env, const sx_con_set* cons, const sx_sat_cost* cost,
                            bool elites, const RolloutPtrs& rp, void* stream) {
    if (!model || (elites && !rp.elite_rows) || !rollout_args_ok(env, rp) || !rollout_shapes_ok(model, env, 0))
        return SX_ERR_ARG;
    if (!con_set_ok(cons, env->n_s) || (cost && !sat_cost_ok(cost, env->n_s))) return SX_ERR_ARG;
    if (cost) return stream_dispatch<StreamCons<true>>(model, nullptr, env, cost, rp, stream, cons);
    return stream_dispatch<StreamCons<false>>(model, nullptr, env, nullptr, rp, stream, cons);
}

// sx_cem_rollout[_elites]_cons_multi: cem_rollout_multi's checks, the set's and the cost's after them, then the multi-model
// streaming kernel with the ONE set of all problems in its step
static int cem_rollout_cons_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_con_set* cons,
                                  const sx_sat_cost* cost, bool elites, const RolloutPtrs& rp, void* stream) {
    if (!table || (elites && !rp.elite_rows) || !rollout_args_ok(env, rp) || !multi_models_ok(models, rp.E)) return SX_ERR_ARG;
    if (models[0].n_s != env->n_s || models[0].n_u != env->n_u) return SX_ERR_ARG;
    if (!con_set_ok(cons, env->n_s) || (cost && !sat_cost_ok(cost, env->n_s))) return SX_ERR_ARG;
    if (cost) return stream_dispatch<StreamCons<true, true>>(models, table, env, cost, rp, stream, cons);
    return stream_dispatch<StreamCons<false, true>>(models, table, env, nullptr, rp, stream, cons);
}

// The entries over rp.E models behind their device `table`, as cem_rollout_single: every one has the streaming kernel only
static int cem_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env, Objective obj, bool elites,
                             const RolloutPtrs& rp, void* stream) {
    if (!table || (elites && !rp.elite_rows) || !rollout_args_ok(env, rp) || !multi_models_ok(models, rp.E)) return SX_ERR_ARG;
    if (models[0].n_s != env->n_s || models[0].n_u != env->n_u) return SX_ERR_ARG;
    if (!obj.sat) return stream_dispatch<StreamPlain<0, true>>(models, table, env, nullptr, rp, stream);
    if (!sat_cost_ok(obj.cost, env->n_s)) return SX_ERR_ARG;
    return stream_dispatch<StreamSat<true>>(models, table, env, obj.cost, rp, stream);
}

// What the form queries of the stream-only entries answer: the form of the launch, -1 where there is none
static int stream_form(const sx_gp_model* models, int E, int H) {
    return models && H > 0 ? plan_stream_multi(models, E, H).form : -1;
}

}  // namespace sx

extern "C" {

int64_t sx_cem_rollout_workspace_bytes(const sx_gp_model* model, int E, int P, int H) {
    if (!model || E <= 0 || P <= 0 || H <= 0) return -1;
    if (sx::plan_rollout(model, 0, H, false).form != SX_FORM_BIG) return 0;
    return sx::big_ws_layout(nullptr, model->n_s, model->n_s + model->n_u, model->n_pad, (int64_t)E * P).total *
           (int64_t)sizeof(double);
}

int sx_cem_rollout_form(const sx_gp_model* model, int H) {
    if (!model || H <= 0) return -1;
    const sx::RolloutPlan plan = sx::plan_rollout(model, 0, H, false);
    return plan.ok ? plan.form : -1;
}

int sx_cem_rollout(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                   const double* mean, const double* std, const double* noise, double* actions, double* traj,
                   double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* workspace,
                   int64_t workspace_bytes, void* stream) {
    return sx_cem_rollout_junk(model, env, 0, E, P, H, x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost,
                               status, workspace, workspace_bytes, stream);
}

int sx_cem_rollout_elites(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                          const double* elite_rows, int k, const double* noise, double* actions, double* traj, double* sigma,
                          double* obj_cost, double* con_cost, int32_t* status, double* mean_out, double* std_out, void* stream) {
    return sx_cem_rollout_elites_junk(model, env, 0, E, P, H, x0, q0, elite_rows, k, noise, actions, traj, sigma, obj_cost,
                                      con_cost, status, mean_out, std_out, stream);
}

int sx_cem_rollout_junk(const sx_gp_model* model, const sx_env* env, int query_shift, int E, int P, int H, const double* x0,
                        const double* q0, const double* mean, const double* std, const double* noise, double* actions,
                        double* traj, double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    const sx::RolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::cem_rollout_single(model, env, query_shift, sx::kEnvObjective, false, rp, workspace, workspace_bytes, stream);
}

int sx_cem_rollout_elites_junk(const sx_gp_model* model, const sx_env* env, int query_shift, int E, int P, int H,
                               const double* x0, const double* q0, const double* elite_rows, int k, const double* noise,
                               double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                               int32_t* status, double* mean_out, double* std_out, void* stream) {
    const sx::RolloutPtrs rp = sx::with_elites({x0, q0, nullptr, nullptr, noise, actions, traj, sigma, obj_cost, con_cost,
                                                status, E, P, H}, elite_rows, k, mean_out, std_out);
    return sx::cem_rollout_single(model, env, query_shift, sx::kEnvObjective, true, rp, nullptr, 0, stream);
}

int sx_cem_rollout_starts_form(const sx_gp_model* model, int H) { return sx::stream_form(model, 1, H); }

// sx_cem_rollout_starts[_cons][_multi]'s own argument checks (before anything touches the device), over the `n_models`
// models behind `model`: 1, or with the multi-model entries one per problem (E of them, as multi_models_ok reads them)
static bool starts_args_ok(const sx_gp_model* model, int n_models, const sx_env* env, int E, int P, int H,
                           const double* mean, const double* std, const double* noise, const double* rows,
                           const double* obj_cost, const double* con_cost, const int32_t* status) {
    if (!model || !env || !rows || !obj_cost || !con_cost || !status || E <= 0 || P <= 0 || H <= 0) return false;
    if (noise && !(mean && std)) return false;
    for (int i = 0; i < n_models; ++i)
        if (model[i].n_s != env->n_s || model[i].n_u != env->n_u || model[i].n_train <= 0 || model[i].n_pad <= 0) return false;
    return true;
}

int sx_cem_rollout_starts(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* mean,
                          const double* std, const double* noise, double* rows, double* traj, double* sigma,
                          double* obj_cost, double* con_cost, int32_t* status, void* stream) {
    if (!starts_args_ok(model, 1, env, E, P, H, mean, std, noise, rows, obj_cost, con_cost, status)) return SX_ERR_ARG;
    // (x0, q0 and the elite-row fields stay empty: the kernel reads the start of a particle from its row)
    const sx::RolloutPtrs rp{nullptr, nullptr, mean, std, noise, rows, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::stream_dispatch<sx::StreamStarts>(model, nullptr, env, nullptr, rp, stream);
}

int sx_cem_rollout_starts_cons(const sx_gp_model* model, const sx_env* env, const sx_con_set* cons, int E, int P, int H,
                               const double* mean, const double* std, const double* noise, double* rows, double* traj,
                               double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream) {
    if (!starts_args_ok(model, 1, env, E, P, H, mean, std, noise, rows, obj_cost, con_cost, status)) return SX_ERR_ARG;
    if (!sx::con_set_ok(cons, env->n_s)) return SX_ERR_ARG;
    const sx::RolloutPtrs rp{nullptr, nullptr, mean, std, noise, rows, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::stream_dispatch<sx::StreamStartsCons>(model, nullptr, env, nullptr, rp, stream, cons);
}

int sx_cem_rollout_gains_form(const sx_gp_model* model, int H) { return sx::stream_form(model, 1, H); }

int sx_cem_rollout_gains(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* mean,
                         const double* std, const double* noise, double* rows, const double* gains, double* traj,
                         double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream) {
    if (!starts_args_ok(model, 1, env, E, P, H, mean, std, noise, rows, obj_cost, con_cost, status)) return SX_ERR_ARG;
    if (H > 1 && !gains) return SX_ERR_ARG;   // (step 0 starts from a point and reads none)
    const sx::RolloutPtrs rp{nullptr, nullptr, mean, std, noise, rows, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::stream_dispatch<sx::StreamGains>(model, nullptr, env, nullptr, rp, stream, nullptr, gains);
}

int sx_cem_rollout_starts_multi_form(const sx_gp_model* models, int E, int H) {
    return sx::multi_models_ok(models, E) ? sx::stream_form(models, E, H) : -1;
}

// (problem e rolls out under models[e] and entry e of `table`; a scenario with R restarts stands R times in both)
int sx_cem_rollout_starts_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                                const double* mean, const double* std, const double* noise, double* rows, double* traj,
                                double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream) {
    if (!starts_args_ok(models, E, env, E, P, H, mean, std, noise, rows, obj_cost, con_cost, status) || !table)
        return SX_ERR_ARG;
    const sx::RolloutPtrs rp{nullptr, nullptr, mean, std, noise, rows, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::stream_dispatch<sx::StreamStartsMulti>(models, table, env, nullptr, rp, stream);
}

int sx_cem_rollout_starts_cons_multi(const sx_gp_model* models, const void* table, const sx_env* env,
                                     const sx_con_set* cons, int E, int P, int H, const double* mean, const double* std,
                                     const double* noise, double* rows, double* traj, double* sigma, double* obj_cost,
                                     double* con_cost, int32_t* status, void* stream) {
    if (!starts_args_ok(models, E, env, E, P, H, mean, std, noise, rows, obj_cost, con_cost, status) || !table)
        return SX_ERR_ARG;
    if (!sx::con_set_ok(cons, env->n_s)) return SX_ERR_ARG;
    const sx::RolloutPtrs rp{nullptr, nullptr, mean, std, noise, rows, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::stream_dispatch<sx::StreamStartsConsMulti>(models, table, env, nullptr, rp, stream, cons);
}

int64_t sx_gp_model_table_bytes(int n_s, int n_u, int E) {
    if (E <= 0 || n_s <= 0 || n_s > SX_MAX_NS || n_u <= 0 || n_u > SX_MAX_NU) return -1;
    const int64_t entry = sx::gp_table_entry_bytes(n_s, n_u);
    return entry == SX_ERR_UNSUPPORTED ? -1 : entry * E;
}

int sx_gp_model_table(const sx_gp_model* models, int E, void* table, void* stream) {
    if (!table || !sx::multi_models_ok(models, E)) return SX_ERR_ARG;
    for (int i = 0; i < E; ++i)
        if (!models[i].x_train || !models[i].a_pack || !models[i].stage_tab) return SX_ERR_ARG;
#define CALL(NS, NU) sx::build_gp_table<NS, NU>(models, E, table, (hipStream_t)stream)
    SX_DISPATCH(models[0].n_s, models[0].n_u, CALL);
#undef CALL
}

int sx_cem_rollout_multi_form(const sx_gp_model* models, int E, int H) {
    return sx::multi_models_ok(models, E) ? sx::stream_form(models, E, H) : -1;
}

int sx_cem_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                         const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                         double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost, int32_t* status,
                         void* stream) {
    const sx::RolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::cem_rollout_multi(models, table, env, sx::kEnvObjective, false, rp, stream);
}

int sx_cem_rollout_elites_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                                const double* x0, const double* q0, const double* elite_rows, int k, const double* noise,
                                double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                                int32_t* status, double* mean_out, double* std_out, void* stream) {
    const sx::RolloutPtrs rp = sx::with_elites({x0, q0, nullptr, nullptr, noise, actions, traj, sigma, obj_cost, con_cost,
                                                status, E, P, H}, elite_rows, k, mean_out, std_out);
    return sx::cem_rollout_multi(models, table, env, sx::kEnvObjective, true, rp, stream);
}

// ---- the saturating cost on the safety ellipsoids: the entries above with a cost handed in ----------
int sx_cem_rollout_sat_form(const sx_gp_model* model, int H) { return sx::stream_form(model, 1, H); }

int sx_cem_rollout_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E, int P, int H,
                       const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                       double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost, int32_t* status,
                       void* stream) {
    const sx::RolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::cem_rollout_single(model, env, 0, {true, cost}, false, rp, nullptr, 0, stream);
}

int sx_cem_rollout_elites_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E, int P, int H,
                              const double* x0, const double* q0, const double* elite_rows, int k, const double* noise,
                              double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                              int32_t* status, double* mean_out, double* std_out, void* stream) {
    const sx::RolloutPtrs rp = sx::with_elites({x0, q0, nullptr, nullptr, noise, actions, traj, sigma, obj_cost, con_cost,
                                                status, E, P, H}, elite_rows, k, mean_out, std_out);
    return sx::cem_rollout_single(model, env, 0, {true, cost}, true, rp, nullptr, 0, stream);
}

int sx_cem_rollout_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_sat_cost* cost, int E,
                             int P, int H, const double* x0, const double* q0, const double* mean, const double* std,
                             const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                             double* con_cost, int32_t* status, void* stream) {
    const sx::RolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::cem_rollout_multi(models, table, env, {true, cost}, false, rp, stream);
}

int sx_cem_rollout_elites_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_sat_cost* cost,
                                    int E, int P, int H, const double* x0, const double* q0, const double* elite_rows, int k,
                                    const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                                    double* con_cost, int32_t* status, double* mean_out, double* std_out, void* stream) {
    const sx::RolloutPtrs rp = sx::with_elites({x0, q0, nullptr, nullptr, noise, actions, traj, sigma, obj_cost, con_cost,
                                                status, E, P, H}, elite_rows, k, mean_out, std_out);
    return sx::cem_rollout_multi(models, table, env, {true, cost}, true, rp, stream);
}

// ---- the SafeMPC constraint set in the step: the entries with a set handed in ---------------------------
int sx_cem_rollout_cons_form(const sx_gp_model* model, int H) { return sx::stream_form(model, 1, H); }

int sx_cem_rollout_cons(const sx_gp_model* model, const sx_env* env, const sx_con_set* cons, const sx_sat_cost* cost, int E,
                        int P, int H, const double* x0, const double* q0, const double* mean, const double* std,
                        const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                        double* con_cost, int32_t* status, void* stream) {
    const sx::RolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::cem_rollout_cons(model, env, cons, cost, false, rp, stream);
}

int sx_cem_rollout_elites_cons(const sx_gp_model* model, const sx_env* env, const sx_con_set* cons, const sx_sat_cost* cost,
                               int E, int P, int H, const double* x0, const double* q0, const double* elite_rows, int k,
                               const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                               double* con_cost, int32_t* status, double* mean_out, double* std_out, void* stream) {
    const sx::RolloutPtrs rp = sx::with_elites({x0, q0, nullptr, nullptr, noise, actions, traj, sigma, obj_cost, con_cost,
                                                status, E, P, H}, elite_rows, k, mean_out, std_out);
    return sx::cem_rollout_cons(model, env, cons, cost, true, rp, stream);
}

// the multi-model entries with the set handed in: one set for all problems, a GP each
int sx_cem_rollout_cons_multi_form(const sx_gp_model* models, int E, int H) {
    return sx::multi_models_ok(models, E) ? sx::stream_form(models, E, H) : -1;
}

int sx_cem_rollout_cons_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_con_set* cons,
                              const sx_sat_cost* cost, int E, int P, int H, const double* x0, const double* q0,
                              const double* mean, const double* std, const double* noise, double* actions, double* traj,
                              double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream) {
    const sx::RolloutPtrs rp{x0, q0, mean, std, noise, actions, traj, sigma, obj_cost, con_cost, status, E, P, H};
    return sx::cem_rollout_cons_multi(models, table, env, cons, cost, false, rp, stream);
}

int sx_cem_rollout_elites_cons_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_con_set* cons,
                                     const sx_sat_cost* cost, int E, int P, int H, const double* x0, const double* q0,
                                     const double* elite_rows, int k, const double* noise, double* actions, double* traj,
                                     double* sigma, double* obj_cost, double* con_cost, int32_t* status, double* mean_out,
                                     double* std_out, void* stream) {
    const sx::RolloutPtrs rp = sx::with_elites({x0, q0, nullptr, nullptr, noise, actions, traj, sigma, obj_cost, con_cost,
                                                status, E, P, H}, elite_rows, k, mean_out, std_out);
    return sx::cem_rollout_cons_multi(models, table, env, cons, cost, true, rp, stream);
}

}  // extern "C"
