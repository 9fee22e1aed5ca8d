// The fused CEM particle rollout kernel (sx_cem_rollout, training sets that fit the LDS budget).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_reach.hpp"
#include "sx_refit.hpp"
#include "sx_conset.hpp"     // ConConst, ctrl_ellipsoid_violated
#include "sx_sat_cost.hpp"   // SatConst, sat_loss

namespace sx {

#ifndef SX_ROLLOUT_THREADS
#define SX_ROLLOUT_THREADS (64 * SX_WAVES)
#endif
constexpr int kRolloutThreads = SX_ROLLOUT_THREADS;  // waves of the CU that owns the 16-particle tile

// ---------------------------------------------------------------------------------------------------------------
// sx_cem_rollout: the fused H-step particle rollout.  One workgroup = 16 particles of one problem for all H steps.
// ---------------------------------------------------------------------------------------------------------------
#ifdef SX_STAMPS
// Diagnostic build only (tools/phase_stamps.py): per-workgroup cycle sums of the three phases of a step.
static __device__ unsigned long long* g_stamp_buf = nullptr;   // (one per translation unit)
__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#endif

struct RolloutPtrs {
    const double* x0;
    const double* q0;
    const double* mean;
    const double* std;
    const double* noise;
    double* actions;
    double* traj;
    double* sigma;
    double* obj_cost;
    double* con_cost;
    int* status;
    int E, P, H;
    // sx_cem_rollout_elites: the sampling distribution is refit from the previous iteration's elite rows
    // [E x elite_k x (2 + H n_u)] in the kernel's prologue (mean / std above are then unused)
    const double* elite_rows = nullptr;
    int elite_k = 0;
    double* mean_out = nullptr;   // [E x H n_u] the refit, written by the first workgroup of each problem (may be null)
    double* std_out = nullptr;
#ifdef SX_STAMPS
    unsigned long long* stamps = nullptr;   // the register-resident kernels take the stamp buffer as an argument
#endif
};

// BYOUT = false: Kstar of all outputs in LDS at once -- two barriers per step (the kernel measured throughout DESIGN.md).
// BYOUT = true: for training sets whose n_s Kstar buffers do not fit in LDS together, one output at a time
// (Kstar_d | MFMA_d for d = 0 .. n_s - 1: 2 n_s barriers per step, per-output stage streams), still ONE launch for the
// whole rollout and no Kstar in HBM.
// SH > 0 (sx_cem_rollout_junk): the GP's inputs are D = NS + NU + SH columns -- training rows [x, u, 0_SH], queries
// [p, 0_SH, u] -- while the reachability and the costs see (NS, NU) and the Jacobian's leading NS + NU columns (the
// exact-GP form of JunkDimensionsSSM).  SH = 0 is the plain rollout.
// MM = true (sx_cem_rollout_multi): every problem has a GP of its own.  The first argument is then the device table of
// the E problems' GpConst (sx_gp_model_table), the workgroup reads its problem's entry with scalar loads (the pointer is
// restrict-qualified and the kernel never writes it), `stage_tab` is unused (each entry carries its own), the LDS
// carve-up follows the problem's n_train / n_pad inside the launch's allocation for the largest model, and `rp.status`
// holds one word per problem.
// (The problem index is derived inside `of`, so that the plain mode's statements keep their order and its ISA.)
template <int NS, int D, bool MM>
struct RolloutGpArg {
    using type = GpConst<NS, D>;
    __device__ static const GpConst<NS, D>& of(const type& gc, const RolloutPtrs&) { return gc; }
};
template <int NS, int D>
struct RolloutGpArg<NS, D, true> {
    using type = const GpConst<NS, D>* __restrict__;
    __device__ static const GpConst<NS, D>& of(type table, const RolloutPtrs& rp) {
        return table[blockIdx.x / ((rp.P + SX_TILE - 1) / SX_TILE)];
    }
};

template <int NS, int NU, bool BYOUT = false, int SH = 0, bool MM = false>
__global__ __launch_bounds__(kRolloutThreads) void cem_rollout_kernel(
    typename RolloutGpArg<NS, NS + NU + SH, MM>::type gc_arg, const int4* __restrict__ stage_tab_arg,
    ReachConst<NS, NU> rc, CostConst<SX_MAX_M, NS, NU> cc, RolloutPtrs rp) {
#define SX_ROLLOUT_PS 0
#define SX_ROLLOUT_SAT 0
#define SX_ROLLOUT_CONS 0
#include "sx_rollout_body.inc"
#undef SX_ROLLOUT_CONS
#undef SX_ROLLOUT_SAT
#undef SX_ROLLOUT_PS
}

// sx_cem_rollout_starts: cem_rollout_kernel with a start state per particle, the first NS entries of its CEM row (the
// SX_ROLLOUT_PS sections of sx_rollout_body.inc).  Plain models only: no query shift, one GP.
template <int NS, int NU, bool BYOUT>
__global__ __launch_bounds__(kRolloutThreads) void cem_rollout_starts_kernel(
    GpConst<NS, NS + NU> gc_arg, const int4* __restrict__ stage_tab_arg, ReachConst<NS, NU> rc,
    CostConst<SX_MAX_M, NS, NU> cc, RolloutPtrs rp) {
    constexpr int SH = 0;
    constexpr bool MM = false;
#define SX_ROLLOUT_PS 1
#define SX_ROLLOUT_SAT 0
#define SX_ROLLOUT_CONS 0
#include "sx_rollout_body.inc"
#undef SX_ROLLOUT_CONS
#undef SX_ROLLOUT_SAT
#undef SX_ROLLOUT_PS
}

// sx_cem_rollout[_elites]_sat[_multi]: cem_rollout_kernel (SH = 0) with the saturating cost of sx_sat_cost.hpp as the
// objective, priced on the safety ellipsoids (p_{t+1}, Q_{t+1}) read as means and covariances (the SX_ROLLOUT_SAT section
// of sx_rollout_body.inc) -- what the reference's n_perf = 0 configs hand their solver.  The cost's
// constants are one more kernel argument, uniform and read by scalar loads on the owner lanes: the LDS plan is the
// parent's byte for byte.  MM and the elite-row prologue are the body's own, so one kernel serves the four entries.
template <int NS, int NU, bool MM>
constexpr size_t rollout_sat_arg_bytes() {
    constexpr size_t a = 8;   // every argument starts on 8 bytes
    return ((sizeof(typename RolloutGpArg<NS, NS + NU, MM>::type) + a - 1) / a + (sizeof(const int4*) + a - 1) / a +
            (sizeof(ReachConst<NS, NU>) + a - 1) / a + (sizeof(CostConst<SX_MAX_M, NS, NU>) + a - 1) / a +
            (sizeof(RolloutPtrs) + a - 1) / a + (sizeof(SatConst<NS>) + a - 1) / a) * a;
}
constexpr size_t kMaxKernelArgBytes = 4096;   // what a HIP launch takes

template <int NS, int NU, bool BYOUT, bool MM>
__global__ __launch_bounds__(kRolloutThreads) void cem_rollout_sat_kernel(
    typename RolloutGpArg<NS, NS + NU, MM>::type gc_arg, const int4* __restrict__ stage_tab_arg, ReachConst<NS, NU> rc,
    CostConst<SX_MAX_M, NS, NU> cc, RolloutPtrs rp, const SatConst<NS> sat) {
    static_assert(rollout_sat_arg_bytes<NS, NU, MM>() <= kMaxKernelArgBytes, "the kernel arguments exceed a launch's limit");
    constexpr int SH = 0;
#define SX_ROLLOUT_PS 0
#define SX_ROLLOUT_SAT 1
#define SX_ROLLOUT_CONS 0
#include "sx_rollout_body.inc"
#undef SX_ROLLOUT_CONS
#undef SX_ROLLOUT_SAT
#undef SX_ROLLOUT_PS
}

// sx_cem_rollout[_elites]_cons[_multi]: cem_rollout_kernel (SH = 0; MM: a GP per problem) with the constraint set of
// sx_conset.hpp in finish() (the SX_ROLLOUT_CONS sections of sx_rollout_body.inc) and, with SAT, the
// saturating cost on the safety ellipsoids as the objective, as cem_rollout_sat_kernel has it.  The set's constants are one
// more kernel argument, uniform and read by scalar loads on the owner lanes: the LDS plan is the parent's byte for byte.
// The two objectives are two templates of one name (the body is text, and its objective a preprocessor choice); SAT picks
// between them.  With MM the set stays ONE argument shared by all problems (the scenarios share sx_env, and so the set);
// only the GP is per problem.
template <int NS, int NU, bool MM>
constexpr size_t rollout_cons_arg_bytes() {
    return rollout_sat_arg_bytes<NS, NU, MM>() + (sizeof(ConConst<NS>) + 7) / 8 * 8;
}

template <int NS, int NU, bool BYOUT, bool SAT, bool MM, std::enable_if_t<!SAT, int> = 0>
__global__ __launch_bounds__(kRolloutThreads) void cem_rollout_cons_kernel(
    typename RolloutGpArg<NS, NS + NU, MM>::type gc_arg, const int4* __restrict__ stage_tab_arg, ReachConst<NS, NU> rc,
    CostConst<SX_MAX_M, NS, NU> cc, RolloutPtrs rp, const ConConst<NS> cons) {
    constexpr int SH = 0;
#define SX_ROLLOUT_PS 0
#define SX_ROLLOUT_SAT 0
#define SX_ROLLOUT_CONS 1
#include "sx_rollout_body.inc"
#undef SX_ROLLOUT_CONS
#undef SX_ROLLOUT_SAT
#undef SX_ROLLOUT_PS
}

template <int NS, int NU, bool BYOUT, bool SAT, bool MM, std::enable_if_t<SAT, int> = 0>
__global__ __launch_bounds__(kRolloutThreads) void cem_rollout_cons_kernel(
    typename RolloutGpArg<NS, NS + NU, MM>::type gc_arg, const int4* __restrict__ stage_tab_arg, ReachConst<NS, NU> rc,
    CostConst<SX_MAX_M, NS, NU> cc, RolloutPtrs rp, const ConConst<NS> cons, const SatConst<NS> sat) {
    static_assert(rollout_cons_arg_bytes<NS, NU, MM>() <= kMaxKernelArgBytes, "the kernel arguments exceed a launch's limit");
    constexpr int SH = 0;
#define SX_ROLLOUT_PS 0
#define SX_ROLLOUT_SAT 1
#define SX_ROLLOUT_CONS 1
#include "sx_rollout_body.inc"
#undef SX_ROLLOUT_CONS
#undef SX_ROLLOUT_SAT
#undef SX_ROLLOUT_PS
}

// sx_cem_rollout_starts_cons: cem_rollout_starts_kernel with the constraint set of sx_conset.hpp (the SX_ROLLOUT_PS and the
// SX_ROLLOUT_CONS sections of sx_rollout_body.inc together; DESIGN.md section 3.10, "the constraint set"): the reference's
// static-exploration NLP has the gain fixed, so the set is its constraints term for term.  The set is one more kernel
// argument, as cem_rollout_cons_kernel takes it: the LDS plan is cem_rollout_starts_kernel's byte for byte.
template <int NS, int NU>
constexpr size_t rollout_starts_cons_arg_bytes() {
    return rollout_cons_arg_bytes<NS, NU, false>() - (sizeof(SatConst<NS>) + 7) / 8 * 8;
}

template <int NS, int NU, bool BYOUT>
__global__ __launch_bounds__(kRolloutThreads) void cem_rollout_starts_cons_kernel(
    GpConst<NS, NS + NU> gc_arg, const int4* __restrict__ stage_tab_arg, ReachConst<NS, NU> rc,
    CostConst<SX_MAX_M, NS, NU> cc, RolloutPtrs rp, const ConConst<NS> cons) {
    static_assert(rollout_starts_cons_arg_bytes<NS, NU>() <= kMaxKernelArgBytes, "the kernel arguments exceed a launch's limit");
    constexpr int SH = 0;
    constexpr bool MM = false;
#define SX_ROLLOUT_PS 1
#define SX_ROLLOUT_SAT 0
#define SX_ROLLOUT_CONS 1
#include "sx_rollout_body.inc"
#undef SX_ROLLOUT_CONS
#undef SX_ROLLOUT_SAT
#undef SX_ROLLOUT_PS
}

}  // namespace sx
