// The per-particle step of the fused CEM rollouts that follows the model prediction -- the action draw, the constraint
// costs, the trajectory and variance stores -- and the particle slots of the kernels that hold one particle per lane.
// Shared by the big-N step kernel (sx_big.hpp), the feature-GP lane kernel (sx_feat.hpp) and the matrix-core MC-dropout
// kernel (sx_mlp_mfma.hpp).  The streaming kernel (sx_rollout.hpp) and the MC-dropout lane kernel (sx_mlp.hpp) spell
// their step out: on these helpers their code changes, and they run 2 % slower.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sx_amd.h"
#include "sx_reach.hpp"

namespace sx {

// The buffers of the feature-GP and MC-dropout rollouts (sx_cem_rollout_feat[_junk|_multi], sx_cem_rollout_mlp[...]).
struct FeatRolloutPtrs {
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
};

// The model argument of the rollout kernels of the feature-GP and MC-dropout families: the constants C themselves, or
// with MM = true (sx_cem_rollout_feat_multi / sx_cem_rollout_mlp_multi) the device table of the E problems' constants
// (sx_feat_model_table / sx_mlp_model_table), of which the workgroup binds its problem's entry.  The pointer is
// restrict-qualified and never written, and the index is uniform: the fields come through scalar loads.  The entry is
// read through the constant address space, which the table is for the launch: the compiler then takes the device
// pointers it holds (weights, masks) to be global, as it does for those of a kernel argument, and reads through them
// with global loads rather than flat ones.
template <typename C, bool MM>
struct ModelArg {
    using type = C;
    __device__ static const C& of(const type& c, int) { return c; }
};
template <typename C>
struct ModelArg<C, true> {
    using type = const C* __restrict__;
    __device__ static const C& of(type table, int e) {
        using ConstC = __attribute__((address_space(4))) const C;
        return *(const C*)((ConstC*)table + e);
    }
};

// MM: the problem of this workgroup.  A multi-model launch covers every problem with ceil(P / TILE) workgroups of its own
// (TILE particles each), so the problem follows from blockIdx alone and is uniform.
template <int TILE>
__device__ __forceinline__ int tile_problem(int P) {
    return (int)blockIdx.x / ((P + TILE - 1) / TILE);
}

// Particle index of this lane within its problem's tiles (MM): `lane` of the workgroup's tile of TILE particles.
template <int TILE>
__device__ __forceinline__ int tile_particle(int e, int P, int lane) {
    return ((int)blockIdx.x - e * ((P + TILE - 1) / TILE)) * TILE + lane;
}

// The particle of `lane` (0 .. TILE - 1) of a workgroup of TILE particles: its [E x P ...] buffer index g, the index gg it
// reads through (g, or for a lane past the particles the first particle of its problem -- of the launch, plain mode), its
// problem e, and whether it is a particle at all (`valid`: only valid lanes write).  Plain mode: the E P particles in a
// row; MM: problem-aligned workgroups (tile_problem).
template <int TILE, bool MM>
__device__ __forceinline__ void particle_slot(const FeatRolloutPtrs& rp, int lane, int64_t& g, int64_t& gg, int& e,
                                              bool& valid) {
    if constexpr (MM) {
        e = tile_problem<TILE>(rp.P);
        const int i = tile_particle<TILE>(e, rp.P, lane);
        valid = i < rp.P;
        g = (int64_t)e * rp.P + i;
        gg = valid ? g : (int64_t)e * rp.P;
    } else {
        const int64_t total = (int64_t)rp.E * rp.P;
        g = blockIdx.x * (int64_t)TILE + lane;
        valid = g < total;
        gg = valid ? g : 0;
        e = (int)(gg / rp.P);
    }
}

// Action c of step t of the particle read through gg (problem e): drawn as mean + std * noise and stored for a valid
// particle, or, without noise, the given action.
template <int NU>
__device__ __forceinline__ double step_action(const FeatRolloutPtrs& rp, int e, int64_t gg, int H, int t, int c,
                                              bool valid) {
    const int64_t gi = (gg * H + t) * NU + c;
    double a;
    if (rp.noise) {
        a = rp.mean[((int64_t)e * H + t) * NU + c] + rp.std[((int64_t)e * H + t) * NU + c] * rp.noise[gi];
        if (valid) rp.actions[gi] = a;
    } else {
        a = rp.actions[gi];
    }
    return a;
}

// The constraint costs of step t of H (safempc_cem.py:102-132,304-312; action constraint: test_safempc_cem.py:59-71) for
// the action u and the state (p1, Q1) it leads to, added to con: the action box, then the state constraint -- every step,
// or the last only, by con_mode.  (The objective is objective_cost.)
template <int NS, int NU>
__device__ __forceinline__ void constraint_costs(const CostConst<SX_MAX_M, NS, NU>& cc, const double (&u)[NU],
                                                 const double (&p1)[NS], const double (&Q1)[NS][NS], int t, int H,
                                                 double& con) {
    double c = con;   // (a local: summed through the reference, the kernels compile differently)
    bool uviol = false;
#pragma unroll
    for (int k = 0; k < NU; ++k) uviol = uviol || (u[k] < cc.u_min[k]) || (u[k] > cc.u_max[k]);
    if (uviol) c += SX_ACTION_VIOLATION_COST;
    if (cc.con_mode == SX_CON_ALL_STATES || t == H - 1) {
        if (polytope_violated<SX_MAX_M, NS>(cc.h_mat, cc.h_vec, cc.m, 1.0, p1, Q1, nullptr)) c += SX_STATE_VIOLATION_COST;
    }
    con = c;
}

// Row t of particle g's trajectory ([p1, Q1], where traj is wanted) and variances (where sigma is), for a valid particle.
template <int NS>
__device__ __forceinline__ void store_step(double* traj, double* sigma, bool valid, int64_t g, int H, int t,
                                           const double (&p1)[NS], const double (&Q1)[NS][NS], const double (&var)[NS]) {
    constexpr int S = NS + NS * NS;
    if (valid && traj) {
        double* tr = traj + (g * H + t) * S;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            tr[i] = p1[i];
#pragma unroll
            for (int j = 0; j < NS; ++j) tr[NS + i * NS + j] = Q1[i][j];
        }
    }
    if (valid && sigma) {
#pragma unroll
        for (int i = 0; i < NS; ++i) sigma[(g * H + t) * NS + i] = var[i];
    }
}

// The body of a one-particle-per-lane rollout kernel (cem_rollout_feat_kernel; cem_rollout_mlp_kernel spells the same
// body out: compiled through this one it runs 4 % slower): LANES particles per workgroup, each for all H steps.
// `predict(with_jac, model, z, lane, mean, var, jac)` is the model's prediction at z (with_jac: std::true_type /
// std::false_type).  The kernel arguments come by reference: a copy of the model constants would go to scratch.
// SH > 0 (the _junk entries): the model's inputs are D = NS + NU + SH columns -- training rows [x, u, 0_SH], queries
// [p, 0_SH, u] -- while the reachability and the costs see (NS, NU) and the Jacobian's leading NS + NU columns
// (JunkDimensionsSSM).  SH = 0 is the plain rollout.
// MM = true (the _multi entries, SH = 0): every problem has a model of its own, `model_arg` is the device table of their
// constants (ModelArg), and `rp.status` holds one word per problem.
template <int NS, int NU, int SH, bool MM, int LANES, typename C, typename Predict>
__device__ __forceinline__ void cem_rollout_lanes(const typename ModelArg<C, MM>::type& model_arg,
                                                  const ReachConst<NS, NU>& rc, const CostConst<SX_MAX_M, NS, NU>& cc,
                                                  const FeatRolloutPtrs& rp, Predict predict) {
    static_assert(!MM || SH == 0, "the multi-model rollout has no query shift");
    constexpr int D = NS + NU + SH;
    constexpr int UC = NS + SH;   // first action column of a query row
    static_assert(D <= SX_MAX_D, "the model's first layer holds at most SX_MAX_D inputs");
    const int lane = threadIdx.x;
    int64_t g, gg;
    bool valid;
    int e;
    particle_slot<LANES, MM>(rp, lane, g, gg, e, valid);
    const C& model = ModelArg<C, MM>::of(model_arg, e);
    const int H = rp.H;
    double p[NS], Q[NS][NS];
    bool have_q = rp.q0 != nullptr;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        p[i] = rp.x0[(int64_t)e * NS + i];
#pragma unroll
        for (int j = 0; j < NS; ++j) Q[i][j] = have_q ? rp.q0[((int64_t)e * NS + i) * NS + j] : 0.0;
    }
    double obj = 0.0, con = 0.0;
    int st = 0;
    for (int t = 0; t < H; ++t) {
        double z[D], u[NU], mean[NS], var[NS], jac[NS][D], p1[NS], Q1[NS][NS];
#pragma unroll
        for (int c = 0; c < NU; ++c) u[c] = step_action<NU>(rp, e, gg, H, t, c, valid);
#pragma unroll
        for (int j = 0; j < NS; ++j) z[j] = p[j];
#pragma unroll
        for (int j = NS; j < UC; ++j) z[j] = 0.0;
#pragma unroll
        for (int c = 0; c < NU; ++c) z[UC + c] = u[c];
        if (have_q) {
            predict(std::true_type{}, model, z, lane, mean, var, jac);
            if constexpr (SH == 0) {
                reach_ellipsoid<NS, NU>(rc, p, Q, u, mean, var, jac, p1, Q1, st);
            } else {
                // [A | B]: the derivatives by the TRAINING rows' state and action columns (the reference's padding)
                double jab[NS][NS + NU];
#pragma unroll
                for (int i = 0; i < NS; ++i)
#pragma unroll
                    for (int j = 0; j < NS + NU; ++j) jab[i][j] = jac[i][j];
                reach_ellipsoid<NS, NU>(rc, p, Q, u, mean, var, jab, p1, Q1, st);
            }
        } else {
            predict(std::false_type{}, model, z, lane, mean, var, jac);
            reach_point<NS, NU>(rc, p, u, mean, var, p1, Q1, st);
        }
        have_q = true;
        obj += objective_cost<SX_MAX_M, NS, NU>(cc, p1, var);
        constraint_costs<NS, NU>(cc, u, p1, Q1, t, H, con);
        store_step<NS>(rp.traj, rp.sigma, valid, g, H, t, p1, Q1, var);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            p[i] = p1[i];
#pragma unroll
            for (int j = 0; j < NS; ++j) Q[i][j] = Q1[i][j];
        }
    }
    if (valid) {
        rp.obj_cost[g] = obj;
        rp.con_cost[g] = con;
        if (st) atomicOr(rp.status + (MM ? e : 0), st);
    }
}

}  // namespace sx
