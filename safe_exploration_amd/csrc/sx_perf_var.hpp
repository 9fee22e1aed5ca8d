// The performance trajectory of the CEM solver WITH the GP's posterior variance (sx_cem_perf_rollout_var): n_perf chained
// mean-equivalent steps per particle,
//     (mean_t, var_t) = GP posterior at [mu_t, v_t],      mu_{t+1} = a mu_t + b v_t + mean_t,
// no feedback term, no variance propagation (sigma_x = None), and var_t = s + noise - || W k* ||^2 per output: the N x N
// triangular product of the safety kernels on the f64 matrix cores, where the mean-only kernel (sx_perf.hpp) needs k* . alpha.
//
// Layout: the skeleton of the streaming safety kernel (sx_rollout.hpp) without its finish().  One workgroup of SX_WAVES
// waves owns a tile of 16 particles of one problem for all n_perf steps; the packed model is the safety rollout's (W
// fragments, the mean / Jacobian rows, the stage table of sx_gp_pack).  Step t:
//     Kstar(t) on all waves, equal shares  |sync|  MFMA(t)  |sync|  gp_collect + the step's tail on the 16 owner lanes
// Every Kstar thread derives its query point of step t + 1 from z_t and the posterior means MFMA(t) left in LDS (the
// next_centre fma chain of the safety kernel), so the owner lanes' tail -- next centre, objective, action box, stores --
// runs beside the start of Kstar(t + 1) and costs no third barrier.  z lives in two LDS buffers, as in the safety kernel:
// the owner writes z_{t+1} into buffer (t + 1) & 1 for the threads of step t + 2.
// The stage stream carries the folded Jacobian rows R_d[1 .. D], which this kernel computes and ignores: they ride in the
// row-blocks that hold the mean row and the zero padding anyway, so no MFMA is issued for them alone.
//
// BYOUT = true: output by output (Kstar_d | MFMA_d for d = 0 .. n_s - 1, 2 n_s barriers per step), for training sets whose
// n_s Kstar buffers do not fit in LDS together -- the same per-output stage streams as the safety kernel's.
// A tile's numbers depend on its 16 particles alone: not on P, the grid or the workgroup it lands in.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_perf.hpp"   // PerfStepConst, PerfPtrs
#include "sx_reach.hpp"      // polytope_violated
#include "sx_sat_cost.hpp"   // sat_loss

namespace sx {

constexpr int kPerfVarThreads = 64 * SX_WAVES;

struct PerfVarPtrs {
    PerfPtrs p;
    double* perf_sigma;   // [E x P x n_perf x NS] | NULL: var_0 .. var_{n_perf - 1}
    int obj_mode;         // SX_OBJ_NEG_VARIANCE | SX_OBJ_AFFINE_ABS
};

// The kind K of a GP-product kernel: its step constants K::Const<NS, NU> and pointers K::Ptrs (kernel arguments in both
// modes: there is one sx_env), and the sections of the body it takes.  K::TAYLOR (PerfTaylorKind, sx_perf_taylor.hpp): the
// covariance step, with the step constants in LDS; K::SAT with it: the objective section prices (mu_{t+1}, Sigma_{t+1})
// with the saturating cost of sx_sat_cost.hpp from the constants' `sat`, which stays a kernel argument.
struct PerfVarKind {
    static constexpr bool TAYLOR = false, SAT = false;
    template <int NS, int NU>
    using Const = PerfStepConst<NS, NU>;
    using Ptrs = PerfVarPtrs;
};

// The one GP-product performance kernel.  MM = false: the arguments are (GpConst, its stage table, constants, pointers) --
// TAB... is that one `const int4* __restrict__`, named explicitly by whoever names the kernel.  MM = true (a GP per problem):
// (the device table of sx_gp_model_table, constants, pointers); the workgroup binds its problem's GpConst through a pointer
// into the constant address space (scalar loads; the table is restrict-qualified and the kernel never writes it), the LDS
// carve-up follows the problem's n_train / n_pad inside the launch's allocation for the largest model, and the status is
// one word per problem.  The workgroups are problem-aligned in both modes.
// The sections of a kind are `if constexpr`, directly in this body: every instantiation holds the instructions its kernel
// had as a definition of its own (a device function for the shared part changed the single-model kernels' registers;
// tools/device_code_diff.py is the check).
template <class K, int NS, int NU, bool BYOUT, bool MM, class... TAB>
__global__ __launch_bounds__(kPerfVarThreads) void cem_perf_gp_rollout_kernel(
    const std::conditional_t<MM, const GpConst<NS, NS + NU>* __restrict__, GpConst<NS, NS + NU>> gc_arg,
    const TAB... stage_tab_arg, const typename K::template Const<NS, NU> c_arg, const typename K::Ptrs ptrs) {
    static_assert(sizeof...(TAB) == (MM ? 0 : 1), "TAB... is the single-model kernel's stage table");
    const PerfVarPtrs& vp = ptrs;   // (the pointers of every kind begin with these)
    const auto& tp = ptrs;          // (Taylor: PerfTaylorPtrs)
    // (`vp` and the single-model `gc` are the arguments themselves, bound without a call in between: one that takes either
    // by reference, inlined or not, changes the single-model kernels' registers.  The lambdas below name their captures for
    // the same reason: with `[&]` the Taylor kernels of shape (1, 1) come out with other registers.)
    const GpConst<NS, NS + NU>* gc_ptr;
    if constexpr (MM) {
        using ConstG = __attribute__((address_space(4))) const GpConst<NS, NS + NU>;
        const int problem = blockIdx.x / ((vp.p.P + SX_TILE - 1) / SX_TILE);
        gc_ptr = (const GpConst<NS, NS + NU>*)((ConstG*)gc_arg + problem);
    } else {
        gc_ptr = &gc_arg;
    }
    const GpConst<NS, NS + NU>& gc = *gc_ptr;
    const int4* __restrict__ const stage_tab = [&gc](const auto&... tab) {
        (void)gc;   // (single-model: not read)
        if constexpr (MM) return gc.stage_tab;
        else return (tab, ...);
    }(stage_tab_arg...);
    // Taylor: the constants the step reads from LDS, without the cost's
    const auto& tc_arg = [&c_arg]() -> decltype(auto) {
        if constexpr (K::SAT) return (c_arg.tc);
        else return (c_arg);
    }();
    constexpr int D = NS + NU;
    constexpr int nw = kPerfVarThreads / 64;
    const PerfPtrs& pp = vp.p;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    GpTileLds<NS, D> lds;
    double* acts = lds.carve(smem, gc.n_train, gc.n_pad, nw, BYOUT ? 1 : NS);   // [16][n_perf][NU]: v_t of the tile
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int H = pp.H, r = pp.r, n_perf = pp.n_perf, T = n_perf - r;
    const int tiles_per_problem = (pp.P + SX_TILE - 1) / SX_TILE;
    const int e = blockIdx.x / tiles_per_problem;
    const int c0 = (blockIdx.x - e * tiles_per_problem) * SX_TILE;   // first particle of the tile within problem e

    // the head of this wave's MFMA stream travels while X, the exp table and the actions are loaded (as in sx_rollout.hpp;
    // output by output every phase fetches the head of its own stream)
    const MfmaHead head = gp_mfma_head(gc, stage_tab, wave, nw, lane, gc.stage_cap);
    const int4* __restrict__ const tab_one = stage_tab + (size_t)nw * (1 + gc.stage_cap);
    gp_load_xs(gc, lds);
    // Taylor: the step constants sit in LDS behind the actions, copied in one pass (`sc` is the variance kernels' argument)
    using StepConst = std::remove_cv_t<std::remove_reference_t<decltype(tc_arg)>>;   // PerfTaylorConst | PerfStepConst
    double* const tcl = acts + SX_TILE * n_perf * NU;
    const StepConst& tc = K::TAYLOR ? *reinterpret_cast<const StepConst*>(tcl) : tc_arg;
    const PerfStepConst<NS, NU>& sc = [&tc]() -> const PerfStepConst<NS, NU>& {
        if constexpr (K::TAYLOR) return tc.step;
        else return tc;
    }();
    if constexpr (K::TAYLOR) {
        constexpr int kConst = (int)(sizeof(StepConst) / sizeof(double));
        static_assert(kConst <= kPerfVarThreads, "one pass copies the step constants");
        static_assert(sizeof(StepConst) % sizeof(double) == 0, "doubles only");
        if (tid < kConst) tcl[tid] = reinterpret_cast<const double*>(&tc_arg)[tid];
    }

    // the tile's rows [safety actions | tail] (the tail drawn by the expression of sx_perf.hpp, or read), and its
    // performance actions v_t = u^s_t (t < r), u^p_t (t >= r) into LDS; a slot past the particles holds zeros
    const int row_len = (H + T) * NU, hl = H * NU;
    for (int i = tid; i < SX_TILE * row_len; i += kPerfVarThreads) {
        const int c = i / row_len, j = i - c * row_len;
        double val = 0.0;
        if (c0 + c < pp.P) {
            const int64_t g = (int64_t)e * pp.P + c0 + c;
            double* row = pp.rows + g * row_len;
            if (j < hl) {
                val = pp.safe_actions[g * hl + j];
                row[j] = val;
            } else if (pp.tail_noise) {
                const int k = j - hl;
                const int64_t ek = (int64_t)e * T * NU + k;
                val = fma(pp.tail_std[ek], pp.tail_noise[g * T * NU + k], pp.tail_mean[ek]);
                row[j] = val;
            } else {
                val = row[j];
            }
        }
        if (j < r * NU)
            acts[c * n_perf * NU + j] = val;
        else if (j >= hl)
            acts[c * n_perf * NU + r * NU + (j - hl)] = val;
    }
    // per-particle state lives in the registers of thread c (tid < 16) for the whole rollout
    const bool owner = tid < SX_TILE;
    const bool valid = owner && (c0 + tid < pp.P);
    double mu[NS];
    double obj = 0.0, con = 0.0;
    int st = 0;
    if (owner) {
#pragma unroll
        for (int i = 0; i < NS; ++i) mu[i] = pp.x0[(int64_t)e * NS + i];
    }
    double S[NS][NS];   // Taylor: Sigma_t beside mu_t on the owner lane, both triangles; Sigma_0 = 0
    if constexpr (K::TAYLOR) {
        if (owner) {
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) S[i][j] = 0.0;
        }
    }
    __syncthreads();
    if (owner) {
#pragma unroll
        for (int i = 0; i < NS; ++i) lds.zs[tid * D + i] = mu[i];
#pragma unroll
        for (int cidx = 0; cidx < NU; ++cidx) lds.zs[tid * D + NS + cidx] = acts[(tid * n_perf + 0) * NU + cidx];
    }
    __syncthreads();

    double* const zs_base = lds.zs;
    // centre of particle c at step t >= 1 from z_{t-1} and the means of step t - 1 (the chain of sx_rollout.hpp)
    auto next_centre = [&](int c, const double* z_prev, double (&out)[NS]) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double s = lds.mj[i * 256 + c];   // posterior mean of output i
#pragma unroll
            for (int j = 0; j < NS; ++j) s = fma(sc.a[i * NS + j], z_prev[j], s);
#pragma unroll
            for (int cidx = 0; cidx < NU; ++cidx) s = fma(sc.b[i * NU + cidx], z_prev[NS + cidx], s);
            out[i] = s;
        }
    };
    // the rest of step t on the owner lanes: posterior (Taylor: and the covariance step), next centre, costs, stores
    auto tail = [&](int t) {
        double z[D], mean[NS], var[NS], jac[NS][D], mu1[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) z[j] = mu[j];
#pragma unroll
        for (int cidx = 0; cidx < NU; ++cidx) z[NS + cidx] = acts[(tid * n_perf + t) * NU + cidx];
        gp_collect<NS, D, K::TAYLOR>(gc, lds, nw, tid, z, mean, var, jac);   // Taylor: with the Jacobian rows
        next_centre(tid, z, mu1);   // exactly the centre the Kstar threads of step t + 1 derive
        if (t + 1 < n_perf) {
            double* zn = zs_base + ((t + 1) & 1) * 16 * D + tid * D;
#pragma unroll
            for (int i = 0; i < NS; ++i) zn[i] = mu1[i];
#pragma unroll
            for (int cidx = 0; cidx < NU; ++cidx) zn[NS + cidx] = acts[(tid * n_perf + t + 1) * NU + cidx];
        }
        double Gt[NS], S1[NS][NS];   // Taylor: diag G_t and Sigma_{t+1}
        bool bad = false;
        if constexpr (K::TAYLOR) {
            // Taylor: G = diag(var) + diag(M Sigma M^T) and Sigma_{t+1} = Hm Sigma Hm^T + diag(var) (upper triangle, then
            // mirrored), with M = J_x + J_u K, Hm = (a + b K) + M; MS = M Sigma, HS = Hm Sigma
            double M[NS][NS], Hm[NS][NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) {
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double s = jac[i][j];
#pragma unroll
                    for (int cidx = 0; cidx < NU; ++cidx) s = fma(jac[i][NS + cidx], tc.k_fb[cidx * NS + j], s);
                    M[i][j] = s;
                    Hm[i][j] = tc.abk[i * NS + j] + s;
                }
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                double ms[NS], hs[NS];   // rows i of M Sigma and Hm Sigma
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double a = 0.0, b = 0.0;
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        a = fma(M[i][k], S[k][j], a);
                        b = fma(Hm[i][k], S[k][j], b);
                    }
                    ms[j] = a;
                    hs[j] = b;
                }
                double g = 0.0;
#pragma unroll
                for (int j = 0; j < NS; ++j) g = fma(ms[j], M[i][j], g);
                Gt[i] = var[i] + g;
#pragma unroll
                for (int j = i; j < NS; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < NS; ++k) s = fma(hs[k], Hm[j][k], s);
                    S1[i][j] = (j == i) ? s + var[i] : s;
                    bad = bad || !(__builtin_fabs(S1[i][j]) <= 1.7976931348623157e308);
                }
                bad = bad || !(__builtin_fabs(mu1[i]) <= 1.7976931348623157e308) ||
                      !(__builtin_fabs(var[i]) <= 1.7976931348623157e308) || !(__builtin_fabs(Gt[i]) <= 1.7976931348623157e308);
            }
#pragma unroll
            for (int i = 1; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < i; ++j) S1[i][j] = S1[j][i];
        } else {
#pragma unroll
            for (int i = 0; i < NS; ++i)
                bad = bad || !(__builtin_fabs(mu1[i]) <= 1.7976931348623157e308) ||
                      !(__builtin_fabs(var[i]) <= 1.7976931348623157e308);
        }
        const double (&G)[NS] = K::TAYLOR ? Gt : var;   // what the objective and perf_sigma see
        double o = 0.0;
        if constexpr (K::SAT) {
            // the saturating cost of (mu_{t+1}, Sigma_{t+1}) (sx_sat_cost.hpp); a non-finite loss never ranks
            o = sat_loss<NS>(c_arg.sat, mu1, S1);
            bad = bad || !(__builtin_fabs(o) <= 1.7976931348623157e308);
        } else if (vp.obj_mode == SX_OBJ_NEG_VARIANCE) {
#pragma unroll
            for (int i = 0; i < NS; ++i) o -= G[i];
        } else {
#pragma unroll
            for (int i = 0; i < NS; ++i) o += sc.w_abs[i] * fabs(sc.target[i] - mu1[i]) + sc.w_lin[i] * mu1[i];
        }
        obj += o;
        if (bad) {
            // a non-finite state, variance or covariance never ranks (the table exponential maps an infinite distance to
            // k* = 0)
            st |= SX_STATUS_NAN;
            obj = __builtin_nan("");
        }
        if (t >= r) {
            bool uviol = false;
#pragma unroll
            for (int cidx = 0; cidx < NU; ++cidx)
                uviol = uviol || (z[NS + cidx] < sc.u_min[cidx]) || (z[NS + cidx] > sc.u_max[cidx]);
            if (uviol) con += SX_ACTION_VIOLATION_COST;
        }
        if constexpr (K::TAYLOR) {
            if (t == tp.safety_step) {
                // Taylor: the terminal-safety coupling: (mu_s, Sigma_s), s = t + 1 = H + 2, inside the safe polytope
                if (polytope_violated<SX_MAX_M, NS>(tc.h_mat, tc.h_vec, tp.m, 1.0, mu1, S1, nullptr))
                    con += SX_STATE_VIOLATION_COST;
            }
        }
        const int64_t g = (int64_t)e * pp.P + c0 + tid;
        if (valid && pp.perf_traj) {
#pragma unroll
            for (int i = 0; i < NS; ++i) pp.perf_traj[(g * n_perf + t) * NS + i] = mu1[i];
        }
        if (valid && vp.perf_sigma) {
#pragma unroll
            for (int i = 0; i < NS; ++i) vp.perf_sigma[(g * n_perf + t) * NS + i] = G[i];
        }
        if constexpr (K::TAYLOR) {
            // Taylor: Sigma_{t+1} goes out and becomes the next step's Sigma
            if (valid && tp.perf_cov) {
                double* cv = tp.perf_cov + (g * n_perf + t) * (NS * NS);
#pragma unroll
                for (int i = 0; i < NS; ++i)
#pragma unroll
                    for (int j = 0; j < NS; ++j) cv[i * NS + j] = S1[i][j];
            }
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) S[i][j] = S1[i][j];
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) mu[i] = mu1[i];
    };

    int q_begin, q_end;   // this wave's share of the Kstar pairs: all waves alike
    kstar_pair_range(gc.n_pad >> 3, wave, 1, nw, q_begin, q_end);
    for (int t = 0; t < n_perf; ++t) {
        // the query point of this thread's particle
        double zq[D];
        {
            const int c = lane & 15;
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < D; ++j) zq[j] = zs_base[c * D + j];
            } else {
                double pc[NS];
                next_centre(c, zs_base + ((t - 1) & 1) * 16 * D + c * D, pc);
#pragma unroll
                for (int i = 0; i < NS; ++i) zq[i] = pc[i];
#pragma unroll
                for (int cidx = 0; cidx < NU; ++cidx) zq[NS + cidx] = acts[(c * n_perf + t) * NU + cidx];
            }
        }
        if constexpr (BYOUT) {
            // (z was derived above, before MFMA_0 overwrites the means of the previous step)
            auto one_output = [&](auto dtag) {
                constexpr int DD = decltype(dtag)::value;
                if constexpr (DD < NS) {
                    const int4* __restrict__ tab_d = tab_one + (size_t)DD * nw * (1 + gc.stage_cap_one);
                    const MfmaHead head_d = gp_mfma_head(gc, tab_d, wave, nw, lane, gc.stage_cap_one);
                    gp_kstar_phase_one<NS, D, DD>(gc, lds, q_begin, q_end, zq);
                    __syncthreads();
                    gp_mfma_phase<NS, D, 1>(gc, tab_d, lds, wave, nw, lane, head_d, gc.stage_cap_one, DD);
                    __syncthreads();
                }
            };
            one_output(std::integral_constant<int, 0>{});
            one_output(std::integral_constant<int, 1>{});
            one_output(std::integral_constant<int, 2>{});
            one_output(std::integral_constant<int, 3>{});
            static_assert(NS <= 4, "one_output is spelled out for up to four outputs");
        } else {
            gp_kstar_phase(gc, lds, q_begin, q_end, zq);
            __syncthreads();
            gp_mfma_phase(gc, stage_tab, lds, wave, nw, lane, head, gc.stage_cap);
            __syncthreads();
        }
        if (owner) tail(t);
    }
    if (valid) {
        const int64_t g = (int64_t)e * pp.P + c0 + tid;
        pp.obj_cost[g] = obj;
        pp.con_cost[g] += con;
        if (st) atomicOr(pp.status + (MM ? e : 0), st);
    }
}

}  // namespace sx
