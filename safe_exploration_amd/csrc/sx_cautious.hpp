// The chance-constrained Taylor rollout of Cautious MPC (sx_cem_cautious_rollout): the trajectory of the Taylor form
// (sx_perf_taylor.hpp) on its own -- no safety rollout in front of it, rows of T feed-forward controls k_ff_0 .. k_ff_{T-1}
// -- with the reference's chance constraints on every step (generate_safety_constraints / _generate_control_constraint,
// cautious_mpc.py:337-442, at c_safety = beta).  Per particle, mu_0 = x0, Sigma_0 = 0, K = k_fb:
//     control   t = 0: k_ff_0 outside [u_min, u_max];   t >= 1: k_ff_t[c] +- beta sqrt(K_c Sigma_t K_c^T) against the box
//     (mean_t, var_t, J_t), M, Hm, G_t, mu_{t+1}, Sigma_{t+1}: the Taylor form's, statement by statement
//     state     some row j: h_j . mu_{t+1} + beta sqrt(h_j^T Sigma_{t+1} h_j) - h_vec_j >= 0
// d >= 0 violates and a NaN distance counts as inside (polytope_violated, sx_reach.hpp).  propagate == 0: the GP step starts
// from Sigma_t = 0 (G_t = var_t, Sigma_{t+1} = diag(var_t): one_step_mean_equivalent); the control constraint of step t
// still sees diag(var_{t-1}).
//
// Layout: the Taylor kernel's -- Kstar(t) |sync| MFMA(t) |sync| tail on the 16 owner lanes beside Kstar(t + 1), the step
// constants (the Taylor constants plus beta) in LDS behind the tile's actions -- with a body of its own: the rows are the
// actions (no [safety | tail] split), con_cost is overwritten, and the tail gains the constraint algebra:
// 2 m n_s^2 + 2 n_u n_s^2 FMAs and m + n_u square roots per step on the owner lane.  The covariance step is written as in
// cem_perf_gp_rollout_kernel (sx_perf_var.hpp), fma for fma: with m = 0 and a wide box mu, diag G and Sigma are the Taylor
// kernel's bits.
// A tile's numbers depend on its 16 particles alone -- in the multi-model mode (MM, sx_cem_cautious_rollout_multi: a GP per
// problem behind a device table) on them and on its problem's model.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sx_amd.h"
#include "sx_gp.hpp"
#include "sx_perf_taylor.hpp"   // PerfTaylorConst, PerfVarPtrs, kPerfVarThreads

namespace sx {

template <int NS, int NU>
struct CautiousConst {
    PerfTaylorConst<NS, NU> tc;
    double beta;
};

struct CautiousPtrs {
    PerfPtrs p;          // x0, tail_mean / tail_std / tail_noise (the row's distribution), rows, obj_cost, con_cost
                         // (overwritten), perf_traj, status; H = n_perf = T, r = 0, no safe_actions
    double* sigma;       // [E x P x T x NS] | NULL: diag G_t
    double* cov;         // [E x P x T x NS x NS] | NULL: Sigma_1 .. Sigma_T
    double* margins;     // [E x P x T x 2] | NULL: largest state row distance, largest control distance
    int obj_mode;
    int m;               // polytope rows
    int propagate;       // 0: mean-equivalent GP steps
};

template <int NS, int NU>
constexpr int cautious_const_doubles() {
    return (int)(sizeof(CautiousConst<NS, NU>) / sizeof(double));
}

// sx_cem_cautious_rollout_sat: the saturating cost (sx_sat_cost.hpp) as the objective; the cost's constants ride behind the
// step constants in one kernel argument and stay there (scalar loads on the owner lanes), so the LDS plan is the same.
template <int NS, int NU>
struct CautiousSatConst {
    CautiousConst<NS, NU> cc;
    SatConst<NS> sat;
};

// SAT: the objective section prices (mu_{t+1}, Sigma_{t+1}) with the saturating cost, and the constants argument is a
// CautiousSatConst; nothing else differs (tools/device_code_diff.py: either instantiation holds the instructions its kernel
// had as a definition of its own).
// MM, TAB...: the conventions of cem_perf_gp_rollout_kernel (sx_perf_var.hpp).  MM = false: the arguments are (GpConst, its
// stage table, constants, pointers) -- TAB... is that one `const int4* __restrict__`, named by whoever names the kernel.
// MM = true (a GP per problem): (the device table of sx_gp_model_table, constants, pointers); the workgroup binds its
// problem's GpConst through a pointer into the constant address space, takes the stage table from it, carves the LDS by the
// problem's n_train / n_pad inside the launch's allocation for the largest model, and the status is one word per problem.
// There is one sx_env (and one sx_sat_cost) for all problems.
template <int NS, int NU, bool BYOUT, bool SAT, bool MM, class... TAB>
__global__ __launch_bounds__(kPerfVarThreads) void cem_cautious_rollout_kernel(
    const std::conditional_t<MM, const GpConst<NS, NS + NU>* __restrict__, GpConst<NS, NS + NU>> gc_arg,
    const TAB... stage_tab_arg,
    const std::conditional_t<SAT, CautiousSatConst<NS, NU>, CautiousConst<NS, NU>> arg, const CautiousPtrs cp) {
    static_assert(sizeof...(TAB) == (MM ? 0 : 1), "TAB... is the single-model kernel's stage table");
    // (the single-model `gc` is the argument itself, bound as in cem_perf_gp_rollout_kernel: a call that takes it by
    // reference in between changes the single-model kernels' registers)
    const GpConst<NS, NS + NU>* gc_ptr;
    if constexpr (MM) {
        using ConstG = __attribute__((address_space(4))) const GpConst<NS, NS + NU>;
        const int problem = blockIdx.x / ((cp.p.P + SX_TILE - 1) / SX_TILE);
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
    const CautiousConst<NS, NU>& cc_arg = [&]() -> const CautiousConst<NS, NU>& {
        if constexpr (SAT) return arg.cc;
        else return arg;
    }();
    constexpr int D = NS + NU;
    constexpr int nw = kPerfVarThreads / 64;
    const PerfPtrs& pp = cp.p;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    GpTileLds<NS, D> lds;
    double* acts = lds.carve(smem, gc.n_train, gc.n_pad, nw, BYOUT ? 1 : NS);   // [16][T][NU]: k_ff_t of the tile
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int T = pp.n_perf;
    const int tiles_per_problem = (pp.P + SX_TILE - 1) / SX_TILE;
    const int e = blockIdx.x / tiles_per_problem;
    const int c0 = (blockIdx.x - e * tiles_per_problem) * SX_TILE;   // first particle of the tile within problem e

    const MfmaHead head = gp_mfma_head(gc, stage_tab, wave, nw, lane, gc.stage_cap);
    const int4* __restrict__ const tab_one = stage_tab + (size_t)nw * (1 + gc.stage_cap);
    gp_load_xs(gc, lds);
    // the step constants sit in LDS behind the actions, copied in one pass
    constexpr int kConst = cautious_const_doubles<NS, NU>();
    static_assert(kConst <= kPerfVarThreads, "one pass copies the step constants");
    static_assert(sizeof(CautiousConst<NS, NU>) % sizeof(double) == 0, "doubles only");
    const int row_len = T * NU;
    double* const ccl = acts + SX_TILE * row_len;
    const CautiousConst<NS, NU>& cc = *reinterpret_cast<const CautiousConst<NS, NU>*>(ccl);
    const PerfTaylorConst<NS, NU>& tc = cc.tc;
    const PerfStepConst<NS, NU>& sc = tc.step;
    if (tid < kConst) ccl[tid] = reinterpret_cast<const double*>(&cc_arg)[tid];

    // the tile's rows (drawn by the expression of sx_perf.hpp, or read) into LDS; a slot past the particles holds zeros
    for (int i = tid; i < SX_TILE * row_len; i += kPerfVarThreads) {
        const int c = i / row_len, j = i - c * row_len;
        double val = 0.0;
        if (c0 + c < pp.P) {
            const int64_t g = (int64_t)e * pp.P + c0 + c;
            double* row = pp.rows + g * row_len;
            if (pp.tail_noise) {
                const int64_t ej = (int64_t)e * row_len + j;
                val = fma(pp.tail_std[ej], pp.tail_noise[g * row_len + j], pp.tail_mean[ej]);
                row[j] = val;
            } else {
                val = row[j];
            }
        }
        acts[i] = val;
    }
    // per-particle state lives in the registers of thread c (tid < 16) for the whole rollout
    const bool owner = tid < SX_TILE;
    const bool valid = owner && (c0 + tid < pp.P);
    double mu[NS];
    double S[NS][NS];   // Sigma_t, both triangles; Sigma_0 = 0.  propagate == 0: diag(var_{t-1}), which only the control
                        // constraint reads
    double obj = 0.0, con = 0.0;
    int st = 0;
    if (owner) {
#pragma unroll
        for (int i = 0; i < NS; ++i) mu[i] = pp.x0[(int64_t)e * NS + i];
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) S[i][j] = 0.0;
    }
    __syncthreads();
    if (owner) {
#pragma unroll
        for (int i = 0; i < NS; ++i) lds.zs[tid * D + i] = mu[i];
#pragma unroll
        for (int cidx = 0; cidx < NU; ++cidx) lds.zs[tid * D + NS + cidx] = acts[(tid * T + 0) * NU + cidx];
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
    // the rest of step t on the owner lanes: the control constraint on Sigma_t, posterior and covariance step, next centre,
    // the state constraint on Sigma_{t+1}, costs, stores
    auto tail = [&](int t) {
        double z[D], mean[NS], var[NS], jac[NS][D], mu1[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) z[j] = mu[j];
#pragma unroll
        for (int cidx = 0; cidx < NU; ++cidx) z[NS + cidx] = acts[(tid * T + t) * NU + cidx];
        // control: the plain box at t = 0, else the box shrunk by beta sqrt(K_c Sigma_t K_c^T) on either side
        bool uviol = false;
        double umax_d = -__builtin_inf();
#pragma unroll
        for (int cidx = 0; cidx < NU; ++cidx) {
            const double k = z[NS + cidx];
            if (t == 0) {
                uviol = uviol || (k < sc.u_min[cidx]) || (k > sc.u_max[cidx]);
                umax_d = fmax(umax_d, fmax(k - sc.u_max[cidx], sc.u_min[cidx] - k));
            } else {
                double q = 0.0;
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < NS; ++j) s = fma(S[i][j], tc.k_fb[cidx * NS + j], s);
                    q = fma(tc.k_fb[cidx * NS + i], s, q);
                }
                const double spread = cc.beta * sqrt(q);
                const double d_hi = (k + spread) - sc.u_max[cidx], d_lo = (sc.u_min[cidx] - k) + spread;
                uviol = uviol || (d_hi >= 0.0) || (d_lo >= 0.0);
                umax_d = fmax(umax_d, fmax(d_hi, d_lo));
            }
        }
        if (uviol) con += SX_ACTION_VIOLATION_COST;

        gp_collect<NS, D, 1>(gc, lds, nw, tid, z, mean, var, jac);   // with the Jacobian rows
        next_centre(tid, z, mu1);   // exactly the centre the Kstar threads of step t + 1 derive
        if (t + 1 < T) {
            double* zn = zs_base + ((t + 1) & 1) * 16 * D + tid * D;
#pragma unroll
            for (int i = 0; i < NS; ++i) zn[i] = mu1[i];
#pragma unroll
            for (int cidx = 0; cidx < NU; ++cidx) zn[NS + cidx] = acts[(tid * T + t + 1) * NU + cidx];
        }
        if (!cp.propagate) {
            // mean-equivalent: the GP step starts from Sigma_t = 0
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) S[i][j] = 0.0;
        }
        // G = diag(var) + diag(M Sigma M^T) and Sigma_{t+1} = Hm Sigma Hm^T + diag(var) (upper triangle, then mirrored),
        // with M = J_x + J_u K, Hm = (a + b K) + M; MS = M Sigma, HS = Hm Sigma  (sx_perf_var.hpp, fma for fma)
        double M[NS][NS], Hm[NS][NS], G[NS], S1[NS][NS];
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
        bool bad = false;
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
            G[i] = var[i] + g;
#pragma unroll
            for (int j = i; j < NS; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < NS; ++k) s = fma(hs[k], Hm[j][k], s);
                S1[i][j] = (j == i) ? s + var[i] : s;
                bad = bad || !(__builtin_fabs(S1[i][j]) <= 1.7976931348623157e308);
            }
            bad = bad || !(__builtin_fabs(mu1[i]) <= 1.7976931348623157e308) ||
                  !(__builtin_fabs(var[i]) <= 1.7976931348623157e308) || !(__builtin_fabs(G[i]) <= 1.7976931348623157e308);
        }
#pragma unroll
        for (int i = 1; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < i; ++j) S1[i][j] = S1[j][i];
        double o = 0.0;
        if constexpr (SAT) {
            // the saturating cost of (mu_{t+1}, Sigma_{t+1}) (sx_sat_cost.hpp); a non-finite loss never ranks
            o = sat_loss<NS>(arg.sat, mu1, S1);
            bad = bad || !(__builtin_fabs(o) <= 1.7976931348623157e308);
        } else if (cp.obj_mode == SX_OBJ_NEG_VARIANCE) {
#pragma unroll
            for (int i = 0; i < NS; ++i) o -= G[i];
        } else {
#pragma unroll
            for (int i = 0; i < NS; ++i) o += sc.w_abs[i] * fabs(sc.target[i] - mu1[i]) + sc.w_lin[i] * mu1[i];
        }
        obj += o;
        if (bad) {
            // a non-finite state, variance or covariance never ranks
            st |= SX_STATUS_NAN;
            obj = __builtin_nan("");
        }
        // state: the ellipsoid (mu_{t+1}, Sigma_{t+1}) scaled by beta against every row of the polytope (the sums of
        // polytope_violated); a NaN distance is neither a violation nor a margin
        bool sviol = false;
        double smax_d = -__builtin_inf();
        for (int row = 0; row < cp.m; ++row) {
            double hc = 0.0, hq = 0.0;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const double hi = tc.h_mat[row * NS + i];
                hc += hi * mu1[i];
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NS; ++j) s += S1[i][j] * tc.h_mat[row * NS + j];
                hq += hi * s;
            }
            const double d = hc + cc.beta * sqrt(hq) - tc.h_vec[row];
            sviol = sviol || (d >= 0.0);
            smax_d = fmax(smax_d, d);
        }
        if (sviol) con += SX_STATE_VIOLATION_COST;

        const int64_t g = (int64_t)e * pp.P + c0 + tid;
        if (valid && pp.perf_traj) {
#pragma unroll
            for (int i = 0; i < NS; ++i) pp.perf_traj[(g * T + t) * NS + i] = mu1[i];
        }
        if (valid && cp.sigma) {
#pragma unroll
            for (int i = 0; i < NS; ++i) cp.sigma[(g * T + t) * NS + i] = G[i];
        }
        if (valid && cp.cov) {
            double* cv = cp.cov + (g * T + t) * (NS * NS);
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) cv[i * NS + j] = S1[i][j];
        }
        if (valid && cp.margins) {
            cp.margins[(g * T + t) * 2 + 0] = smax_d;
            cp.margins[(g * T + t) * 2 + 1] = umax_d;
        }
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) S[i][j] = S1[i][j];
#pragma unroll
        for (int i = 0; i < NS; ++i) mu[i] = mu1[i];
    };

    int q_begin, q_end;   // this wave's share of the Kstar pairs: all waves alike
    kstar_pair_range(gc.n_pad >> 3, wave, 1, nw, q_begin, q_end);
    for (int t = 0; t < T; ++t) {
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
                for (int cidx = 0; cidx < NU; ++cidx) zq[NS + cidx] = acts[(c * T + t) * NU + cidx];
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
        pp.con_cost[g] = con;
        if (st) atomicOr(pp.status + (MM ? e : 0), st);
    }
}

}  // namespace sx
