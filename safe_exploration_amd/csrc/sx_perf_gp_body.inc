// The body of the four GP-product performance kernels, included as text: cem_perf_var_rollout[_multi]_kernel
// (sx_perf_var.hpp) with SX_PERF_TAYLOR 0 and cem_perf_taylor_rollout[_multi]_kernel (sx_perf_taylor.hpp) with
// SX_PERF_TAYLOR 1.  As text and with the kind's sections picked by the preprocessor, so that every kernel sees the
// statements it had when each kernel had a body of its own and compiles to the same instructions (a device function for
// the shared part changed the single-model kernel's registers; tools/device_code_diff.py is the check).
// In scope: NS, NU, BYOUT; MM (false | true: a GP per problem); `gc` (the GpConst kernel argument, or the problem's entry
// of the device table of sx_gp_model_table), `stage_tab` (its stage table); the step constants and the pointers, which
// are kernel arguments in both modes (there is one sx_env): `sc`, `vp` for the variance kernels, `tc_arg`, `tp` for the
// Taylor kernels.
// MM = true: the LDS carve-up follows the problem's n_train / n_pad inside the launch's allocation for the largest model,
// and the status is one word per problem.  The workgroups are problem-aligned in both modes.
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
#if SX_PERF_TAYLOR
    // Taylor: the step constants sit in LDS behind the actions, copied in one pass (`sc` is the variance kernels' argument)
    constexpr int kConst = perf_taylor_const_doubles<NS, NU>();
    static_assert(kConst <= kPerfVarThreads, "one pass copies the step constants");
    static_assert(sizeof(PerfTaylorConst<NS, NU>) % sizeof(double) == 0, "doubles only");
    double* const tcl = acts + SX_TILE * n_perf * NU;
    const PerfTaylorConst<NS, NU>& tc = *reinterpret_cast<const PerfTaylorConst<NS, NU>*>(tcl);
    const PerfStepConst<NS, NU>& sc = tc.step;
    if (tid < kConst) tcl[tid] = reinterpret_cast<const double*>(&tc_arg)[tid];
#endif

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
#if SX_PERF_TAYLOR
    double S[NS][NS];   // Taylor: Sigma_t beside mu_t on the owner lane, both triangles; Sigma_0 = 0
    if (owner) {
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) S[i][j] = 0.0;
    }
#endif
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
        gp_collect<NS, D, SX_PERF_TAYLOR>(gc, lds, nw, tid, z, mean, var, jac);   // Taylor: with the Jacobian rows
        next_centre(tid, z, mu1);   // exactly the centre the Kstar threads of step t + 1 derive
        if (t + 1 < n_perf) {
            double* zn = zs_base + ((t + 1) & 1) * 16 * D + tid * D;
#pragma unroll
            for (int i = 0; i < NS; ++i) zn[i] = mu1[i];
#pragma unroll
            for (int cidx = 0; cidx < NU; ++cidx) zn[NS + cidx] = acts[(tid * n_perf + t + 1) * NU + cidx];
        }
#if SX_PERF_TAYLOR
        // Taylor: G = diag(var) + diag(M Sigma M^T) and Sigma_{t+1} = Hm Sigma Hm^T + diag(var) (upper triangle, then
        // mirrored), with M = J_x + J_u K, Hm = (a + b K) + M; MS = M Sigma, HS = Hm Sigma
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
#else
        const double (&G)[NS] = var;   // what the objective and perf_sigma see
        bool bad = false;
#pragma unroll
        for (int i = 0; i < NS; ++i)
            bad = bad || !(__builtin_fabs(mu1[i]) <= 1.7976931348623157e308) ||
                  !(__builtin_fabs(var[i]) <= 1.7976931348623157e308);
#endif
        double o = 0.0;
        if (vp.obj_mode == SX_OBJ_NEG_VARIANCE) {
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
#if SX_PERF_TAYLOR
        if (t == tp.safety_step) {
            // Taylor: the terminal-safety coupling: (mu_s, Sigma_s), s = t + 1 = H + 2, inside the safe polytope
            if (polytope_violated<SX_MAX_M, NS>(tc.h_mat, tc.h_vec, tp.m, 1.0, mu1, S1, nullptr))
                con += SX_STATE_VIOLATION_COST;
        }
#endif
        const int64_t g = (int64_t)e * pp.P + c0 + tid;
        if (valid && pp.perf_traj) {
#pragma unroll
            for (int i = 0; i < NS; ++i) pp.perf_traj[(g * n_perf + t) * NS + i] = mu1[i];
        }
        if (valid && vp.perf_sigma) {
#pragma unroll
            for (int i = 0; i < NS; ++i) vp.perf_sigma[(g * n_perf + t) * NS + i] = G[i];
        }
#if SX_PERF_TAYLOR
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
#endif
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
