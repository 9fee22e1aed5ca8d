// The body of cem_perf_rollout_kernel and cem_perf_rollout_multi_kernel (sx_perf.hpp), included into both: as text, so that
// the single-model kernel compiles to the instructions it had before the multi-model one existed (a shared device function
// changed its register allocation).  In scope: NS, NU; MM (false | true: a GP per problem); `pc` with the GP part
// (k_nh_ils2, k_log_os, x_train, alpha, n_train, n_pad) -- the kernel argument, or the problem's entry of the device table --;
// `step`, the PerfStepConst kernel argument; `pp`.
// MM = true: the grid is problem-aligned, E x ceil(P / kPerfTile) workgroups, so that a workgroup stages ONE problem's
// training inputs and alpha with that problem's n_pad inside the launch's allocation for the largest model; a slot past P
// in a problem's last tile computes on the problem's first particle and writes nothing; pp.status holds E words.
    constexpr int D = NS + NU;
    extern __shared__ __attribute__((aligned(16))) double perf_lds[];
    const int n_pad = pc.n_pad;
    double* xs = perf_lds;                // [D][n_pad]
    double* al = xs + (size_t)D * n_pad;  // [NS][n_pad]
    double* etab = al + (size_t)NS * n_pad;
    for (int idx = threadIdx.x; idx < n_pad * D; idx += kPerfThreads) {
        const int i = idx / D, c = idx - i * D;
        xs[c * n_pad + i] = i < pc.n_train ? pc.x_train[idx] : 0.0;
    }
    for (int idx = threadIdx.x; idx < n_pad * NS; idx += kPerfThreads) {
        const int d = idx / n_pad, i = idx - d * n_pad;
        al[idx] = i < pc.n_train ? pc.alpha[(size_t)d * pc.n_train + i] : 0.0;
    }
    if (threadIdx.x < kExpTab) etab[threadIdx.x] = kExp2Tab[threadIdx.x];
    constexpr int kStepDoubles = (int)(sizeof(PerfStepConst<NS, NU>) / sizeof(double));
    static_assert(kStepDoubles <= kPerfThreads, "one thread per constant");
    if (threadIdx.x < kStepDoubles) etab[kExpTab + threadIdx.x] = reinterpret_cast<const double*>(&step)[threadIdx.x];
    __syncthreads();
    typedef __attribute__((address_space(3))) const PerfStepConst<NS, NU> LdsStep;
    LdsStep& sc = *(LdsStep*)(etab + kExpTab);

    const int sub = (int)threadIdx.x & (kPerfLanes - 1);
    int64_t g, gg;   // the particle of the launch; the one this slot reads through
    bool valid;
    int e;
    if constexpr (MM) {
        const int tiles_per_problem = (pp.P + kPerfTile - 1) / kPerfTile;
        e = (int)blockIdx.x / tiles_per_problem;
        const int c = ((int)blockIdx.x - e * tiles_per_problem) * kPerfTile + ((int)threadIdx.x / kPerfLanes);
        valid = c < pp.P;
        g = (int64_t)e * pp.P + c;
        gg = valid ? g : (int64_t)e * pp.P;   // a slot past P reads through the problem's first particle and writes nothing
    } else {
        const int64_t total = (int64_t)pp.E * pp.P;
        g = (int64_t)blockIdx.x * kPerfTile + ((int)threadIdx.x / kPerfLanes);
        valid = g < total;
        gg = valid ? g : 0;   // a slot past the particles reads through the first one and writes nothing
        e = (int)(gg / pp.P);
    }
    const int H = pp.H, r = pp.r, n_perf = pp.n_perf, T = n_perf - r;
    const int64_t row_len = (int64_t)(H + T) * NU;
    const double* safe = pp.safe_actions + gg * H * NU;
    const double* t_mean = pp.tail_noise ? pp.tail_mean + (int64_t)e * T * NU : nullptr;
    const double* t_std = pp.tail_noise ? pp.tail_std + (int64_t)e * T * NU : nullptr;
    const double* t_noise = pp.tail_noise ? pp.tail_noise + gg * T * NU : nullptr;
    double* row = pp.rows + gg * row_len;

    // the particle's row: the safety actions as the safety rollout wrote them, then the tail
    if (valid) {
        for (int i = sub; i < H * NU; i += kPerfLanes) row[i] = safe[i];
        if (t_noise)
            for (int i = sub; i < T * NU; i += kPerfLanes) row[H * NU + i] = fma(t_std[i], t_noise[i], t_mean[i]);
    }
    // action c of performance step t: shared with the safety trajectory below r, the tail from there (drawn by the
    // same expression as the stored one, so that no lane waits for another lane's store)
    auto action = [&](int t, int c) -> double {
        if (t < r) return safe[t * NU + c];
        const int i = (t - r) * NU + c;
        return t_noise ? fma(t_std[i], t_noise[i], t_mean[i]) : row[H * NU + i];
    };

    double log_os[NS];
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        log_os[d] = pc.k_log_os[d];
        asm volatile("" : "+v"(log_os[d]));
    }
    double mu[NS], v[NU];
#pragma unroll
    for (int i = 0; i < NS; ++i) mu[i] = pp.x0[(int64_t)e * NS + i];
#pragma unroll
    for (int c = 0; c < NU; ++c) v[c] = action(0, c);
    double obj = 0.0, con = 0.0;
    int st = 0;
    const lds_f64* xl = (const lds_f64*)xs + sub;
    const lds_f64* all = (const lds_f64*)al + sub;
    const lds_f64* el = (const lds_f64*)etab;
    const int trips = n_pad / kPerfPad;
    for (int t = 0; t < n_perf; ++t) {
        double vn[NU];   // the next step's action travels while this step's sum runs
#pragma unroll
        for (int c = 0; c < NU; ++c) vn[c] = t + 1 < n_perf ? action(t + 1, c) : 0.0;
        double z[D], acc[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) z[j] = mu[j];
#pragma unroll
        for (int c = 0; c < NU; ++c) z[NS + c] = v[c];
#pragma unroll
        for (int d = 0; d < NS; ++d) acc[d] = 0.0;
        // the operands of trip k + 1 are read while trip k's exponentials run (one wave per SIMD at P = 4096: nobody
        // else hides the LDS latency); the read behind the last trip wraps to the first rows
        double xr[kPerfUnroll][D], ar[kPerfUnroll][NS];
        perf_load_trip<NS, D>(xl, all, n_pad, 0, xr, ar);
        for (int k = 0; k < trips; ++k) {
            double xc[kPerfUnroll][D], ac[kPerfUnroll][NS];
#pragma unroll
            for (int h = 0; h < kPerfUnroll; ++h) {
#pragma unroll
                for (int j = 0; j < D; ++j) xc[h][j] = xr[h][j];
#pragma unroll
                for (int d = 0; d < NS; ++d) ac[h][d] = ar[h][d];
            }
            perf_load_trip<NS, D>(xl, all, n_pad, k + 1 < trips ? (k + 1) * kPerfPad : 0, xr, ar);
            double arg[kPerfUnroll * NS], val[kPerfUnroll * NS];
#pragma unroll
            for (int h = 0; h < kPerfUnroll; ++h) {
                double sq[D];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const double df = z[j] - xc[h][j];
                    sq[j] = df * df;
                }
#pragma unroll
                for (int d = 0; d < NS; ++d) {
                    double a = log_os[d];
#pragma unroll
                    for (int j = 0; j < D; ++j) a = fma(sq[j], pc.k_nh_ils2[d * D + j], a);
                    arg[h * NS + d] = a;
                }
            }
            exp_tab_f64_n<kPerfUnroll * NS>(arg, val, el);
#pragma unroll
            for (int h = 0; h < kPerfUnroll; ++h)
#pragma unroll
                for (int d = 0; d < NS; ++d) acc[d] = fma(val[h * NS + d], ac[h][d], acc[d]);
        }
        // the 16 partial sums of the particle: xor butterfly, every lane ends with the same bits
#pragma unroll
        for (int d = 0; d < NS; ++d)
#pragma unroll
            for (int m = kPerfLanes / 2; m > 0; m >>= 1) acc[d] += __shfl_xor(acc[d], m, kPerfLanes);
        double mu1[NS];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double s = acc[i];
#pragma unroll
            for (int j = 0; j < NS; ++j) s += sc.a[i * NS + j] * mu[j];
#pragma unroll
            for (int c = 0; c < NU; ++c) s += sc.b[i * NU + c] * v[c];
            mu1[i] = s;
            bad = bad || !(__builtin_fabs(s) <= 1.7976931348623157e308);
        }
        if (bad) {
            // (the table exponential drops a NaN argument: a non-finite state stays one by hand)
            st |= SX_STATUS_NAN;
#pragma unroll
            for (int i = 0; i < NS; ++i) mu1[i] = __builtin_nan("");
        }
        double o = 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) o += sc.w_abs[i] * fabs(sc.target[i] - mu1[i]) + sc.w_lin[i] * mu1[i];
        obj += o;
        if (t >= r) {
            bool uviol = false;
#pragma unroll
            for (int c = 0; c < NU; ++c) uviol = uviol || (v[c] < sc.u_min[c]) || (v[c] > sc.u_max[c]);
            if (uviol) con += SX_ACTION_VIOLATION_COST;
        }
        if (valid && sub == 0 && pp.perf_traj) {
#pragma unroll
            for (int i = 0; i < NS; ++i) pp.perf_traj[(g * n_perf + t) * NS + i] = mu1[i];
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) mu[i] = mu1[i];
#pragma unroll
        for (int c = 0; c < NU; ++c) v[c] = vn[c];
    }
    if (valid && sub == 0) {
        pp.obj_cost[g] = obj;
        pp.con_cost[g] += con;
        if (st) atomicOr(pp.status + (MM ? e : 0), st);
    }
