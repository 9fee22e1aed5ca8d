/*
 * sx_amd.h -- C ABI of libsxamd.so, the MI355X (gfx950) implementation of the CEM safe-MPC hot path of
 * oscarkey/safe-exploration.
 *
 * The reference has no FFI: its boundary is two Python ABCs and one factory branch.  This header is
 * the boundary a maintainer binds with ctypes (INTEGRATION.md shows the stub).  Each entry point names the reference
 * interface it replaces; paths are relative to the reference root.
 *
 * Conventions
 *   - every pointer marked "dev" is a device pointer into HBM, row-major, contiguous, float64 unless noted;
 *     the library borrows it for the duration of the call's kernels and allocates nothing persistent;
 *   - structs are passed by pointer to HOST memory and copied into kernel arguments;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued on it, nothing is
 *     synchronised, the calls are re-entrant per stream;
 *   - return value: SX_OK or an SX_ERR_* code (bad shape, unsupported dimension, HIP launch error);
 *   - numerical trouble is reported through a device status word (SX_STATUS_* bits), read by the host once per solve
 *     and mapped onto the reference's ValueError (safe_exploration/gp_reachability_pytorch.py:76-80,117-121,149-153).
 */
#ifndef SX_AMD_H
#define SX_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SX_MAX_NS 4              /* state dimension: pendulum 2, cart-pole 4 */
#define SX_MAX_NU 2
#define SX_MAX_D (SX_MAX_NS + SX_MAX_NU)
#define SX_MAX_M 16              /* polytope rows: pendulum 4, cart-pole 9 */
#define SX_TILE 16               /* particles per workgroup = one f64 MFMA tile column block */

#define SX_OK 0
#define SX_ERR_ARG 1             /* null pointer / non-positive size / inconsistent shapes */
#define SX_ERR_UNSUPPORTED 2     /* (n_s, n_u) not instantiated, m > SX_MAX_M, n_train too large for the fused path */
#define SX_ERR_LAUNCH 3          /* HIP reported an error on launch */

#define SX_STATUS_NAN 1          /* _fix_zeros_nans saw a NaN: gp_reachability_pytorch.py:234-236 */
#define SX_STATUS_ZERO_FIX 2     /* an exact zero was replaced by 1e-5: gp_reachability_pytorch.py:238-241 */
#define SX_STATUS_UB_NONPOS 4    /* ellipsoid_from_rectangle got u_b <= 0: utils_ellipsoid.py:304 */

#define SX_OBJ_NEG_VARIANCE 0    /* -sum_d sigma_d: safempc_cem.py:308-311 */
#define SX_OBJ_AFFINE_ABS 1      /* sum_j w_abs_j |target_j - p_j| + w_lin_j p_j: environments.py:505-510, lunarlander.py:111-113 */
#define SX_CON_TERMINAL 0        /* EllipsoidTerminalConstraint: safempc_cem.py:102-113 */
#define SX_CON_ALL_STATES 1      /* EllipsoidStateConstraint on every prefix: safempc_cem.py:116-132 */

#define SX_ACTION_VIOLATION_COST 3.0  /* test_safempc_cem.py:59-71 */
#define SX_STATE_VIOLATION_COST 10.0  /* safempc_cem.py:132 */

/* Exact multi-output GP in the form the kernels consume.
 * Replaces: the gpytorch model behind GpCemSSM (ssm_cem/gp_ssm_cem.py:33-57, ssm_pytorch/gaussian_process.py:82-140).
 * Built by sx_gp_pack() from the inverse Cholesky factors W_d = chol(K_d + noise_d I)^-1 and alpha_d. */
typedef struct sx_gp_model {
    int32_t n_s, n_u;            /* outputs, action dims; D = n_s + n_u inputs */
    int32_t n_train;             /* N */
    int32_t n_pad;               /* 16 * ceil((N + 1 + D) / 16): W_d padded, with room for the mean/Jacobian rows */
    double inv_ls2[SX_MAX_NS * SX_MAX_D];  /* [n_s x D] 1 / lengthscale^2 (ARD, per output) */
    double outputscale[SX_MAX_NS];
    double noise[SX_MAX_NS];     /* likelihood noise, added to the predictive variance (gp_ssm_cem.py:93) */
    const double* x_train;       /* dev [N x D] */
    const double* a_pack;        /* dev, sx_gp_pack_sizes() doubles: W_d with the rows alpha_d, alpha_d * X_j / l_dj^2
                                    appended, in MFMA fragment order */
    const int32_t* stage_tab;    /* dev, sx_gp_pack_sizes() int32: the static MFMA operand stream of every wave */
} sx_gp_model;

/* Environment / solver constants of one MPC problem.
 * Replaces: the attributes CemSafeMPC reads from env/conf (safempc_cem.py:166-196) and the constraint objects
 * (safempc_cem.py:135-146). */
typedef struct sx_env {
    int32_t n_s, n_u;
    int32_t m;                   /* polytope rows */
    int32_t obj_mode;            /* SX_OBJ_* */
    int32_t con_mode;            /* SX_CON_* */
    int32_t reserved;
    double beta;                 /* c_safety */
    double a[SX_MAX_NS * SX_MAX_NS];      /* linear prior A (zeros if no prior: safempc_cem.py:291-296) */
    double b[SX_MAX_NS * SX_MAX_NU];
    double k_fb[SX_MAX_NU * SX_MAX_NS];   /* LQR feedback (safempc_simple.py:1105-1129) */
    double l_mu[SX_MAX_NS];
    double l_sigma[SX_MAX_NS];
    double h_mat[SX_MAX_M * SX_MAX_NS];   /* safe polytope h_mat x <= h_vec */
    double h_vec[SX_MAX_M];
    double u_min[SX_MAX_NU];
    double u_max[SX_MAX_NU];
    double obj_w_abs[SX_MAX_NS];
    double obj_target[SX_MAX_NS];
    double obj_w_lin[SX_MAX_NS];
} sx_env;

/* Library / build identification: returns "sxamd <version> gfx950". */
const char* sx_version(void);

/* ---- exact GPs with a degenerate kernel: 'linear' and 'nn' of ssm_cem/gp_ssm_cem.py:45-57,140-185 ----
 * k_d(x, x') = c_d phi(x) . phi(x'), phi = identity (linear kernel) or a small fully connected network with the reference's
 * per-point min/max normalisation (NNFeatureKernel).  Such a GP is Bayesian linear regression on F features: the kernels
 * below work in weight space (A_d = Phi^T Phi + noise_d / c_d I, F x F), one particle per lane, no N x N operand. */
#define SX_FEAT_MAX_WIDTH 32     /* widest layer / feature count F */
#define SX_FEAT_MAX_LAYERS 3     /* linear layers of the feature network (0 = linear kernel) */
typedef struct sx_feat_model {
    int32_t n_s, n_u;
    int32_t n_feat;              /* F: D for the linear kernel, the last layer's width otherwise */
    int32_t n_layers;            /* 0 = phi(z) = z */
    int32_t normalise;           /* 1 = phi = 2 (f - min f) / max f - 1 per point (gp_ssm_cem.py:176-181) */
    int32_t width[SX_FEAT_MAX_LAYERS + 1];   /* width[0] = D, width[l] = outputs of layer l */
    double prelu;                /* slope of the PReLU behind the last layer (ReLU between the layers) */
    double noise[SX_MAX_NS];     /* likelihood noise, included in the predictive variance */
    const double* net;           /* dev: per layer W_l [width[l] x width[l-1]] row-major, then b_l [width[l]] */
    const double* wbar;          /* dev [n_s x F]      posterior weight means (sx_feat_fit) */
    const double* minv;          /* dev [n_s x F x F]  M_d = chol(A_d)^-1, lower triangular (sx_feat_fit) */
} sx_feat_model;

/* phi dev [N x F] = phi(x dev [N x D]).  Uses model->{n_s,n_u,n_feat,n_layers,normalise,width,prelu,net}. */
int sx_feat_features(const sx_feat_model* model, const double* x, int N, double* phi, void* stream);
/* Weight-space fit from phi dev [N x F], y dev [N x n_s], lambda host [n_s] = noise_d / c_d:
 * wbar dev [n_s x F], minv dev [n_s x F x F], stats dev [n_s x 3] = { y^T y, |M Phi^T y|^2, sum log diag chol(A) } (what the
 * exact marginal likelihood needs), status dev int32 (SX_STATUS_NOT_PD).
 * Replaces: gpytorch's ExactGP on set_train_data for these kernels (ssm_cem/gp_ssm_cem.py:96-101). */
int sx_feat_fit(const sx_feat_model* model, const double* phi, const double* y, int N, const double* lambda, double* wbar,
                double* minv, double* stats, int32_t* status, void* stream);
/* Posterior at z dev [P x D]: same outputs as sx_gp_predict.  Replaces GpCemSSM.predict_* for these kernels. */
int sx_feat_predict(const sx_feat_model* model, const double* z, int P, double* mean, double* var, double* jac, void* stream);
/* The CEM particle rollout over such a GP: same arguments and outputs as sx_cem_rollout (no workspace). */
int sx_cem_rollout_feat(const sx_feat_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                        const double* mean, const double* std, const double* noise, double* actions, double* traj,
                        double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream);

/* sx_cem_rollout_feat for a JunkDimensionsSSM over such a GP: as sx_cem_rollout_junk for the exact RBF GP.  The junk
 * columns reach the features only through the network's first layer (phi = z for the linear kernel), so the padded GP's
 * real outputs are those of the GP over the D = n_s + n_u + s kept columns (training rows [x, u, 0_s], queries [x, 0_s, u],
 * s = query_shift = min(J_s, n_u)); for the linear kernel A_d splits into a kept and a junk block and the kept block is the
 * fit on the kept features with the same lambda_d.  `model` is that GP (model->n_s == env->n_s, model->n_u == env->n_u +
 * query_shift, fitted by sx_feat_fit on the kept columns); `env` and every buffer are shaped by (n_s, n_u) as in
 * sx_cem_rollout_feat; the reachability step receives the Jacobian's leading n_s + n_u columns.
 *   query_shift 0 .. env->n_u; 0 is sx_cem_rollout_feat itself.
 * SX_ERR_ARG (before any device access) for null pointers, non-positive sizes, inconsistent shapes or a shift outside that
 * range; SX_ERR_UNSUPPORTED for a shape that is not instantiated: (n_s, n_u, s) in (1,1,1) (2,1,1) (3,1,1) (2,2,1) (2,2,2)
 * (3,2,1), the shapes a padded model with n_s + J_s <= SX_MAX_NS and n_u + J_a <= SX_MAX_NU has.
 * sx_feat_features and sx_feat_fit take that model too (any n_u with n_s + n_u <= SX_MAX_D); sx_feat_predict does not. */
int sx_cem_rollout_feat_junk(const sx_feat_model* model, const sx_env* env, int query_shift, int E, int P, int H,
                             const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                             double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                             int32_t* status, void* stream);

/* ---- MC-dropout state-space models: ssm_cem/dropout_ssm_cem.py, gal_concrete_dropout.py ----
 * An ensemble of S thinned ReLU networks: dropout masks drawn once per (re)training and held fixed, prediction = mean and
 * unbiased variance over the members, mean Jacobian by reverse sweeps.  One or two hidden layers of <= 64 units run on the
 * f64 matrix cores (csrc/sx_mlp_mfma.hpp: a 16-particle tile per workgroup, a member per wave, activations in registers);
 * other shapes one particle per lane (csrc/sx_mlp.hpp).  SX_MLP_PATH=valu in the environment forces the latter (A/B runs). */
#define SX_MLP_MAX_HIDDEN 4      /* hidden layers */
#define SX_MLP_MAX_WIDTH 64      /* hidden units per layer (the reference's default network is 64 x 64) */
typedef struct sx_mlp_model {
    int32_t n_s, n_u;
    int32_t n_hidden;            /* L */
    int32_t n_out;               /* rows of the output layer (>= n_s; the first n_s are the predicted means) */
    int32_t n_samples;           /* S ensemble members (mc_dropout_num_samples) */
    int32_t predict_std;         /* 1: outputs n_s .. 2 n_s - 1 are log standard deviations; the variance gains the members'
                                    mean exp(2 log std): the expectation of dropout_ssm_cem.py:106-109 over its fresh noise */
    int32_t width[SX_MLP_MAX_HIDDEN + 1];   /* width[0] = D, width[l] = hidden layer l */
    const double* net;           /* dev: W_1 [w1 x D] row-major, b_1, ..., W_L, b_L, W_out [n_out x w_L], b_out */
    const double* masks;         /* dev [S x (width[0] + ... + width[L])]: the multipliers of the input and of every hidden
                                    layer's activations (0 or 1 / keep for Bernoulli dropout, relaxed values for concrete) */
} sx_mlp_model;
/* Posterior at z dev [P x D]: same outputs as sx_gp_predict.  Replaces McDropoutSSM / GalConcreteDropoutSSM.predict_*
 * (dropout_ssm_cem.py:79-112, gal_concrete_dropout.py:164-196). */
int sx_mlp_predict(const sx_mlp_model* model, const double* z, int P, double* mean, double* var, double* jac, void* stream);
/* The CEM particle rollout over the ensemble: same arguments and outputs as sx_cem_rollout (no workspace). */
int sx_cem_rollout_mlp(const sx_mlp_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                       const double* mean, const double* std, const double* noise, double* actions, double* traj,
                       double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream);

/* sx_cem_rollout_mlp for a JunkDimensionsSSM over an MC-dropout model, as sx_cem_rollout_feat_junk: the junk columns reach
 * the network only through its first layer, so `model` is the ensemble over the D = n_s + n_u + query_shift kept columns
 * (first-layer weight columns and input-mask columns of those), with the mean rows [0, n_s) of the output layer and, with
 * predict_std, the log-std rows [n_s + J_s, n_s + J_s + n_s) as rows [n_s, 2 n_s).  Same checks and shapes as
 * sx_cem_rollout_feat_junk; query_shift 0 is sx_cem_rollout_mlp itself; SX_MLP_PATH=valu applies as there. */
int sx_cem_rollout_mlp_junk(const sx_mlp_model* model, const sx_env* env, int query_shift, int E, int P, int H,
                            const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                            double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                            int32_t* status, void* stream);

/* Optional kernel timer -- measurement support, not part of the reference's surface (it has no profiler: SURVEY.md 5).
 * While enabled, the launches of the path's kernels (every `sx_profile_stride`-th of each kind) carry a start and a stop HIP
 * event on the stream the kernel is launched on (hipExtLaunchKernelGGL: the dispatch's own begin / end timestamps, the
 * interval rocprofv3's kernel trace reports; SX_PROF_RECORD=1 in the environment: two hipEventRecord around the launch, as
 * in rounds 1-2, which read ~2.8 us more).  At most `max_launches` launches are recorded; sx_profile_collect synchronises
 * those events and returns the summed elapsed time and the launch count of one kernel class.  bench.py's
 * `roofline.avg_launch_us` comes from here. */
#define SX_PROF_ROLLOUT_FUSED 0  /* cem_rollout_kernel            */
#define SX_PROF_RANK 1           /* cem_rank_kernel               */
#define SX_PROF_KSTAR_BIG 2      /* kstar_big_kernel   (large-N path) */
#define SX_PROF_TRMM_BIG 3       /* trmm_reduce_kernel (large-N path) */
#define SX_PROF_STEP_BIG 4       /* step_big_kernel    (large-N path) */
#define SX_PROF_ROLLOUT_FEAT 5   /* cem_rollout_feat_kernel (degenerate-kernel GPs) */
#define SX_PROF_ROLLOUT_MLP 6    /* cem_rollout_mlp_mfma_kernel / cem_rollout_mlp_kernel (MC-dropout ensembles) */
#define SX_PROF_KINDS 7
int sx_profile_enable(int max_launches);
int sx_profile_stride(int every);   /* time every n-th launch of a kernel class only (default 1): a timed launch costs the
                                       launch path a few microseconds, which a 130 us kernel notices */
int sx_profile_stride_kind(int kind, int every);   /* the same for one kernel class */
int sx_profile_collect(int kind, double* total_ms, int64_t* launches);
int sx_profile_disable(void);

#ifndef SX_WAVES
#define SX_WAVES 8               /* waves per workgroup in the GP kernels (the stage table is laid out for it) */
#endif

/* Sizes of sx_gp_model.a_pack (doubles) and sx_gp_model.stage_tab (int32).
 * sx_gp_pack_sizes, sx_gp_fit and sx_gp_pack take any n_u with n_s + n_u <= SX_MAX_D: beyond SX_MAX_NU that is the
 * widened GP of sx_cem_rollout_junk (n_u = real actions + query shift), which only that entry point consumes. */
int sx_gp_pack_sizes(int n_s, int n_u, int n_train, int64_t* a_doubles, int64_t* tab_ints);

#define SX_STATUS_NOT_PD 8       /* sx_gp_fit: K + noise I is not positive definite (gpytorch would raise too) */

/* Exact-GP fit for fixed hyper-parameters: K_d + noise_d I = L_d L_d^T, linv = L_d^-1 (dev [n_s x N x N]),
 * alpha_d = (K_d + noise_d I)^-1 y_d (dev [n_s x N]), logdet_d = sum log diag L_d (dev [n_s]).
 * model->{n_s,n_u,n_train,inv_ls2,outputscale,noise,x_train} must be set; y_train dev [N x n_s];
 * work dev [n_s x N x N] scratch (holds L on return); status dev int32 (SX_STATUS_NOT_PD).  N <= 4096.
 * Replaces: what gpytorch's ExactGP computes when GpCemSSM sets new training data
 * (ssm_cem/gp_ssm_cem.py:96-101, ssm_pytorch/gaussian_process.py:82-140). */
int sx_gp_fit(const sx_gp_model* model, const double* y_train, double* work, double* linv, double* alpha,
              double* logdet, int32_t* status, void* stream);

/* Exact marginal log likelihood per output and its gradient w.r.t. the hyper-parameters, from sx_gp_fit's outputs:
 * mll dev [n_s]; grad dev [n_s x (D + 2)] = d mll_d / d (lengthscale_d[0..D), outputscale_d, noise_d).
 * work dev [n_s x N x N]: scratch, overwritten (sx_gp_fit's `work` may be passed: L is not needed any more).
 * Replaces: the autograd pass of GpCemSSM._train_model (ssm_cem/gp_ssm_cem.py:103-129,
 * gpytorch.ExactMarginalLogLikelihood); the Adam update itself stays on the host. */
int sx_gp_mll_grad(const sx_gp_model* model, const double* y_train, const double* linv, const double* alpha,
                   const double* logdet, double* work, double* mll, double* grad, void* stream);

/* ---- k <= 64 rows appended to a fitted exact GP without refactorising the old ones ----
 * model->{n_s,n_u,n_train,inv_ls2,outputscale,noise,x_train} set as for sx_gp_fit with n_train = N + k and x_train dev
 * [(N + k) x D], whose first n_old = N rows are the fitted ones; y_train dev [(N + k) x n_s]; linv_old dev [n_s x N x N],
 * alpha_old dev [n_s x N] and logdet_old dev [n_s] as sx_gp_fit (or this entry) wrote them for those N rows and these
 * hyper-parameters.  Per output, with K_c = k(X, X_c), K_cc = k(X_c, X_c) + noise I and B = W K_c:
 *     S = K_cc - B^T B = L_s L_s^T,  W_s = L_s^-1,  new rows of W: [ -W_s B^T W | W_s ],  old rows: W with k zeros appended,
 *     alpha' = [alpha; 0] + W_bot^T (W_bot y'),  logdet' = logdet + sum log diag L_s.
 * linv dev [n_s x (N + k) x (N + k)], alpha dev [n_s x (N + k)] and logdet dev [n_s] get exactly the layout sx_gp_fit leaves
 * for N + k rows (zeros above the diagonal included), so sx_gp_pack, sx_gp_mll_grad, sx_gp_predict_var_jac and a further
 * sx_gp_append take them unchanged; the old rows of linv are linv_old's bit for bit.  The old and the new buffers must be
 * DISTINCT (the row stride changes).  status dev int32, or-ed into: SX_STATUS_NOT_PD where a pivot of S is not > 0 (NaN
 * included); the outputs are then unspecified.  workspace dev, sx_gp_append_workspace_bytes(n_s, N + k, k) bytes.  Six
 * launches on `stream`, O(N^2 k) work, every sum in an order that depends on N and k only; nothing is waited for.
 * SX_ERR_ARG (before any device access) for a null pointer, a shape sx_gp_fit refuses, n_old < 1, n_train - n_old outside
 * 1 .. 64 or a workspace that is too small; SX_ERR_UNSUPPORTED for n_train > 4096.
 * Replaces: the refit gpytorch's ExactGP runs when GpCemSSM gets new training data (ssm_cem/gp_ssm_cem.py:96-101), where
 * the new data extend the old and the hyper-parameters have not changed: exploration_runner adds one pair per iteration
 * (exploration_runner.py), episode_runner one episode's rows.
 *
 * Bytes of the workspace; < 0 for n_s outside 1 .. SX_MAX_NS, k outside 1 .. 64, n_train - k < 1 or n_train > 4096. */
int64_t sx_gp_append_workspace_bytes(int n_s, int n_train, int k);
int sx_gp_append(const sx_gp_model* model, int n_old, const double* y_train, const double* linv_old, const double* alpha_old,
                 const double* logdet_old, double* linv, double* alpha, double* logdet, int32_t* status,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The k <= 64 oldest rows removed from a fitted exact GP without refactorising the kept ones ----
 * linv_old dev [n_s x N x N] as sx_gp_fit (or sx_gp_append, or this entry) wrote it for N = n_old rows; the first k rows are
 * dropped and m = N - k are kept; y_train dev [m x n_s], the KEPT rows' targets.  No hyper-parameters and no training
 * inputs are needed.  Per output, with W = linv_old partitioned after the first k rows and columns, W = [ W11 0 ; W21 W22 ]:
 *     K22 = L22 L22^T + L21 L21^T (a rank-k update, positive sign),  L11 = W11^-1,  V = L22^-1 L21 = -W21 L11 [m x k],
 *     W' = chol(I + V V^T)^-1 W22,  alpha' = W'^T (W' y),  logdet' = -sum log diag W',
 * chol(I + V V^T)^-1 applied as k rank-1 stages in one pass over the rows, to every column of W22 independently.
 * linv dev [n_s x m x m], alpha dev [n_s x m] and logdet dev [n_s] get exactly the layout sx_gp_fit leaves for m rows (zeros
 * above the diagonal included), so sx_gp_pack, sx_gp_mll_grad, sx_gp_predict_var_jac, sx_gp_append and a further sx_gp_drop
 * take them unchanged.  The old and the new buffers must be DISTINCT (the row stride changes); the inputs are not written.
 * status dev int32, or-ed into: SX_STATUS_NOT_PD where a diagonal element of W11 or of W' is not > 0, an element of W11 or
 * a stage's t + u^2 is not finite, or a NaN appears; the outputs are then unspecified.  workspace dev,
 * sx_gp_drop_workspace_bytes(n_s, n_old, k) bytes.  Seven launches on `stream`, O(N^2 k) work, every sum in an order that
 * depends on N and k only, no atomics on doubles; nothing is waited for.
 * SX_ERR_ARG (before any device access) for a null pointer, n_s outside 1 .. SX_MAX_NS, k outside 1 .. 64, n_old - k < 1 or
 * a workspace that is too small; SX_ERR_UNSUPPORTED for n_old > 4096.
 * Replaces: the refit of a GpCemSSM that keeps its most recent rows (conf.cem_gp_window), together with sx_gp_append.
 *
 * Bytes of the workspace; < 0 for n_s outside 1 .. SX_MAX_NS, k outside 1 .. 64, n_old - k < 1 or n_old > 4096. */
int64_t sx_gp_drop_workspace_bytes(int n_s, int n_old, int k);
int sx_gp_drop(int n_s, int n_old, int k, const double* y_train, const double* linv_old, double* linv, double* alpha,
               double* logdet, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Lockstep appends: k rows appended to each of E fitted exact GPs in one launch sequence ----
 * Every problem e has its own fitted rows (its own N_e) and hyper-parameters; all share (n_s, n_u) and k.  Problem e's linv,
 * alpha and logdet are those of sx_gp_append for model e alone, BIT FOR BIT: they are independent of which other problems
 * share the call and of their order.  The per-problem constants and buffers live in a table of SX_GP_APPEND_ENTRY_BYTES
 * per problem, which sx_gp_append_table writes to HOST memory: the caller copies it to the device (from pinned memory that
 * needs no wait) and passes the device copy to sx_gp_append_multi, which reads it and copies nothing from the host.
 *
 * Bytes of the table for E problems (E * SX_GP_APPEND_ENTRY_BYTES); < 0 for E <= 0. */
#define SX_GP_APPEND_ENTRY_BYTES 408
int64_t sx_gp_append_table_bytes(int E);
/* Lays the E models (host array, each set as for sx_gp_append: n_train = N_e + k, x_train dev [(N_e + k) x D] with the fitted
 * rows first) out in `table` (HOST memory, sx_gp_append_table_bytes() bytes) with problem e's device buffers (host arrays of
 * E device pointers, each as the argument of that name of sx_gp_append): y_train[e], linv_old[e], alpha_old[e],
 * logdet_old[e], linv[e], alpha[e], logdet[e]; workspace[e] dev, workspace_bytes[e] >=
 * sx_gp_append_workspace_bytes(n_s, N_e + k, k) (the E workspaces may be cut from one allocation); and the shared status
 * dev int32 [E], one word per problem, or-ed into: SX_STATUS_NOT_PD in word e says that problem e's outputs are
 * unspecified and nothing about the others'.  No device access.
 * SX_ERR_ARG for a null pointer (an element of the pointer arrays included), E <= 0, k outside 1 .. 64, models of different
 * (n_s, n_u), a shape sx_gp_fit refuses, N_e < 1 or a workspace that is too small; SX_ERR_UNSUPPORTED for N_e + k > 4096 or
 * E * n_s > 65535 (a grid's y-extent). */
int sx_gp_append_table(const sx_gp_model* models, int E, int k, const double* const* y_train, const double* const* linv_old,
                       const double* const* alpha_old, const double* const* logdet_old, double* const* linv,
                       double* const* alpha, double* const* logdet, int32_t* status, void* const* workspace,
                       const int64_t* workspace_bytes, void* table);
/* sx_gp_append for the E problems of `table` (dev, the device copy of sx_gp_append_table's output for the same `models` and
 * k): six launches on `stream` for all of them, each sized by the largest N_e; a workgroup beyond its own problem's extent
 * returns at once, and every sum keeps the order that its problem's N_e and k give it.  Nothing is waited for.  The checks
 * of sx_gp_append_table that concern `models`, E and k (before any device access).
 * Replaces: the refits of the n_scenarios GpCemSSM models between two solves of the exploration loop
 * (exploration_runner.py), one new row per scenario. */
int sx_gp_append_multi(const sx_gp_model* models, int E, int k, const void* table, void* stream);

/* ---- Lockstep drops: the k oldest rows removed from each of E fitted exact GPs in one launch sequence ----
 * Every problem e has its own fitted rows (its own N_e = n_old[e]); all share n_s and k.  Problem e's linv, alpha and logdet
 * are those of sx_gp_drop for model e alone, BIT FOR BIT: they are independent of which other problems share the call and
 * of their order.  The per-problem buffers live in a table of SX_GP_DROP_ENTRY_BYTES per problem, which sx_gp_drop_table
 * writes to HOST memory: the caller copies it to the device (from pinned memory that needs no wait) and passes the device
 * copy to sx_gp_drop_multi, which reads it and copies nothing from the host.
 *
 * Bytes of the table for E problems (E * SX_GP_DROP_ENTRY_BYTES); < 0 for E <= 0. */
#define SX_GP_DROP_ENTRY_BYTES 104
int64_t sx_gp_drop_table_bytes(int E);
/* Lays the E problems out in `table` (HOST memory, sx_gp_drop_table_bytes() bytes): n_old host [E], the fitted rows N_e, and
 * problem e's device buffers (host arrays of E device pointers, each as the argument of that name of sx_gp_drop):
 * y_train[e] (the m_e = N_e - k KEPT rows' targets), linv_old[e], linv[e], alpha[e], logdet[e]; workspace[e] dev,
 * workspace_bytes[e] >= sx_gp_drop_workspace_bytes(n_s, N_e, k) (the E workspaces may be cut from one allocation); and the
 * shared status dev int32 [E], one word per problem, or-ed into: SX_STATUS_NOT_PD in word e says that problem e's outputs are
 * unspecified and nothing about the others'.  No device access.
 * SX_ERR_ARG for a null pointer (an element of the pointer arrays included), E <= 0, n_s outside 1 .. SX_MAX_NS, k outside
 * 1 .. 64, N_e - k < 1 or a workspace that is too small; SX_ERR_UNSUPPORTED for N_e > 4096 or E * n_s > 65535 (a grid's
 * y-extent). */
int sx_gp_drop_table(int n_s, int E, int k, const int* n_old, const double* const* y_train, const double* const* linv_old,
                     double* const* linv, double* const* alpha, double* const* logdet, int32_t* status,
                     void* const* workspace, const int64_t* workspace_bytes, void* table);
/* sx_gp_drop for the E problems of `table` (dev, the device copy of sx_gp_drop_table's output for the same n_s, k and n_old):
 * seven launches on `stream` for all of them, each sized by the largest m_e; a workgroup beyond its own problem's extent
 * returns before it touches memory, and every sum keeps the order that its problem's N_e and k give it.  Nothing is waited
 * for.  The checks of sx_gp_drop_table that concern n_s, E, k and n_old (before any device access).
 * Replaces: the model-by-model slides of the n_scenarios windowed GpCemSSM models between two solves of the exploration
 * loop (conf.cem_gp_window with conf.cem_gp_incremental_lockstep), together with sx_gp_append_multi. */
int sx_gp_drop_multi(int n_s, int E, int k, const int* n_old, const void* table, void* stream);

/* ---- E exact GPs' fit and MLL gradient in one launch sequence (batched hyper-parameter training) ----
 * Every problem e has its own training set (its own N <= 4096) and hyper-parameters; all share (n_s, n_u).  Problem e's
 * linv, alpha, logdet, mll and gradient are bit-identical to what sx_gp_fit / sx_gp_mll_grad give for that model alone.
 * The per-problem constants and buffers live in a table of SX_GP_FIT_ENTRY_BYTES per problem, which sx_gp_fit_table
 * writes to HOST memory: the caller copies it to the device (from pinned memory that needs no wait) and passes the
 * device copy to the two launchers, which read it and copy nothing from the host.
 *
 * Bytes of the table for E problems (E * SX_GP_FIT_ENTRY_BYTES); < 0 for E <= 0. */
#define SX_GP_FIT_ENTRY_BYTES 360
int64_t sx_gp_fit_table_bytes(int E);
/* Lays the E models (host array: {n_s, n_u, n_train, inv_ls2, outputscale, noise, x_train} set as for sx_gp_fit) out in
 * `table` (HOST memory, sx_gp_fit_table_bytes() bytes) with problem e's device buffers (host arrays of E device
 * pointers): y_train[e] dev [N_e x n_s], work[e] dev [n_s x N_e x N_e] (scratch), linv[e] dev [n_s x N_e x N_e],
 * alpha[e] dev [n_s x N_e], logdet[e] dev [n_s]; and the shared outputs status dev int32 [E] (one word per problem,
 * SX_STATUS_NOT_PD), mll dev [E x n_s], grad dev [E x n_s x (D + 2)].  No device access.
 * SX_ERR_ARG for a null pointer, E <= 0, models of different (n_s, n_u) or n_s + n_u > SX_MAX_D; SX_ERR_UNSUPPORTED for
 * N > 4096. */
int sx_gp_fit_table(const sx_gp_model* models, int E, const double* const* y_train, double* const* work,
                    double* const* linv, double* const* alpha, double* const* logdet, int32_t* status, double* mll,
                    double* grad, void* table);
/* sx_gp_fit for the E problems of `table` (dev, the device copy of sx_gp_fit_table's output for the same `models`): one
 * launch of the one-workgroup kernel for every problem with N <= 96 and one blocked launch sequence, sized by the
 * largest N, for the others.  The argument checks of sx_gp_fit_table (before any device access). */
int sx_gp_fit_multi(const sx_gp_model* models, int E, const void* table, void* stream);
/* sx_gp_mll_grad for the E problems of `table`, after sx_gp_fit_multi: mll and grad into the table's [E x ...] outputs.
 * Replaces: the autograd pass of the n_scenarios GpCemSSM._train_model runs (episode_runner.py:55,123). */
int sx_gp_mll_grad_multi(const sx_gp_model* models, int E, const void* table, void* stream);

/* ---- Max-variance subset of a pool of training inputs (a bounded training set for the exact GP) ----
 * For each of E problems: m of the n_e pool rows models[e].x_train (dev [n_e x D]), chosen greedily.  Per output d the
 * residuals r_d[i] start at s_d + noise_d; step j = 0 .. m-1 takes the pivot p_j = seed_idx[e][j] while j < n_seed, else
 * the unchosen row with the largest sum_d r_d[i] (ties: the LOWEST index, whatever the launch geometry), records
 * idx[e][j] = p_j and sel_var[e][j] = sum_d r_d[p_j] -- the predictive variance of x_p, noise included, given the rows
 * chosen before it, summed over the outputs -- and updates, for every row i,
 *     c = (k_d(x_i, x_p) + noise_d [i = p] - sum_{l<j} C_d[l][i] C_d[l][p]) / sqrt(r_d[p]),   C_d[j][i] = c,   r_d[i] -= c^2
 * with k_d the kernel value sx_gp_fit builds K from: a jointly pivoted Cholesky factorisation of the K_d + noise_d I.
 * If some r_d[p_j] is not > 0 (NaN included), or a seed is out of range or repeated, status[e] gets SX_STATUS_NOT_PD,
 * idx[e][j..m) stays -1 and sel_var[e][j..m) NaN, and the problem's remaining steps do nothing (as they do where the
 * caller passes a status word with that bit set).  The training targets play no part.
 * Replaces: SimpleGPModel.choose_datapoints_maxvar (ssm_gpy/gaussian_process.py:279-344), without its k-means seeds.
 *
 * models: host array of E models with {n_s, n_u, n_train = n_e, inv_ls2, outputscale, noise, x_train} set as for
 * sx_gp_fit_multi; one (n_s, n_u) with n_s + n_u <= SX_MAX_D, the n_e may differ.  seed_idx dev int32 [E x n_seed] or NULL
 * (n_seed = 0); idx dev int32 [E x m]; sel_var dev [E x m]; status dev int32 [E] (or-ed into: the caller zeroes it);
 * workspace dev, sx_gp_select_workspace_bytes(n_s, E, max n_e, m) bytes.  One init launch per 8 problems and one launch
 * per step, all on `stream`; nothing is waited for.  Problem e's results are bit-identical to a call with that problem
 * alone.
 * SX_ERR_ARG (before any device access) for a null pointer, E <= 0, m <= 0, m > n_e, models of different (n_s, n_u),
 * n_seed outside [0, m] or a workspace that is too small; SX_ERR_UNSUPPORTED for m > 4096 (sx_gp_fit's limit),
 * n_e > 65536 or E > 65535.
 *
 * Bytes of the workspace; < 0 for a non-positive size, m > n_max or a size beyond those limits. */
int64_t sx_gp_select_workspace_bytes(int n_s, int E, int n_max, int m);
int sx_gp_select(const sx_gp_model* models, int E, int m, const int32_t* seed_idx, int n_seed, int32_t* idx,
                 double* sel_var, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* Lays W_d = L_d^-1 (dev [n_s x N x N], lower triangular) and alpha (dev [n_s x N]) out in fragment order.
 * model->{n_s,n_u,n_train,inv_ls2,x_train,a_pack,stage_tab} must be set; n_pad is filled in.
 * Replaces: GpCemSSM._update_model (ssm_cem/gp_ssm_cem.py:96-101) -- where the prediction operands are (re)built. */
int sx_gp_pack(sx_gp_model* model, const double* linv, const double* alpha, void* stream);

/* Posterior at z dev [P x D]: mean dev [P x n_s], var dev [P x n_s] (noise included), jac dev [P x n_s x D] or NULL.
 * Replaces: GpCemSSM.predict_with_jacobians / predict_without_jacobians / _predict (ssm_cem/gp_ssm_cem.py:59-94)
 * and compute_jacobian_fast (ssm_pytorch/utilities.py:54-85). */
int sx_gp_predict(const sx_gp_model* model, const double* z, int P, double* mean, double* var, double* jac,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* d var / d z at z dev [P x D]: jac_var dev [P x n_s x D]; `linv` dev [n_s x N x N] as produced by sx_gp_fit for this model.
 * Not on the CEM path: it completes the numpy adapter (StateSpaceModel.predict(..., jacobians=True) returns it as its
 * fourth output).  Replaces: compute_jacobian(pred_var, inp) in GPyTorchSSM._predict
 * (ssm_pytorch/gaussian_process.py:222-231). */
int sx_gp_predict_var_jac(const sx_gp_model* model, const double* linv, const double* z, int P, double* jac_var,
                          void* stream);

/* d^2 mean / dz dz^T at z dev [P x D]: hess dev [P x n_s x D x D] (symmetric); `alpha` dev [n_s x N] as produced by sx_gp_fit.
 * Not on the CEM path: it completes the numpy adapter's linearize_predict / get_linearize_reverse, which the casadi
 * callback of the reference's other solvers consumes (state_space_models.py:279-304).  Replaces:
 * GPyTorchSSM._compute_hessian_mean (ssm_pytorch/gaussian_process.py:160-187, the `hessian` package over autograd). */
int sx_gp_predict_mean_hessian(const sx_gp_model* model, const double* alpha, const double* z, int P, double* hess,
                               void* stream);

/* Bytes of workspace sx_gp_predict needs (0 while the training set fits the single-launch kernel; < 0 = bad arguments). */
int64_t sx_gp_predict_workspace_bytes(const sx_gp_model* model, int P);

/* One-step ellipsoidal reachability given the GP outputs at (p, u).
 * p dev [P x n_s]; Q dev [P x n_s x n_s] or NULL (point branch); u dev [P x n_u]; mean/var dev [P x n_s];
 * jac dev [P x n_s x D] (ignored in the point branch); outputs p1 dev [P x n_s], Q1 dev [P x n_s x n_s],
 * sigma dev [P x n_s] (the variance after the zero fix-up); status dev int32 (OR-ed; bit 16 is used as scratch during
 * the call and is clear on return).
 * The zero fix-up follows the reference's WHOLE-BATCH rule: an exact zero anywhere in `var` lifts every var <= 0 of the
 * batch to 1e-5 (a one-workgroup pre-pass over `var` finds it); without one a negative variance ends as SX_STATUS_NAN.
 * Uses env->{a,b,k_fb,l_mu,l_sigma,beta}.
 * Replaces: onestep_reachability (gp_reachability_pytorch.py:18-181) with its helpers
 * compute_remainder_overapproximations_pytorch (utils.py:152-194), ellipsoid_from_rectangle_pytorch and
 * sum_two_ellipsoids_pytorch (utils_ellipsoid.py:102-140,282-309), _fix_zeros_nans (:234-243). */
int sx_onestep_reach(const sx_env* env, int P, const double* p, const double* Q, const double* u, const double* mean,
                     const double* var, const double* jac, double* p1, double* Q1, double* sigma, int32_t* status,
                     void* stream);

/* d dev [P x m] = h_mat p + c_safety sqrt(diag(h_mat Q h_mat^T)) - h_vec; inside dev uint8 [P] or NULL.
 * Replaces: lin_ellipsoid_safety_distance / is_ellipsoid_inside_polytope (gp_reachability_pytorch.py:184-231). */
int sx_polytope_distance(const sx_env* env, int P, const double* p, const double* Q, double c_safety, double* d,
                         uint8_t* inside, void* stream);

/* The fused CEM particle rollout: E independent problems x P particles x H steps in ONE launch.
 *   x0      dev [E x n_s]              start states (points; the reference starts every solve from a point,
 *                                      safempc_cem.py:234-235)
 *   q0      dev [E x n_s x n_s] | NULL start shape matrices (NULL = point)
 *   mean,std dev [E x H x n_u]         sampling distribution (ignored when noise == NULL)
 *   noise   dev [E x P x H x n_u]|NULL standard-normal draws; NULL = `actions` is an INPUT
 *   actions dev [E x P x H x n_u]      out: mean + std * noise  (or in, see above)
 *   traj    dev [E x P x H x (n_s + n_s^2)] | NULL   flat states [p | vec_rowmajor(Q)] (PQFlattener, safempc_cem.py:30-76)
 *   sigma   dev [E x P x H x n_s] | NULL
 *   obj_cost, con_cost dev [E x P]     summed objective / constraint cost
 *   status  dev int32                  OR of SX_STATUS_*
 *   workspace dev, sx_cem_rollout_workspace_bytes() bytes (may be NULL when that is 0): training sets whose Kstar tile does
 *                                      not fit in LDS (config 4: N = 2000) take the three-launch-per-step path and keep
 *                                      Kstar, partial sums and particle state there
 * Replaces: the H sequential DynamicsFunc callbacks + per-trajectory Constraint calls the optimiser makes per
 * iteration (safempc_cem.py:102-156,288-312; call sites of the absent constrained-cem-mpc). */
int sx_cem_rollout(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                   const double* mean, const double* std, const double* noise, double* actions, double* traj,
                   double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* sx_cem_rollout for every CEM iteration after the first: the sampling distribution is not handed in but REFIT from the
 * previous iteration's elite rows inside the kernel's prologue -- mean and unbiased standard deviation (0 when k == 1) over
 *   elite_rows dev [E x k x (2 + H*n_u)]  the [con, obj, actions...] rows sx_cem_rank_refit writes (any order),
 * by every workgroup for itself (a wave per column, fixed summation order: the same numbers in every workgroup and on
 * every GPU), while the kernel's other start-up loads travel.  actions = mean + std * noise as in sx_cem_rollout.
 *   mean_out, std_out dev [E x H*n_u] | both NULL   the refit, for callers that want to see it
 * Only for models on the single-launch path (sx_cem_rollout_workspace_bytes() == 0) with 2 H n_u <= 256 (1 + n_s);
 * SX_ERR_UNSUPPORTED otherwise: use sx_cem_rank_refit's mean / std and sx_cem_rollout there.
 * Replaces: the refit step of ConstrainedCemMpc.get_actions (as sx_cem_rank_refit's mean / std outputs do), moved off the
 * ranking kernel's serial tail. */
int sx_cem_rollout_elites(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* x0, const double* q0,
                          const double* elite_rows, int k, const double* noise, double* actions, double* traj, double* sigma,
                          double* obj_cost, double* con_cost, int32_t* status, double* mean_out, double* std_out, void* stream);

/* sx_cem_rollout for a JunkDimensionsSSM over an exact RBF GP (n_s real states and n_u real actions padded with J_s junk
 * states and J_a junk actions, all zero).  Input columns that are zero in every training row and every query add nothing
 * to any kernel value, so the padded GP's real outputs are those of a GP over the D = n_s + n_u + s columns that are ever
 * non-zero, s = query_shift = min(J_s, n_u): training rows [x, u, 0_s], queries [x, 0_s, u].  `model` is that GP
 * (model->n_s == env->n_s, model->n_u == env->n_u + query_shift); `env` and every buffer are shaped by (n_s, n_u) exactly as
 * in sx_cem_rollout.  The reachability step receives the Jacobian's leading n_s + n_u columns -- for the "action" block
 * the derivative by the training rows' action columns, as the reference's padding has it.
 *   query_shift 0 .. env->n_u; 0 is sx_cem_rollout itself (every form, the workspace path included).
 * SX_ERR_ARG (checked before any device access) for null pointers, non-positive sizes or inconsistent shapes;
 * SX_ERR_UNSUPPORTED for query_shift > 0 where the training set needs the workspace path (sx_cem_rollout_workspace_bytes()
 * of the model > 0 -- roll out step by step there) or the shape is not instantiated (n_s + n_u + query_shift <= 6, n_u <= 2).
 * Replaces: the H dynamics callbacks through JunkDimensionsSSM (ssm_cem/ssm_cem.py:134-210) that the optimiser makes per
 * iteration for the reference's junk-dimension experiment (utils_config.py:45-47, safempc_cem.py:288-312). */
int sx_cem_rollout_junk(const sx_gp_model* model, const sx_env* env, int query_shift, int E, int P, int H, const double* x0,
                        const double* q0, const double* mean, const double* std, const double* noise, double* actions,
                        double* traj, double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* sx_cem_rollout_elites for the same models as sx_cem_rollout_junk (the refit from the previous iteration's elite rows, whose
 * action part is H * env->n_u wide).  query_shift 0 is sx_cem_rollout_elites itself.
 * Replaces: as sx_cem_rollout_junk, for every CEM iteration after the first (ConstrainedCemMpc.get_actions' refit step). */
int sx_cem_rollout_elites_junk(const sx_gp_model* model, const sx_env* env, int query_shift, int E, int P, int H,
                               const double* x0, const double* q0, const double* elite_rows, int k, const double* noise,
                               double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                               int32_t* status, double* mean_out, double* std_out, void* stream);

/* Bytes of workspace sx_cem_rollout needs for this model and problem size: 0 = the fused single-launch path applies;
 * < 0 = bad arguments. */
int64_t sx_cem_rollout_workspace_bytes(const sx_gp_model* model, int E, int P, int H);

/* Which kernel sx_cem_rollout / sx_cem_rollout_elites launch for this model and horizon (no launch, no device access):
 *   SX_FORM_RH      cem_rollout_rh_kernel: 8 waves, the GP's triangular factors partly resident (registers / LDS / L2)
 *   SX_FORM_RW      cem_rollout_rw_kernel: 4 waves, the factors in the register file
 *   SX_FORM_STREAM  cem_rollout_kernel: the factors streamed from L2, Kstar of all outputs in LDS
 *   SX_FORM_BYOUT   cem_rollout_kernel, one output's Kstar in LDS at a time
 *   SX_FORM_BIG     the three-launch-per-step path (Kstar in HBM)
 * or < 0 for bad arguments and wherever sx_cem_rollout would answer SX_ERR_UNSUPPORTED ((n_s, n_u) without a rollout
 * kernel; SX_ROLLOUT_STRICT with a forced form that does not apply).  Reporting only (bench.py names the kernel it timed);
 * the choice itself is the library's, and the same one sx_cem_rollout makes.
 * No counterpart in the reference. */
#define SX_FORM_STREAM 0
#define SX_FORM_RW 1
#define SX_FORM_RH 2
#define SX_FORM_BYOUT 3
#define SX_FORM_BIG 4
int sx_cem_rollout_form(const sx_gp_model* model, int H);

/* How the three-launch path (SX_FORM_BIG, and sx_gp_predict beyond its single launch) tiles the triangular product of this
 * model (its n_s and n_pad) over `particles` query points -- E * P of a rollout, P of a prediction -- (no launch, no device
 * access):
 *   pt       particle tiles of 16 per workgroup: 8 (128 x 128 tiles) or 4 (128 x 64)
 *   order    tile order: 16 = paired row tiles, 8 = longest tile first, 1 = XCD-contiguous, 0 = plain (+ the diagnostic bits)
 *   variant  <fragment pairs per K-chunk><LDS buffers> of the kernel: 13, 12, 22 or 23
 *   grid     workgroups of the launch
 * The shape decides, and the process's SX_TRMM_ORDER / SX_TRMM_VARIANT / SX_TRMM_PT as in the launch itself:
 * the answer is the one the launcher acts on.  It is given for any model, whether or not its training set takes that path
 * (sx_cem_rollout_form, sx_gp_predict_workspace_bytes say so).  SX_ERR_ARG for null pointers, particles < 0 or a model
 * without sizes.  Reporting only, as sx_cem_rollout_form.
 * No counterpart in the reference. */
int sx_gp_big_tiling(const sx_gp_model* model, int64_t particles, int* pt, int* order, int* variant, int64_t* grid);

/* sx_cem_rollout with a start state per particle (static exploration: the start is a decision variable of the optimiser).
 * The CEM row of a particle is [x0 (n_s) | u_0 .. u_{H-1} (H n_u)], L = n_s + H n_u entries with one Gaussian each:
 *   mean,std dev [E x L]               sampling distribution of the rows (ignored when noise == NULL)
 *   noise   dev [E x P x L] | NULL     standard-normal draws; NULL = `rows` is an INPUT
 *   rows    dev [E x P x L]            out: mean + std * noise  (or in, see above)
 *   traj, sigma, obj_cost, con_cost, status   as in sx_cem_rollout
 * Every particle is rolled out from the point x0 of its own row with the actions of its row, and the costs are
 * sx_cem_rollout's (env->obj_mode, env->con_mode, the action box) plus SX_STATE_VIOLATION_COST once, in either constraint
 * mode, for a start outside the safe polytope (h_mat x0 - h_vec >= 0 in any row): a sample is taken at (x0, u_0), so the
 * system is put there.  The reference's NLP leaves p_0 free; this rule is this library's own.
 * The streaming kernel only (SX_FORM_STREAM or SX_FORM_BYOUT, sx_cem_rollout_starts_form): no workspace path.
 * SX_ERR_ARG (checked before any device access) for null pointers, non-positive sizes, a model whose (n_s, n_u) differ from
 * env's, or noise without mean / std; SX_ERR_UNSUPPORTED (before any launch) for a shape without a rollout kernel,
 * env->m > SX_MAX_M, or a training set that needs the workspace path (sx_cem_rollout_workspace_bytes() > 0) or fits neither
 * form.
 * Replaces: the rollout and constraint evaluation inside StaticSafeMPCExploration's NLP over [p_0, u_0, k_ff]
 * (safempc_exploration.py:100-163,281-330), one NLP solve per restart. */
int sx_cem_rollout_starts(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* mean,
                          const double* std, const double* noise, double* rows, double* traj, double* sigma,
                          double* obj_cost, double* con_cost, int32_t* status, void* stream);
/* The form sx_cem_rollout_starts launches for this model and horizon (no launch, no device access): SX_FORM_STREAM or
 * SX_FORM_BYOUT, or < 0 for bad arguments and wherever sx_cem_rollout_starts would answer SX_ERR_UNSUPPORTED for the model.
 * The same contract as sx_cem_rollout_form.
 * Replaces: nothing in safempc_exploration.py:100-163,281-330, whose NLP has one form. */
int sx_cem_rollout_starts_form(const sx_gp_model* model, int H);

/* sx_cem_rollout_starts under a feedback gain per particle and step (multi-step reachability, u = K_t (x - p_t) + k_ff_t):
 *   gains   dev [E x P x (H-1) x n_u x n_s]   K_t of particle (e, c) for step t = 1 .. H-1 at index t - 1, row-major
 *                                             [n_u x n_s]; required for H > 1, may be NULL for H == 1
 *   every other argument as in sx_cem_rollout_starts (the rows [x0 | k_ff_0 .. k_ff_{H-1}], drawn or given)
 * Step 0 starts from the point x0 of the particle's row and reads no gain (the reference's k_fb_init = None); step t >= 1
 * propagates the ellipsoid (p_t, Q_t) under K_t: the lane that owns the particle forms the lower Cholesky factor of
 * I + K_t^T K_t for itself.  env->k_fb is NOT read by this entry.  traj, sigma, obj_cost, con_cost (the objective, the
 * action box on the rows' actions, the polytope mode, SX_STATE_VIOLATION_COST for a start outside the polytope) and status
 * are sx_cem_rollout_starts' otherwise.  A non-finite gain sets SX_STATUS_NAN for the launch and leaves every other
 * particle's outputs as they are without it; a gain is data only, never an index.
 * The streaming kernel only (SX_FORM_STREAM or SX_FORM_BYOUT, sx_cem_rollout_gains_form): no workspace path.
 * SX_ERR_ARG and SX_ERR_UNSUPPORTED (both before any device access) as sx_cem_rollout_starts, and SX_ERR_ARG for NULL gains
 * with H > 1.
 * Replaces: multistep_reachability (gp_reachability.py:168-221), one onestep_reachability per rollout and step, as
 * run_uncertainty_propagation calls it per rollout (uncertainty_propagation_runner.py:28-41). */
int sx_cem_rollout_gains(const sx_gp_model* model, const sx_env* env, int E, int P, int H, const double* mean,
                         const double* std, const double* noise, double* rows, const double* gains, double* traj,
                         double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream);
/* The form sx_cem_rollout_gains launches for this model and horizon (no launch, no device access): the answer, and the
 * contract, of sx_cem_rollout_starts_form.
 * Replaces: nothing in gp_reachability.py:168-221, which has one form. */
int sx_cem_rollout_gains_form(const sx_gp_model* model, int H);

/* ---- E problems with an exact GP each in one rollout launch (independent exploration runs) ----
 * Every problem e of the launch has its own training set (its own N) and hyper-parameters; all models share (n_s, n_u),
 * the sx_env and the buffer shapes of sx_cem_rollout.  The per-problem GP constants live in a device table that is built
 * once per model change (the warm path); the rollout entries read it and copy nothing from the host.
 *
 * Bytes of the table for E models of shape (n_s, n_u); < 0 for bad arguments or a shape without a rollout kernel. */
int64_t sx_gp_model_table_bytes(int n_s, int n_u, int E);
/* Packs the E models (host array, each built by sx_gp_fit + sx_gp_pack) into `table` (dev, sx_gp_model_table_bytes()
 * bytes): their GP constants and the device pointers x_train, a_pack, stage_tab, which must stay valid while the table is
 * used.  One host -> device copy on `stream`, and the call waits for it.  SX_ERR_ARG (before any device access) for a null
 * pointer, E <= 0 or models of different (n_s, n_u); SX_ERR_UNSUPPORTED for a shape without a rollout kernel.
 * Replaces: nothing in the reference, which runs its n_scenarios solvers one after another (episode_runner.py:40-123). */
int sx_gp_model_table(const sx_gp_model* models, int E, void* table, void* stream);
/* sx_cem_rollout over E problems with a GP each: `models` is the host array the table was built from (the launch plans
 * from it: N of every model), `table` the device table.  Buffers as in sx_cem_rollout except
 *   status  dev int32 [E]   one word per problem (OR of SX_STATUS_*): a NaN in one problem's model leaves the others clear
 * The streaming kernel only: output by output for all problems where any model needs it, the LDS of the largest model.
 * SX_ERR_ARG (before any device access) for null pointers, non-positive sizes or shapes that differ between the models or
 * from env; SX_ERR_UNSUPPORTED where any model needs the workspace path (sx_cem_rollout_workspace_bytes() > 0) or the shape
 * has no rollout kernel.  Replaces: the n_scenarios sequential solves' rollouts (episode_runner.py:40-123). */
int sx_cem_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                         const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                         double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost, int32_t* status,
                         void* stream);
/* sx_cem_rollout_elites over E problems with a GP each: the refit prologue from elite_rows [E x k x (2 + H n_u)], then
 * sx_cem_rollout_multi.  Same limits as sx_cem_rollout_elites and sx_cem_rollout_multi; status dev int32 [E]. */
int sx_cem_rollout_elites_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                                const double* x0, const double* q0, const double* elite_rows, int k, const double* noise,
                                double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                                int32_t* status, double* mean_out, double* std_out, void* stream);
/* The form sx_cem_rollout_multi launches for these models and horizon (no launch, no device access): SX_FORM_STREAM or
 * SX_FORM_BYOUT, or < 0 for bad arguments and wherever sx_cem_rollout_multi would answer SX_ERR_UNSUPPORTED.  The same
 * contract as sx_cem_rollout_form. */
int sx_cem_rollout_multi_form(const sx_gp_model* models, int E, int H);

/* ---- E problems with a feature GP / an MC-dropout ensemble each in one rollout launch ----
 * As sx_cem_rollout_multi for the exact GP: every problem e has its own model (its own training data, hyper-parameters,
 * network weights and masks); the models share (n_s, n_u), the sx_env, the buffer shapes of sx_cem_rollout_feat /
 * sx_cem_rollout_mlp and their ARCHITECTURE, which fixes the kernel and its LDS for the whole launch:
 *   feature GP:  n_layers, width[0 .. n_layers], normalise, n_feat
 *   MC-dropout:  n_hidden, width[0 .. n_hidden], n_out, n_samples, predict_std   (SX_MLP_PATH=valu applies as for one model)
 * The per-problem constants live in a device table built once per model change.
 *
 * Bytes of the table for these E models; < 0 for bad arguments, models whose (n_s, n_u) or architecture differ, or a shape
 * without a rollout kernel: the host-only answer to "does one launch serve these models". */
int64_t sx_feat_model_table_bytes(const sx_feat_model* models, int E);
/* Packs the E models (host array) into `table` (dev, sx_feat_model_table_bytes() bytes): their constants and the device
 * pointers net, wbar, minv, which must stay valid while the table is used.  One host -> device copy on `stream`, and the
 * call waits for it.  SX_ERR_ARG (before any device access) for a null pointer, E <= 0 or models of different (n_s, n_u);
 * SX_ERR_UNSUPPORTED for differing architectures or a shape without a rollout kernel. */
int sx_feat_model_table(const sx_feat_model* models, int E, void* table, void* stream);
/* sx_cem_rollout_feat over E problems with a feature GP each: `models` is the host array the table was built from,
 * `table` the device table.  Buffers as in sx_cem_rollout_feat except
 *   status  dev int32 [E]   one word per problem (OR of SX_STATUS_*): a NaN in one problem's model leaves the others clear
 * SX_ERR_ARG (before any device access) for null pointers, E <= 0, non-positive sizes or shapes that differ between the
 * models or from env; SX_ERR_UNSUPPORTED (before any launch) for differing architectures or a shape without a kernel.
 * No elite-row form.  Replaces: the n_scenarios sequential solves' rollouts (episode_runner.py:40-123). */
int sx_cem_rollout_feat_multi(const sx_feat_model* models, const void* table, const sx_env* env, int E, int P, int H,
                              const double* x0, const double* q0, const double* mean, const double* std,
                              const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                              double* con_cost, int32_t* status, void* stream);
/* The same three for MC-dropout ensembles: the table carries the device pointers net and masks. */
int64_t sx_mlp_model_table_bytes(const sx_mlp_model* models, int E);
int sx_mlp_model_table(const sx_mlp_model* models, int E, void* table, void* stream);
int sx_cem_rollout_mlp_multi(const sx_mlp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                             const double* x0, const double* q0, const double* mean, const double* std,
                             const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                             double* con_cost, int32_t* status, void* stream);

/* ---- The performance trajectory of the CEM solver ----
 * A SafeMPC plans two trajectories: the safety trajectory (sx_cem_rollout: H steps of ellipsoids, the constraints) and
 * the performance trajectory, n_perf steps of plain mean predictions that share their first r actions with the safety
 * trajectory and carry the objective.  One launch per CEM iteration, after the safety rollout, for E problems x P particles:
 *   v_t = safe_actions[t] (t < r), tail[t - r] (t >= r);   mu_0 = x0,   mu_{t+1} = a mu_t + b v_t + mean_GP([mu_t, v_t])
 * (one_step_mean_equivalent with sigma_x = None, chained as mean_equivalent_multistep: no feedback term, no variance).
 *   model        {n_s, n_u, n_train, inv_ls2, outputscale, x_train} of the exact RBF GP
 *   alpha        dev [n_s x N]                 as sx_gp_fit wrote it
 *   env          {n_s, n_u, a, b, u_min, u_max, obj_mode, obj_w_abs, obj_target, obj_w_lin}
 *   H, n_perf, r 1 <= r <= H, n_perf > r; T = n_perf - r tail steps
 *   x0           dev [E x n_s]
 *   safe_actions dev [E x P x H x n_u]         what the safety rollout wrote (the shared actions are then bit-identical)
 *   tail_mean, tail_std dev [E x T x n_u]      sampling distribution of the tail (ignored when tail_noise == NULL)
 *   tail_noise   dev [E x P x T x n_u] | NULL  standard-normal draws; NULL = the tail of `rows` is an INPUT
 *   rows         dev [E x P x (H + T) x n_u]   out: [safe_actions | tail], tail = tail_mean + tail_std * tail_noise: the rows
 *                                              sx_cem_rank_refit ranks and refits (row_len = (H + T) n_u)
 *   obj_cost     dev [E x P]                   OVERWRITTEN with sum_{t = 1..n_perf} cost(mu_t), cost = SX_OBJ_AFFINE_ABS
 *   con_cost     dev [E x P]                   ADDED TO: SX_ACTION_VIOLATION_COST per tail step whose action leaves
 *                                              [u_min, u_max] (the safety rollout has counted the shared steps; the
 *                                              performance trajectory has no state constraint)
 *   perf_traj    dev [E x P x n_perf x n_s] | NULL   mu_1 .. mu_n_perf
 *   status       dev int32                     OR-ed with SX_STATUS_NAN on a non-finite mu_t
 * A particle's numbers do not depend on P or on the launch's grid.
 * SX_ERR_ARG (before any device access) for null pointers, non-positive sizes, r outside 1 .. H, n_perf <= r, tail_noise
 * without tail_mean / tail_std, or shapes that differ between model and env; SX_ERR_UNSUPPORTED for env->obj_mode ==
 * SX_OBJ_NEG_VARIANCE (the variance needs the safety kernels' N x N product), a shape sx_cem_rollout is not instantiated
 * for, or a training set beyond the kernel's LDS ((2 n_s + n_u) N doubles: N <= 2016 at the widest shape).
 * Replaces: nothing in the reference's CEM solver, which has no performance trajectory (safempc_cem.py:212-215); its casadi
 * solver builds one in safempc_simple.py:398-490. */
int sx_cem_perf_rollout(const sx_gp_model* model, const double* alpha, const sx_env* env, int E, int P, int H, int n_perf,
                        int r, const double* x0, const double* safe_actions, const double* tail_mean,
                        const double* tail_std, const double* tail_noise, double* rows, double* obj_cost, double* con_cost,
                        double* perf_traj, int32_t* status, void* stream);

/* The performance trajectory WITH the GP's posterior variance ("variance form"): what an
 * exploration run plans with.  Per particle, with v_t and mu_0 as above,
 *   (mean_t, var_t) = GP posterior at [mu_t, v_t] (noise included, as sx_gp_predict)
 *   mu_{t+1} = a mu_t + b v_t + mean_t;   obj += cost(mu_{t+1}, var_t)       t = 0 .. n_perf - 1
 * cost = -sum_d var_t[d] for SX_OBJ_NEG_VARIANCE (the CEM solver's exploration objective, safempc_cem.py:304-312, moved
 * onto the performance trajectory), the separable objective on mu_{t+1} for SX_OBJ_AFFINE_ABS (sx_cem_perf_rollout's
 * objective; the variances are then an extra output).  No zero / negative fix-up of var_t (nothing takes its square root),
 * no variance propagation, no feedback term, no state constraint.
 * Arguments as sx_cem_perf_rollout, except:
 *   model        the PACKED exact-GP model sx_cem_rollout takes (x_train, a_pack, stage_tab, n_pad of sx_gp_pack): the
 *                variance needs W and the stage table, not alpha
 *   perf_sigma   dev [E x P x n_perf x n_s] | NULL   var_0 .. var_{n_perf - 1}
 *   status       OR-ed with SX_STATUS_NAN on a non-finite mu_t or var_t (that particle's objective is NaN: it never ranks)
 * One workgroup of SX_WAVES waves per tile of 16 particles, the Kstar and matrix phases of the streaming safety kernel per
 * step; a tile's numbers do not depend on P or on the launch's grid.
 * SX_ERR_ARG (before any device access) as sx_cem_perf_rollout, and for a model without a_pack / stage_tab / a valid n_pad
 * or an obj_mode that is neither of the two; SX_ERR_UNSUPPORTED for a shape sx_cem_rollout is not instantiated for and for
 * training sets outside the two forms built: Kstar of all outputs in LDS beside the tile's n_perf actions (N up to ~ 524
 * at (n_s, n_u) = (2, 1)), else output by output (n_s > 1).  Both need n_pad <= 1024 AND their LDS, which grows with n_perf:
 * one output reaches n_pad = 1024 (N = 1021 at (1, 1), up to n_perf = 68); for n_s > 1 the training inputs and one
 * output's Kstar fill the LDS before that -- at n_perf = 2 the largest N is 988 at (2, 1), 939 at (2, 2), 923 at (3, 1),
 * 858 at (4, 1), 809 at (4, 2) -- and a model just below goes from all outputs in LDS to output by output as n_perf grows.
 * sx_cem_perf_rollout_var_form answers for a model and an n_perf.  No resident-W form, no workspace path.
 * Replaces: nothing in the reference's CEM solver; its casadi solver sums gp_sigma_pred of mean_equivalent_multistep
 * (safempc_simple.py:292-321, 398-490). */
int sx_cem_perf_rollout_var(const sx_gp_model* model, const sx_env* env, int E, int P, int H, int n_perf, int r,
                            const double* x0, const double* safe_actions, const double* tail_mean, const double* tail_std,
                            const double* tail_noise, double* rows, double* obj_cost, double* con_cost, double* perf_traj,
                            double* perf_sigma, int32_t* status, void* stream);

/* ---- The performance trajectory for E problems with an exact GP each ("multi-model form") ----
 * One performance-rollout launch per CEM iteration for E exploration scenarios, after sx_cem_rollout_multi: every problem
 * e has its own model; all models share (n_s, n_u), the sx_env and the buffer shapes of sx_cem_perf_rollout[_var], per
 * problem.  `models` is the host array the launch plans from (N of every model), the device table carries the constants.
 *
 * The mean-only form reads alpha, which the packed sx_gp_model does not carry: a table of its own, built once per model
 * change.  Bytes of it for E models of shape (n_s, n_u); < 0 for bad arguments or a shape without a kernel. */
int64_t sx_cem_perf_table_bytes(int n_s, int n_u, int E);
/* Packs, for each of the E models (host array), the kernel constants, the device pointers x_train and alphas[e] (host
 * array of E device pointers, dev [n_s x N_e] as sx_gp_fit wrote them) and N_e into `table` (dev,
 * sx_cem_perf_table_bytes() bytes); the pointers must stay valid while the table is used.  One host -> device copy on
 * `stream`, and the call waits for it.  SX_ERR_ARG (before any device access) for a null pointer (a null alphas[e]
 * included), E <= 0, models of different (n_s, n_u) or without x_train / n_train; SX_ERR_UNSUPPORTED for a shape without a
 * kernel. */
int sx_cem_perf_table(const sx_gp_model* models, const double* const* alphas, int E, void* table, void* stream);
/* sx_cem_perf_rollout over E problems with a GP each: problem e's numbers are those of sx_cem_perf_rollout on model e
 * alone, bit for bit (the lanes per particle and every model's padding are the single-model kernel's).  Arguments as
 * sx_cem_perf_rollout except
 *   models      host array of the E models the table was built from
 *   perf_table  dev, built by sx_cem_perf_table
 *   status      dev int32 [E]   one word per problem: a NaN in one problem's model leaves the others clear
 * The grid is problem-aligned, E x ceil(P / 16) workgroups: a workgroup stages its own problem's training inputs and alpha
 * in LDS, inside the launch's allocation for the largest model.
 * SX_ERR_ARG (before any device access) for null pointers, non-positive sizes, r outside 1 .. H, n_perf <= r, tail_noise
 * without tail_mean / tail_std, shapes that differ between the models or from env, or an obj_mode that is none of the two;
 * SX_ERR_UNSUPPORTED (before any launch) for SX_OBJ_NEG_VARIANCE, a shape without a kernel or a model beyond the kernel's
 * LDS, as sx_cem_perf_rollout.  Replaces: nothing in the reference's CEM solver; its n_scenarios casadi solvers each build
 * a performance trajectory and run one after another (episode_runner.py:40-123, safempc_simple.py:398-490). */
int sx_cem_perf_rollout_multi(const sx_gp_model* models, const void* perf_table, const sx_env* env, int E, int P, int H,
                              int n_perf, int r, const double* x0, const double* safe_actions, const double* tail_mean,
                              const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                              double* con_cost, double* perf_traj, int32_t* status, void* stream);
/* sx_cem_perf_rollout_var over E problems with a GP each.  Arguments as sx_cem_perf_rollout_var except
 *   models  host array of the E PACKED models
 *   table   dev, the table sx_gp_model_table built from them (the one sx_cem_rollout_multi reads)
 *   status  dev int32 [E]   one word per problem
 * Output by output for every problem where any model needs it, with the LDS of the largest model
 * (sx_cem_perf_rollout_var_multi_form); where that form is model e's own (sx_cem_perf_rollout_var_form) problem e's numbers
 * are those of sx_cem_perf_rollout_var on model e alone, bit for bit.
 * SX_ERR_ARG (before any device access) as sx_cem_perf_rollout_var, for every model, and for shapes that differ between
 * the models or from env; SX_ERR_UNSUPPORTED (before any launch) where any model has no form or the shape no kernel. */
int sx_cem_perf_rollout_var_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                                  int n_perf, int r, const double* x0, const double* safe_actions, const double* tail_mean,
                                  const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                                  double* con_cost, double* perf_traj, double* perf_sigma, int32_t* status, void* stream);
/* The form sx_cem_perf_rollout_var / sx_cem_perf_rollout_var_multi launch for this model / these models and n_perf (no
 * launch, no device access): SX_FORM_STREAM (Kstar of all outputs in LDS) or SX_FORM_BYOUT, or < 0 for bad arguments (a
 * null pointer, n_perf <= 1, an unpacked model, models of different shapes) and wherever the entry would answer
 * SX_ERR_UNSUPPORTED.  The same contract as sx_cem_rollout_form / sx_cem_rollout_multi_form. */
int sx_cem_perf_rollout_var_form(const sx_gp_model* model, int n_perf);
int sx_cem_perf_rollout_var_multi_form(const sx_gp_model* models, int E, int n_perf);

/* ---- The performance trajectory with Taylor uncertainty propagation ("Taylor form") ----
 * sx_cem_perf_rollout_var with the state covariance carried from step to step: a first-order propagation under the fixed
 * feedback K = env->k_fb, the gain the safety rollout uses.  Per particle, with v_t and mu_0 as above and Sigma_0 = 0:
 *   (mean_t, var_t, J_t) = GP posterior and mean Jacobian at [mu_t, v_t] (noise included, as sx_gp_predict), J_t = [J_x | J_u]
 *   M = J_x + J_u K;   Hm = a + b K + M;   G_t = diag(var_t) + M Sigma_t M^T
 *   mu_{t+1} = a mu_t + b v_t + mean_t;   Sigma_{t+1} = Hm Sigma_t Hm^T + diag(var_t)
 *   obj += cost(mu_{t+1}, diag G_t)                                         t = 0 .. n_perf - 1
 * cost = -tr G_t for SX_OBJ_NEG_VARIANCE, the separable objective on mu_{t+1} for SX_OBJ_AFFINE_ABS.  mu is the variance
 * form's, bit for bit (the feedback term has zero mean); G_0 = diag(var_0) and Sigma_1 = diag(var_0) exactly.  No zero /
 * negative fix-up.
 * Arguments as sx_cem_perf_rollout_var, except:
 *   env          also {k_fb, m, h_mat, h_vec}
 *   perf_sigma   dev [E x P x n_perf x n_s] | NULL          diag G_0 .. diag G_{n_perf - 1}
 *   perf_cov     dev [E x P x n_perf x n_s x n_s] | NULL    Sigma_1 .. Sigma_{n_perf}, row-major, symmetric to the bit
 *   terminal_safety  != 0: the ellipsoid (mu_s, Sigma_s), s = H + 2, must lie inside the safe polytope -- some
 *                h_j . mu_s + sqrt(h_j^T Sigma_s h_j) - h_vec_j >= 0 adds SX_STATE_VIOLATION_COST to con_cost once (a NaN
 *                distance counts as inside, as everywhere); needs n_perf >= H + 2 and m > 0
 *   status       OR-ed with SX_STATUS_NAN on a non-finite mu_t, var_t, G_t or Sigma_t (that particle's objective is NaN)
 * The variance kernel's layout and forms (all outputs in LDS, else output by output; n_pad <= 1024 and the LDS bound both,
 * as there), with the step constants (41 .. 144 doubles) in LDS behind the tile's actions: they count against the same LDS, so
 * a form ends at a smaller n_perf or N than the variance kernel's (at n_perf = 2: N = 907 at (3, 1), 842 at (4, 1), else the
 * variance form's; sx_cem_perf_rollout_taylor_form answers).  A tile's numbers do not depend on P or on the grid.
 * SX_ERR_ARG (before any device access) as sx_cem_perf_rollout_var, and for terminal_safety with n_perf < H + 2 or without
 * polytope rows; SX_ERR_UNSUPPORTED as sx_cem_perf_rollout_var and for m > SX_MAX_M.
 * Replaces: one_step_taylor / multi_step_taylor_symbolic (uncertainty_propagation_casadi.py:11-149) as the casadi solver
 * chains them for type_perf_traj = 'taylor', and its terminal safety performance constraint (safempc_simple.py:471-479);
 * the reference's CEM solver has neither. */
int sx_cem_perf_rollout_taylor(const sx_gp_model* model, const sx_env* env, int E, int P, int H, int n_perf, int r,
                               const double* x0, const double* safe_actions, const double* tail_mean,
                               const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                               double* con_cost, double* perf_traj, double* perf_sigma, double* perf_cov,
                               int terminal_safety, int32_t* status, void* stream);
/* The form sx_cem_perf_rollout_taylor launches for this model and n_perf (no launch, no device access): SX_FORM_STREAM or
 * SX_FORM_BYOUT, or < 0 for bad arguments and wherever the entry would answer SX_ERR_UNSUPPORTED: the contract of
 * sx_cem_perf_rollout_var_form, decided by the same rule over the variance kernel's LDS plus the step constants
 * (uncertainty_propagation_casadi.py:11-149 and safempc_simple.py:471-479 have no such notion). */
int sx_cem_perf_rollout_taylor_form(const sx_gp_model* model, int n_perf);
/* sx_cem_perf_rollout_taylor over E problems with a GP each.  Arguments as sx_cem_perf_rollout_taylor except
 *   models  host array of the E PACKED models
 *   table   dev, the table sx_gp_model_table built from them (the one sx_cem_rollout_multi reads)
 *   status  dev int32 [E]   one word per problem
 * There is one env: k_fb, the polytope and the terminal-safety step H + 2 are the same for all problems.  Output by output
 * for every problem where any model needs it, with the LDS of the largest model plus the step constants
 * (sx_cem_perf_rollout_taylor_multi_form); where that form is model e's own (sx_cem_perf_rollout_taylor_form) problem e's
 * numbers are those of sx_cem_perf_rollout_taylor on model e alone, bit for bit.
 * SX_ERR_ARG (before any device access) as sx_cem_perf_rollout_taylor, for every model, and for shapes that differ between
 * the models or from env; SX_ERR_UNSUPPORTED (before any launch) for m > SX_MAX_M, where any model has no form or the
 * shape no kernel.  Replaces: nothing in the reference's CEM solver; its n_scenarios casadi solvers with
 * type_perf_traj = 'taylor' run one after another (episode_runner.py:40-123, safempc_simple.py:398-490). */
int sx_cem_perf_rollout_taylor_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                                     int n_perf, int r, const double* x0, const double* safe_actions,
                                     const double* tail_mean, const double* tail_std, const double* tail_noise,
                                     double* rows, double* obj_cost, double* con_cost, double* perf_traj,
                                     double* perf_sigma, double* perf_cov, int terminal_safety, int32_t* status,
                                     void* stream);
/* The form sx_cem_perf_rollout_taylor_multi launches for these models and n_perf (no launch, no device access): the
 * contract of sx_cem_perf_rollout_var_multi_form (< 0 also for unpacked models), by the rule of
 * sx_cem_perf_rollout_taylor_form. */
int sx_cem_perf_rollout_taylor_multi_form(const sx_gp_model* models, int E, int n_perf);

/* ---- Cautious MPC: the chance-constrained Taylor rollout ----
 * The trajectory of sx_cem_perf_rollout_taylor on its own -- no safety rollout in front of it -- with the reference's
 * chance constraints on every step.  A particle's row is k_ff_0 .. k_ff_{T-1} [T x n_u]; mu_0 = x0[e], Sigma_0 = 0,
 * K = env->k_fb, beta = env->beta.  For t = 0 .. T - 1:
 *   control  t = 0:  k_ff_0 outside [u_min, u_max] adds SX_ACTION_VIOLATION_COST
 *            t >= 1: s_c = beta sqrt(K_c Sigma_t K_c^T); k_ff_t[c] + s_c - u_max[c] >= 0 or u_min[c] - k_ff_t[c] + s_c >= 0
 *                    for any control c adds SX_ACTION_VIOLATION_COST, once per step
 *   (mean_t, var_t, J_t), M, Hm, G_t, mu_{t+1}, Sigma_{t+1}: as sx_cem_perf_rollout_taylor, at [mu_t, k_ff_t]
 *   state    some row j of env's polytope with h_j . mu_{t+1} + beta sqrt(h_j^T Sigma_{t+1} h_j) - h_vec_j >= 0 adds
 *            SX_STATE_VIOLATION_COST, once per step (m = 0: none)
 *   obj += cost(mu_{t+1}, diag G_t)          SX_OBJ_AFFINE_ABS | SX_OBJ_NEG_VARIANCE, as sx_cem_perf_rollout_taylor
 * A distance d >= 0 violates and a NaN distance counts as inside, as everywhere.  Which polytope env->{m, h_mat, h_vec} is
 * (the reference checks the obstacle polytope h_mat_obs) is the caller's choice.
 *   mean, std    dev [E x T x n_u], noise dev [E x P x T x n_u]: the rows are drawn as mean + std * noise and written; with
 *                noise NULL the rows are an input
 *   rows         dev [E x P x T x n_u]
 *   obj_cost     dev [E x P]   overwritten; NaN, with SX_STATUS_NAN in status, on a non-finite mu, var, G or Sigma
 *   con_cost     dev [E x P]   OVERWRITTEN: there is no safety rollout before this one
 *   traj         dev [E x P x T x n_s] | NULL          mu_1 .. mu_T
 *   sigma        dev [E x P x T x n_s] | NULL          diag G_0 .. diag G_{T-1}
 *   cov          dev [E x P x T x n_s x n_s] | NULL    Sigma_1 .. Sigma_T, symmetric to the bit
 *   margins      dev [E x P x T x 2] | NULL            per step: the largest state row distance (-inf for m = 0), the
 *                largest of the 2 n_u control distances (at t = 0 the plain box's k - u_max, u_min - k)
 *   propagate    0: every GP step starts from Sigma_t = 0, so G_t = var_t and Sigma_{t+1} = diag(var_t) (the reference's
 *                perf_trajectory = 'mean_equivalent', one_step_mean_equivalent); the control constraint of step t still
 *                sees diag(var_{t-1})
 * The Taylor kernel's layout and forms (SX_FORM_STREAM, else SX_FORM_BYOUT; n_pad <= 1024), the step constants plus beta in
 * LDS behind the tile's T actions.  A tile's numbers do not depend on P or on the grid.
 * SX_ERR_ARG (before any device access) for null pointers, T < 1, non-positive sizes, noise without mean / std, an
 * unpacked model, a shape different from env's, an obj_mode that is neither of the two; SX_ERR_UNSUPPORTED (before any
 * launch) for m > SX_MAX_M, a shape without a kernel or a model without a form.
 * Replaces: generate_safety_constraints and _generate_control_constraint (cautious_mpc.py:337-442) over
 * multi_step_taylor_symbolic / mean_equivalent_multistep, which CautiousMPC.init_solver hands to IPOPT as one NLP. */
int sx_cem_cautious_rollout(const sx_gp_model* model, const sx_env* env, int E, int P, int T, const double* x0,
                            const double* mean, const double* std, const double* noise, double* rows, double* obj_cost,
                            double* con_cost, double* traj, double* sigma, double* cov, double* margins, int propagate,
                            int32_t* status, void* stream);
/* The form sx_cem_cautious_rollout launches for this model and T (no launch, no device access): SX_FORM_STREAM or
 * SX_FORM_BYOUT, or < 0 for bad arguments (T < 1 among them) and wherever the entry would answer SX_ERR_UNSUPPORTED for
 * the model: the contract of sx_cem_perf_rollout_taylor_form (cautious_mpc.py has no such notion). */
int sx_cem_cautious_rollout_form(const sx_gp_model* model, int T);
/* sx_cem_cautious_rollout over E problems with a GP each.  Arguments as sx_cem_cautious_rollout except
 *   models  host array of the E PACKED models, all of one (n_s, n_u)
 *   table   dev, the table sx_gp_model_table built from them (the one sx_cem_rollout_multi reads)
 *   status  dev int32 [E]   one word per problem
 * There is one env: k_fb, the box, the polytope and beta are the same for all problems.  Output by output for every
 * problem where any model needs it, with the LDS of the largest model plus the step constants
 * (sx_cem_cautious_rollout_multi_form); where that form is model e's own (sx_cem_cautious_rollout_form) problem e's numbers
 * are those of sx_cem_cautious_rollout on model e alone, bit for bit.
 * SX_ERR_ARG (before any device access) as sx_cem_cautious_rollout, for every model, a NULL table, and for shapes that
 * differ between the models or from env; SX_ERR_UNSUPPORTED (before any launch) for m > SX_MAX_M, where any model has no
 * form or the shape no kernel.  Replaces: nothing in the reference's solver; the n_scenarios CautiousMPC solvers of an
 * experiment run one after another (episode_runner.py:40-123 over cautious_mpc.py:337-442). */
int sx_cem_cautious_rollout_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int T,
                                  const double* x0, const double* mean, const double* std, const double* noise,
                                  double* rows, double* obj_cost, double* con_cost, double* traj, double* sigma,
                                  double* cov, double* margins, int propagate, int32_t* status, void* stream);
/* The form sx_cem_cautious_rollout_multi launches for these n models and T (no launch, no device access): SX_FORM_STREAM
 * where every model's Kstar fits in LDS, SX_FORM_BYOUT as soon as one model needs it, < 0 for bad arguments (T < 1, mixed
 * shapes or an unpacked model among them) and wherever the entry would answer SX_ERR_UNSUPPORTED: the contract of
 * sx_cem_perf_rollout_taylor_multi_form over the cautious step constants (cautious_mpc.py has no such notion). */
int sx_cem_cautious_rollout_multi_form(const sx_gp_model* models, int n, int T);

/* ---- The PILCO saturating cost of a state Gaussian, as a kernel objective of the Taylor rollouts ---------------------------
 * What the reference's cart-pole configs hand to init_solver (defaultconfig_episode.py:113-159 over utils_casadi.py:178-363,
 * trig_aug with a = 1, keep_radian = False).  For (mu [n_s], Sigma [n_s x n_s]) and an optional angle index i = trig_idx:
 *   e0 = exp(-Sigma_ii / 2), s = e0 sin mu_i, c = e0 cos mu_i, e1 = exp(-2 Sigma_ii)
 *   V_ss = (1 - e1 cos 2 mu_i) / 2 - s^2,  V_cc = (1 + e1 cos 2 mu_i) / 2 - c^2,  V_sc = e1 sin(2 mu_i) / 2 - s c
 *   Cov(x, sin) = Sigma[:, i] c,  Cov(x, cos) = -Sigma[:, i] s
 *   m~ = [mu without entry i, s, c] (n_a = n_s + 1), S~ the matching covariance; without an angle m~ = mu, S~ = Sigma, n_a = n_s
 *   loss = 1 - exp(-1/2 d^T W (I + S~ W)^-1 d) / sqrt(det(I + S~ W)),  d = m~ - target,  W = V V^T
 * evaluated in the symmetric form y = V^T d, S = I_k + V^T S~ V, L = chol(S), loss = 1 - exp(-|L^-1 y|^2 / 2) / prod diag L. */
#define SX_SAT_MAX_DIM (SX_MAX_NS + 1)
typedef struct sx_sat_cost {
    int32_t trig_idx;                                /* -1: no augmentation; else 0 .. n_s-1 */
    int32_t rank;                                    /* k, 1 .. n_a */
    double target[SX_SAT_MAX_DIM];                   /* z [n_a] */
    double v[SX_SAT_MAX_DIM * SX_SAT_MAX_DIM];       /* V [n_a x k] row-major, W = V V^T */
} sx_sat_cost;

/* The cost alone, one particle per lane: loss[p] of (mu[p], cov[p]), p < P (dev [P x n_s], [P x n_s x n_s], [P]).  A
 * non-finite loss is stored as NaN and sets SX_STATUS_NAN in *status (dev int32, or-ed into).
 * SX_ERR_ARG (before any device access) for null pointers, n_s outside 1 .. SX_MAX_NS, P <= 0, trig_idx outside
 * -1 .. n_s-1, rank outside 1 .. n_a, a non-finite constant. */
int sx_sat_cost_eval(const sx_sat_cost* cost, int n_s, int P, const double* mu, const double* cov, double* loss,
                     int32_t* status, void* stream);

/* sx_cem_perf_rollout_taylor, sx_cem_perf_rollout_taylor_multi and sx_cem_cautious_rollout with the saturating cost as the
 * objective: obj_cost = sum_t loss(mu_{t+1}, Sigma_{t+1}) over the (mu, Sigma) the step holds (generic_cost: stage and
 * terminal cost are the same function); env->obj_mode is not read.  Everything else the parent entry computes is the
 * parent's, bit for bit.  With propagate = 0 the cautious rollout prices Sigma_{t+1} = diag(var_t).  A non-finite loss sets
 * SX_STATUS_NAN and makes the particle's objective NaN.  The cost's constants travel as a kernel argument: the launch is
 * the form the parent's _form query reports, with the parent's LDS plan and limits.
 * SX_ERR_ARG (before any device access) for a NULL cost, trig_idx outside -1 .. n_s-1, rank outside 1 .. n_a, a non-finite
 * constant, and whatever the parent entry refuses (but for obj_mode); SX_ERR_UNSUPPORTED exactly where the parent answers it. */
int sx_cem_perf_rollout_taylor_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E, int P, int H,
                                   int n_perf, int r, const double* x0, const double* safe_actions, const double* tail_mean,
                                   const double* tail_std, const double* tail_noise, double* rows, double* obj_cost,
                                   double* con_cost, double* perf_traj, double* perf_sigma, double* perf_cov,
                                   int terminal_safety, int32_t* status, void* stream);
int sx_cem_perf_rollout_taylor_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env,
                                         const sx_sat_cost* cost, int E, int P, int H, int n_perf, int r, const double* x0,
                                         const double* safe_actions, const double* tail_mean, const double* tail_std,
                                         const double* tail_noise, double* rows, double* obj_cost, double* con_cost,
                                         double* perf_traj, double* perf_sigma, double* perf_cov, int terminal_safety,
                                         int32_t* status, void* stream);
int sx_cem_cautious_rollout_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E, int P, int T,
                                const double* x0, const double* mean, const double* std, const double* noise, double* rows,
                                double* obj_cost, double* con_cost, double* traj, double* sigma, double* cov,
                                double* margins, int propagate, int32_t* status, void* stream);
/* sx_cem_cautious_rollout_multi with the saturating cost: one cost for all problems, everything else the multi-model
 * parent's, bit for bit; the form is the one sx_cem_cautious_rollout_multi_form reports.  Replaces: the n_scenarios
 * CautiousMPC solvers of the reference's cart-pole configs, run one after another (episode_runner.py:40-123 with the cost of
 * defaultconfig_episode.py:113-159). */
int sx_cem_cautious_rollout_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env,
                                      const sx_sat_cost* cost, int E, int P, int T, const double* x0, const double* mean,
                                      const double* std, const double* noise, double* rows, double* obj_cost,
                                      double* con_cost, double* traj, double* sigma, double* cov, double* margins,
                                      int propagate, int32_t* status, void* stream);

/* ---- The saturating cost on the safety trajectory ----------------------------------------------------------------------------
 * sx_cem_rollout, sx_cem_rollout_elites and their _multi forms with the saturating cost as the objective, priced on the
 * safety ellipsoids: obj_cost = sum_{t=1..H} loss(p_t, Q_t), every centre read as a mean and every shape matrix as a
 * covariance -- what a SafeMPC without a performance trajectory hands its solver (defaultconfig_episode.py:150-157:
 * generic_cost over p_all, q_all).  env->obj_mode is not read, not even to reject an odd value.  actions, traj, sigma,
 * con_cost, status and the refit are the streaming kernel's of the parent entry, bit for bit.  A non-finite loss sets
 * SX_STATUS_NAN and makes the particle's objective NaN.  Arguments as the parent entry's with the cost behind env;
 * sx_cem_rollout_sat takes no workspace.  The cost's constants travel as a kernel argument: the LDS plan is the parent's.
 * The streaming kernel only: the resident forms and the workspace path (SX_FORM_RH, SX_FORM_RW, SX_FORM_BIG) are not served.
 * SX_ERR_ARG (before any device access) for whatever the parent entry answers it for, a NULL cost, trig_idx outside
 * -1 .. n_s-1, rank outside 1 .. n_a, a non-finite constant; SX_ERR_UNSUPPORTED (before any launch) for a shape without a
 * kernel, m outside 1 .. SX_MAX_M, a training set on the workspace path or fitting neither streaming form, and from the
 * elite-row entries beyond 2 H n_u <= 256 (1 + n_s). */
int sx_cem_rollout_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E, int P, int H,
                       const double* x0, const double* q0, const double* mean, const double* std, const double* noise,
                       double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost, int32_t* status,
                       void* stream);
int sx_cem_rollout_elites_sat(const sx_gp_model* model, const sx_env* env, const sx_sat_cost* cost, int E, int P, int H,
                              const double* x0, const double* q0, const double* elite_rows, int k, const double* noise,
                              double* actions, double* traj, double* sigma, double* obj_cost, double* con_cost,
                              int32_t* status, double* mean_out, double* std_out, void* stream);
int sx_cem_rollout_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_sat_cost* cost, int E,
                             int P, int H, const double* x0, const double* q0, const double* mean, const double* std,
                             const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                             double* con_cost, int32_t* status, void* stream);
int sx_cem_rollout_elites_sat_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_sat_cost* cost,
                                    int E, int P, int H, const double* x0, const double* q0, const double* elite_rows, int k,
                                    const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                                    double* con_cost, int32_t* status, double* mean_out, double* std_out, void* stream);
/* The form sx_cem_rollout_sat launches for this model and H (no launch, no device access): SX_FORM_STREAM or SX_FORM_BYOUT,
 * or < 0 for bad arguments and wherever the entry would answer SX_ERR_UNSUPPORTED for the model: the contract of
 * sx_cem_rollout_starts_form.  The _multi entries launch what sx_cem_rollout_multi_form reports. */
int sx_cem_rollout_sat_form(const sx_gp_model* model, int H);

/* ---- The SafeMPC constraint set on the safety trajectory ---------------------------------------------------------------------
 * What the reference's SafeMPC constrains beside the terminal safe set (safempc_simple.py:325-396, _generate_control_constraint
 * :492-536), as penalties of the CEM rollout.  Steps t = 0 .. H-1; (p_t, Q_t) is the ellipsoid step t starts from (Q_0 = q0,
 * or a point), u_t the row's action (k_ff), (p_{t+1}, Q_{t+1}) what the step reaches, K = env->k_fb.
 *   feedback bounds (ctrl_ellipsoid = 1): a step that starts from an ellipsoid is ellipsoid-violated where the control
 *       ellipsoid (u_t, Q_u = K Q_t K^T) is not certified inside the action box: some
 *       +-u_c + sqrt(Q_u[c][c]) -+ bound_c >= 0, the polytope test over h = [I; -I], h_vec = [u_max; -u_min], c_safety = 1
 *       (a NaN distance is not a violation).  The step costs SX_ACTION_VIOLATION_COST ONCE if it is box-violated (the
 *       parent's strict test) or ellipsoid-violated.  A step that starts from a point keeps the box test alone.
 *   obstacle polytope (m_obs > 0): every step with t + 1 < H whose (p_{t+1}, Q_{t+1}) is not certified inside
 *       h_mat_obs x <= h_obs (some h_j . p + sqrt(h_j^T Q h_j) - h_obs_j >= 0) costs SX_STATE_VIOLATION_COST, on top of
 *       whatever env->con_mode charges for the safe polytope.  The terminal ellipsoid is not checked against these rows.
 *   m_obs = 0 and ctrl_ellipsoid = 0: the empty set; every output is the streaming parent's bit for bit. */
typedef struct sx_con_set {
    int32_t m_obs;                            /* obstacle rows, 0 .. SX_MAX_M */
    int32_t ctrl_ellipsoid;                   /* 0 | 1: the feedback bounds */
    double h_mat_obs[SX_MAX_M * SX_MAX_NS];   /* [m_obs x n_s] row-major, rows n_s apart (as sx_env.h_mat) */
    double h_obs[SX_MAX_M];
} sx_con_set;

/* The set's cost of one step alone, one particle per lane (the step-by-step path's and the tests'):
 *   con_step[p] = SX_ACTION_VIOLATION_COST if u[p] is box-violated, or q_start is given, ctrl_ellipsoid is set and
 *                 (u[p], K q_start[p] K^T) is ellipsoid-violated
 *               + SX_STATE_VIOLATION_COST if check_obstacle != 0 and (p_next[p], q_next[p]) violates the obstacle rows
 * u dev [P x n_u], q_start dev [P x n_s x n_s] or NULL (the step starts from a point), p_next dev [P x n_s], q_next dev
 * [P x n_s x n_s] (both may be NULL with check_obstacle = 0 or m_obs = 0), con_step dev [P] (overwritten).  Reads n_s,
 * n_u, k_fb, u_min, u_max of env.  No status word: nothing here fails.
 * SX_ERR_ARG (before any device access) for null pointers, P <= 0, n_s outside 1 .. SX_MAX_NS, n_u outside
 * 1 .. SX_MAX_NU, m_obs outside 0 .. SX_MAX_M, ctrl_ellipsoid outside {0, 1}, a non-finite constant in the rows in use. */
int sx_conset_eval(const sx_env* env, const sx_con_set* cons, int P, const double* u, const double* q_start,
                   const double* p_next, const double* q_next, int check_obstacle, double* con_step, void* stream);

/* sx_cem_rollout and sx_cem_rollout_elites with the constraint set in the step: con_cost carries the set's costs beside the
 * parent's; actions, traj, sigma, obj_cost, status and the refit are those of the same launch with the empty set, bit for
 * bit.  cost == NULL: the objective of env->obj_mode, and the launch with the empty set is the streaming kernel of the parent
 * entry bit for bit.  Otherwise the saturating cost on the safety ellipsoids, exactly as sx_cem_rollout_sat (env->obj_mode is
 * not read) -- what the reference's n_perf = 0 cart-pole configs solve.  Arguments as the parent entry's with (cons, cost)
 * behind env; no workspace.  The set's constants travel as a kernel argument: the LDS plan is the parent's.
 * The streaming kernel only: the resident forms and the workspace path are not served.
 * SX_ERR_ARG (before any device access) for whatever the parent entry answers it for, a NULL cons, m_obs outside
 * 0 .. SX_MAX_M, ctrl_ellipsoid outside {0, 1}, a non-finite constant in the rows in use, and a cost sx_cem_rollout_sat
 * refuses; SX_ERR_UNSUPPORTED exactly where sx_cem_rollout_sat answers it. */
int sx_cem_rollout_cons(const sx_gp_model* model, const sx_env* env, const sx_con_set* cons, const sx_sat_cost* cost, int E,
                        int P, int H, const double* x0, const double* q0, const double* mean, const double* std,
                        const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                        double* con_cost, int32_t* status, void* stream);
int sx_cem_rollout_elites_cons(const sx_gp_model* model, const sx_env* env, const sx_con_set* cons, const sx_sat_cost* cost,
                               int E, int P, int H, const double* x0, const double* q0, const double* elite_rows, int k,
                               const double* noise, double* actions, double* traj, double* sigma, double* obj_cost,
                               double* con_cost, int32_t* status, double* mean_out, double* std_out, void* stream);
/* The form sx_cem_rollout_cons launches for this model and H: the contract of sx_cem_rollout_sat_form. */
int sx_cem_rollout_cons_form(const sx_gp_model* model, int H);

/* sx_cem_rollout_multi and sx_cem_rollout_elites_multi with the constraint set in the step: E problems with a GP each behind
 * their device table (sx_gp_model_table) and ONE set shared by all of them, as they share env.  Arguments as the parent
 * entry's with (cons, cost) behind env; status dev int32 [E].  cost == NULL: the objective of env->obj_mode, and the launch
 * with the empty set is sx_cem_rollout[_elites]_multi bit for bit; otherwise the saturating cost, and the launch with the
 * empty set is sx_cem_rollout[_elites]_sat_multi bit for bit.  Problem e of a launch is sx_cem_rollout[_elites]_cons of
 * model e alone, bit for bit where that launch has the same form.
 * SX_ERR_ARG (before any device access), checked in this order: whatever sx_cem_rollout[_elites]_multi answers it for (a NULL
 * table, a missing elite_rows, models of differing shape or not of env's), then a NULL cons, m_obs outside 0 .. SX_MAX_M,
 * ctrl_ellipsoid outside {0, 1}, a non-finite constant in the rows in use, then a cost sx_cem_rollout_sat refuses;
 * SX_ERR_UNSUPPORTED exactly where sx_cem_rollout_sat_multi answers it. */
int sx_cem_rollout_cons_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_con_set* cons,
                              const sx_sat_cost* cost, int E, int P, int H, const double* x0, const double* q0,
                              const double* mean, const double* std, const double* noise, double* actions, double* traj,
                              double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream);
int sx_cem_rollout_elites_cons_multi(const sx_gp_model* models, const void* table, const sx_env* env, const sx_con_set* cons,
                                     const sx_sat_cost* cost, int E, int P, int H, const double* x0, const double* q0,
                                     const double* elite_rows, int k, const double* noise, double* actions, double* traj,
                                     double* sigma, double* obj_cost, double* con_cost, int32_t* status, double* mean_out,
                                     double* std_out, void* stream);
/* The form sx_cem_rollout_cons_multi launches for these models and H: the contract of sx_cem_rollout_multi_form. */
int sx_cem_rollout_cons_multi_form(const sx_gp_model* models, int E, int H);

/* sx_cem_rollout_starts with the constraint set in the step (static exploration with the reference's constraints:
 * StaticSafeMPCExploration optimises [p_0, u_0, k_ff] with the gain a fixed parameter, so the set is its NLP's constraints
 * term for term).  Arguments as sx_cem_rollout_starts' with cons behind env.  A particle starts from a point, so step 0 pays
 * the box test alone, steps t >= 1 the feedback bounds, every (p_{t+1}, Q_{t+1}) with t + 1 < H the obstacle rows; and the
 * start x0 itself (a point, Q = 0) costs SX_STATE_VIOLATION_COST once where it violates the obstacle rows (some
 * h_j . x0 - h_obs_j >= 0; a NaN distance is not a violation), independent of the safe-polytope cost of the start: a start
 * outside both pays twice.  The reference bounds p_1 .. p_{H-1} only; the start test is this library's own (DESIGN.md section
 * 7).  rows, traj, sigma, obj_cost and status are those of the same launch with the empty set, bit for bit; with the empty
 * set (m_obs = 0, ctrl_ellipsoid = 0) every output is sx_cem_rollout_starts'.  The objective is env->obj_mode's.
 * The plan is sx_cem_rollout_starts': sx_cem_rollout_starts_form answers for both entries (the set's constants travel as a
 * kernel argument, the LDS plan is the parent's).
 * SX_ERR_ARG (before any device access) for whatever sx_cem_rollout_starts answers it for, then a NULL cons, m_obs outside
 * 0 .. SX_MAX_M, ctrl_ellipsoid outside {0, 1}, a non-finite constant in the rows in use; SX_ERR_UNSUPPORTED (before any
 * launch) exactly where sx_cem_rollout_starts answers it.
 * Replaces: the constraint groups of StaticSafeMPCExploration's NLP (safempc_exploration.py:100-233). */
int sx_cem_rollout_starts_cons(const sx_gp_model* model, const sx_env* env, const sx_con_set* cons, int E, int P, int H,
                               const double* mean, const double* std, const double* noise, double* rows, double* traj,
                               double* sigma, double* obj_cost, double* con_cost, int32_t* status, void* stream);

/* sx_cem_rollout_starts over E problems with an exact GP each in ONE launch (static exploration of several scenarios at
 * once, every scenario with its restarts): problem e is rolled out under models[e] and entry e of `table`
 * (sx_gp_model_table over the same E models, unchanged); a scenario with R restarts stands R times in `models` and in the
 * table.  All models share (n_s, n_u) and the env.  Buffers are sx_cem_rollout_starts' ([E x L] mean and std, so that every
 * problem has a start distribution of its own); status holds one word PER PROBLEM.  Problem e's outputs are those of
 * sx_cem_rollout_starts(models + e, E = 1) on its slice of the buffers, bit for bit where that model's own form
 * (sx_cem_rollout_starts_form) is the launch's; where another model moves the launch to SX_FORM_BYOUT, con_cost and
 * status are the same and the rest agrees to the rollout's rounding ("the multi-model form").
 * SX_ERR_ARG (before any device access) for null models / table / env / rows / cost / status pointers, non-positive sizes,
 * noise without mean / std, any model whose (n_s, n_u) differ from env's or whose training set is empty; SX_ERR_UNSUPPORTED
 * (before any launch) exactly where sx_cem_rollout_starts_multi_form answers < 0, or env->m > SX_MAX_M.
 * Replaces: the per-scenario loop over StaticSafeMPCExploration's NLP solves (sacred_helper.py's n_scenarios runs of
 * safempc_exploration.py:281-330). */
int sx_cem_rollout_starts_multi(const sx_gp_model* models, const void* table, const sx_env* env, int E, int P, int H,
                                const double* mean, const double* std, const double* noise, double* rows, double* traj,
                                double* sigma, double* obj_cost, double* con_cost, int32_t* status /* [E] */, void* stream);
/* sx_cem_rollout_starts_multi with the constraint set of sx_cem_rollout_starts_cons in the step: ONE set, shared by all
 * problems.  With the empty set every output is sx_cem_rollout_starts_multi's.  SX_ERR_ARG as sx_cem_rollout_starts_multi,
 * then as sx_cem_rollout_starts_cons for the set; SX_ERR_UNSUPPORTED where sx_cem_rollout_starts_multi answers it.
 * Replaces: as sx_cem_rollout_starts_multi, with the constraint groups of safempc_exploration.py:100-233. */
int sx_cem_rollout_starts_cons_multi(const sx_gp_model* models, const void* table, const sx_env* env,
                                     const sx_con_set* cons, int E, int P, int H, const double* mean, const double* std,
                                     const double* noise, double* rows, double* traj, double* sigma, double* obj_cost,
                                     double* con_cost, int32_t* status /* [E] */, void* stream);
/* The form sx_cem_rollout_starts[_cons]_multi launch for these models and H (no launch, no device access): the fold of
 * sx_cem_rollout_starts_form over the models -- SX_FORM_BYOUT where any model needs it, < 0 where any model has no form or
 * for bad arguments.  The contract of sx_cem_rollout_multi_form.
 * Replaces: nothing in the reference. */
int sx_cem_rollout_starts_multi_form(const sx_gp_model* models, int E, int H);

/* The ONE device -> host hand-off of a solve, packed by one launch: out dev double [G + E + 1 + E*row_len] =
 *   [status words of the G ranks | best_ok[E] | 1.0 if any of the `q_count` doubles at `q_block` is non-zero | best [E x row_len]]
 * (q_block may be NULL: the flag is 0).  The caller copies `out` to the host once and reads everything from it.
 * Replaces: the synchronisations of CemSafeMPC.get_action (safempc_cem.py:231-263): PQFlattener's `q.nonzero()` scan
 * (:69-71), the optimiser's return value and the failure check of gp_reachability_pytorch.py:149-153, each a trip of its own
 * in the reference. */
int sx_cem_pack_result(int G, int E, int row_len, const int32_t* status, const int32_t* best_ok, const double* q_block,
                       int64_t q_count, const double* best, double* out, void* stream);

/* 1 if sx_cem_rank_refit ranks E problems of P candidates by counting over the whole chip (elite rows in rank order), 0 if
 * by one workgroup per problem (best first, then index order).  Depends on (E, P) only.  A caller that moves the refit into
 * the next rollout (sx_cem_rollout_elites) does so where this returns 1: with many problems at once the one-workgroup
 * kernels refit side by side and the rollout's prologue has nothing to gain. */
int sx_cem_rank_counts(int E, int P);

/* Ranking + elite refit for E problems.  One or two problems of up to 8192 candidates are ranked by counting, spread over
 * the whole chip (csrc/sx_rank_count.hpp: needs elite_rows whenever mean is wanted); anything else by one workgroup per
 * problem (csrc/sx_rank.hpp).  The choice depends on (E, P) only.
 * Candidates c = 0..P-1 of problem e have con = con_cost[(e*P+c)*cost_stride], obj likewise, and an action row of
 * `row_len` doubles at actions + (e*P+c)*act_stride.  Order: lexicographic (con, obj, c); NaN sorts last.
 *   elite_idx  dev int32 [E x k]            elite indices: the best first, the others in a deterministic but unspecified order (may be NULL)
 *   elite_rows dev [E x k x (2 + row_len)]  [con, obj, actions...] of the elites, same order (may be NULL) -- the buffer
 *                                           that is all-reduced across GPUs
 *   mean, std  dev [E x row_len]            refit (unbiased std; 0 when k == 1)  (may be NULL: no refit)
 *   best       dev [E x row_len]            first-ranked action sequence (may be NULL)
 *   best_ok    dev int32 [E]                1 if the first-ranked candidate has con == 0 (may be NULL)
 * Replaces: elite selection / refit / "best feasible or None" of ConstrainedCemMpc.get_actions (safempc_cem.py:235,
 * test_safempc_cem.py:83-148). */
int sx_cem_rank_refit(int E, int P, int k, int row_len, const double* con_cost, const double* obj_cost,
                      int64_t cost_stride, const double* actions, int64_t act_stride, int32_t* elite_idx,
                      double* elite_rows, double* mean, double* std, double* best, int32_t* best_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SX_AMD_H */
