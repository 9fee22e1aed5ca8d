"""Reference for the exact-GP warm path (tests/test_gpu_warm_path.py, tests/test_warm_path_reference_host.py): plain numpy,
no GPU, none of the project's kernels, and written independently of oracle/gp.py.

One output d of an exact RBF GP:  K = s exp(-1/2 sum_j ((x_ij - x_kj) / l_j)^2) + noise I = L L^T,  W = L^-1,
alpha = K^-1 y,  logdet = sum log diag L,  mll = -1/2 y.alpha - logdet - N/2 log 2 pi,
d mll / d theta = 1/2 tr((alpha alpha^T - K^-1) dK/dtheta)  for theta = (l_0 .. l_{D-1}, s, noise)  (closed form, no autograd),
d var / d z_j = 2 sum_i v_i k*_i (z_j - x_ij) / l_j^2  with  v = W^T W k*,
d^2 mean / dz dz^T = sum_i alpha_i k*_i [g_i g_i^T - diag(1 / l^2)]  with  g_i = (z - x_i) / l^2.

Two precisions: float64 through LAPACK (any N), and np.longdouble through a hand-written column Cholesky and forward
substitution (N <= LD_MAX_N: numpy has no BLAS for it).  The long-double result is the truth the tests measure both
LAPACK's and the kernels' float64 error against; where long double is no wider than double the tests cannot do that
and say so (HAVE_LD)."""
import functools
from typing import NamedTuple

import numpy as np
import scipy.linalg as sla

F64, LD = np.float64, np.longdouble
EPS = float(np.finfo(F64).eps)
HAVE_LD = np.finfo(LD).eps < 1e-18
LD_MAX_N = 410
SHAPES = ((1, 1), (2, 1), (3, 1), (2, 2), (4, 2))     # every entry of the warm path takes them
WIDE_SHAPES = ((2, 4), (1, 5))                        # only the fit and the multi entries do (n_s + n_u <= 6)
RATIOS = (1e-2, 1e-4, 1e-6)                           # noise / outputscale


class Problem(NamedTuple):
    key: tuple           # names the problem (the cache key of reference())
    n_s: int
    n_u: int
    X: np.ndarray        # [N x D]
    Y: np.ndarray        # [N x n_s]
    ls: np.ndarray       # [n_s x D]
    s: np.ndarray        # [n_s]
    noise: np.ndarray    # [n_s]


@functools.lru_cache(maxsize=None)
def problem(n_s, n_u, n, ratio=1e-2):
    """X uniform in [-1, 1]^D, lengthscales in [0.4, 1.5], outputscale in [0.5, 2], Y smooth plus 1 % noise,
    noise = ratio * outputscale.  One fixed problem per (shape, N, ratio)."""
    rng = np.random.default_rng([n_s, n_u, n, int(round(-np.log10(ratio)))])
    D = n_s + n_u
    X = rng.uniform(-1.0, 1.0, size=(n, D))
    Y = np.stack([np.sin(X @ rng.normal(size=D)) + 0.1 * X[:, d % D] for d in range(n_s)], 1) \
        + 0.01 * rng.normal(size=(n, n_s))
    ls = rng.uniform(0.4, 1.5, size=(n_s, D))
    s = rng.uniform(0.5, 2.0, size=n_s)
    return _frozen(Problem((n_s, n_u, n, ratio), n_s, n_u, X, Y, ls, s, ratio * s))


def not_pd_problem(n, a, b, n_s=2, n_u=1):
    """K + noise I whose Cholesky factorisation meets its first non-positive pivot at row b exactly: the points lie on
    a grid 8 lengthscales apart (K = s I to 1e-14), noise = -0.01 s keeps the diagonal at 0.99 s, and row b repeats row
    a < b, so that pivot b is 0.99 s - s / 0.99 < 0."""
    assert 0 <= a < b < n
    D = n_s + n_u
    side = int(np.ceil(n ** (1.0 / D)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * D, indexing='ij'), -1).reshape(-1, D)[:n]
    X = 8.0 * grid.astype(F64)
    X[b] = X[a]
    rng = np.random.default_rng([n, a, b])
    s = rng.uniform(0.5, 2.0, size=n_s)
    return _frozen(Problem(('not_pd', n, a, b, n_s, n_u), n_s, n_u, X, rng.normal(size=(n, n_s)), np.ones((n_s, D)), s,
                           -0.01 * s))


def _frozen(p):
    for a in p[3:]:
        a.setflags(write=False)
    return p


def sqdist(A, B, ls_d, dtype=F64):
    """[len(A) x len(B)]  sum_j ((a_j - b_j) / l_j)^2, from the differences (no expanded square)."""
    A, B, l = np.asarray(A, dtype), np.asarray(B, dtype), np.asarray(ls_d, dtype)
    q = np.zeros((A.shape[0], B.shape[0]), dtype)
    for j in range(A.shape[1]):
        df = (A[:, j, None] - B[None, :, j]) / l[j]
        q += df * df
    return q


def kstar(p, d, z, dtype=F64):
    """[P x N]  k_d(z, X)"""
    return dtype(p.s[d]) * np.exp(-0.5 * sqdist(z, p.X, p.ls[d], dtype))


def kmat(p, d, dtype=F64):
    """K_d + noise_d I"""
    K = kstar(p, d, p.X, dtype)
    K[np.diag_indices_from(K)] += dtype(p.noise[d])
    return K


def cholesky_ld(K):
    """Lower Cholesky factor, a column at a time (left-looking), in K's own precision.  LinAlgError at the first pivot
    that is not positive."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        v = K[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f'pivot {j} is not positive')
        L[j:, j] = v / np.sqrt(v[0])
    return L


def tri_inverse_ld(L):
    """W = L^-1 by forward substitution, a row at a time: W[i] = (e_i - L[i, :i] W[:i]) / L[i, i]."""
    n = L.shape[0]
    W = np.zeros_like(L)
    for i in range(n):
        row = -(L[i, :i] @ W[:i, :i + 1])
        row[i] += 1
        W[i, :i + 1] = row / L[i, i]
    return W


class Output:
    """The factorisation of one output in one precision, and what follows from it."""

    def __init__(self, p, d, dtype):
        self.p, self.d, self.dtype = p, d, dtype
        self.K = kmat(p, d, dtype)
        y = self.y = np.asarray(p.Y[:, d], dtype)
        n = self.n = len(y)
        if dtype is F64:
            self.L = np.linalg.cholesky(self.K)
            self.W = sla.solve_triangular(self.L, np.eye(n), lower=True)
            self.alpha = sla.cho_solve((self.L, True), y)
        else:
            assert n <= LD_MAX_N, 'the long-double reference is a python loop: small N only'
            self.L = cholesky_ld(self.K)
            self.W = tri_inverse_ld(self.L)
            self.alpha = self.W.T @ (self.W @ y)
        self.logdet = np.log(np.diag(self.L)).sum()
        two_pi = 8 * np.arctan(dtype(1))
        self.mll = -(y @ self.alpha) / 2 - self.logdet - dtype(n) / 2 * np.log(two_pi)

    @functools.cached_property
    def grad(self):
        """[D + 2]  d mll / d (l_0 .. l_{D-1}, s, noise) = 1/2 tr((alpha alpha^T - K^-1) dK/dtheta)"""
        p, d, dtype, n = self.p, self.d, self.dtype, self.n
        Kinv = sla.cho_solve((self.L, True), np.eye(n)) if dtype is F64 else self.W.T @ self.W
        G = np.outer(self.alpha, self.alpha) - Kinv
        Kf = self.K.copy()
        Kf[np.diag_indices(n)] -= dtype(p.noise[d])
        GK = G * Kf
        out = np.empty(p.X.shape[1] + 2, dtype)
        for c in range(p.X.shape[1]):
            l = dtype(p.ls[d, c])
            x = np.asarray(p.X[:, c], dtype)
            df = x[:, None] - x[None, :]
            out[c] = (GK * (df * df)).sum() / (l * l * l) / 2
        out[-2] = GK.sum() / dtype(p.s[d]) / 2
        out[-1] = np.trace(G) / 2
        return out


class Reference:
    """All outputs of a problem in one precision: linv [n_s x N x N], alpha [n_s x N], logdet, mll [n_s],
    grad [n_s x (D + 2)], K (a list of [N x N])."""

    def __init__(self, p, dtype):
        self.p, self.dtype = p, dtype
        self.out = [Output(p, d, dtype) for d in range(p.n_s)]
        self.linv = np.stack([o.W for o in self.out])
        for d, o in enumerate(self.out):
            o.W = self.linv[d]                      # one copy
        self.alpha = np.stack([o.alpha for o in self.out])
        self.logdet = np.array([o.logdet for o in self.out], dtype)
        self.mll = np.array([o.mll for o in self.out], dtype)

    @property
    def K(self):
        return [o.K for o in self.out]

    @functools.cached_property
    def grad(self):
        return np.stack([o.grad for o in self.out])


_references = {}


def reference(p, long_double=False):
    """Cached: computed once per problem and precision, shared by the tests, never modified."""
    key = (p.key, bool(long_double))
    if key in _references:
        return _references[key]
    ref = Reference(p, LD if long_double else F64)
    if p.X.shape[0] <= 1100:                        # the two largest problems serve one test each
        _references[key] = ref
    return ref


def variance_jacobian(p, linv, z, dtype=F64):
    """[P x n_s x D]  d var_d / d z from a given W = linv [n_s x N x N] (taken as exact), evaluated in `dtype`.  W is
    converted a slab of rows at a time: v = W^T (W k*) = sum over slabs of W_b^T (W_b k*)."""
    z = np.asarray(z, dtype)
    n, D = p.X.shape
    out = np.empty((z.shape[0], p.n_s, D), dtype)
    for d in range(p.n_s):
        ks = kstar(p, d, z, dtype)                                     # [P x N]
        v = np.zeros_like(ks)
        for r0 in range(0, n, 512):
            Wb = np.asarray(linv[d, r0:r0 + 512], dtype)
            v += (Wb @ ks.T).T @ Wb
        w = v * ks
        diff = z[:, None, :] - np.asarray(p.X, dtype)[None, :, :]      # [P x N x D]
        l = np.asarray(p.ls[d], dtype)
        out[:, d, :] = 2 * np.einsum('pi,pij->pj', w, diff) / (l * l)
    return out


def mean_hessian(p, alpha, z, dtype=F64):
    """[P x n_s x D x D]  d^2 mean_d / dz dz^T from a given alpha [n_s x N] (taken as exact), evaluated in `dtype`."""
    z = np.asarray(z, dtype)
    D = p.X.shape[1]
    out = np.empty((z.shape[0], p.n_s, D, D), dtype)
    for d in range(p.n_s):
        l = np.asarray(p.ls[d], dtype)
        w = kstar(p, d, z, dtype) * np.asarray(alpha[d], dtype)[None, :]
        g = (z[:, None, :] - np.asarray(p.X, dtype)[None, :, :]) / (l * l)
        out[:, d] = np.einsum('pi,pij,pil->pjl', w, g, g) - w.sum(1)[:, None, None] * np.diag(1 / (l * l))[None]
    return out


def residuals(K, W, alpha, y):
    """(max |W K W^T - I|,  max |K alpha - y| / max |y|)  of one output, in float64."""
    K, W = np.asarray(K, F64), np.asarray(W, F64)
    r1 = np.abs(W @ K @ W.T - np.eye(K.shape[0])).max()
    r2 = np.abs(K @ np.asarray(alpha, F64) - y).max() / np.abs(y).max()
    return float(r1), float(r2)


def cond2(K):
    """2-norm condition number of a symmetric positive definite K (largest over smallest eigenvalue)."""
    ev = np.linalg.eigvalsh(np.asarray(K, F64))
    return float(ev[-1] / ev[0])


def rel_err(q, truth):
    """max |q - truth| / max |truth|  (the e of the tolerance rule), as a float"""
    truth = np.asarray(truth)
    return float(np.abs(np.asarray(q, truth.dtype) - truth).max() / np.abs(truth).max())


def queries(p, P, far=True):
    """P query points [P x D]: a point of the cube, then (P >= 2) a training point itself, then (P >= 3 and `far`) a
    point 40 of the longest lengthscales beyond the cube in every dimension, where every k* underflows."""
    rng = np.random.default_rng([p.X.shape[0], p.n_s, p.n_u, P])
    z = rng.uniform(-1.0, 1.0, size=(P, p.X.shape[1]))
    if P >= 2:
        z[1] = p.X[p.X.shape[0] // 2]
    if P >= 3 and far:
        z[2] = 1.0 + 40.0 * p.ls.max()
    return z


# ---- the problems tests/test_gpu_warm_path.py runs: (n_s, n_u, N, ratio) -------------------------------------------

FIT_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 193, 1023, 1024, 1025)
FIT_SIZES_EVERY_SHAPE = (33, 65, 97, 193)
MLL_SIZES = (1, 33, 65, 96, 97, 193, 1025)
PREDICT_SIZES = (1, 63, 65, 255, 256, 257, 1100)
PREDICT_SHAPES = ((1, 1), (2, 2), (3, 1), (4, 2))
COND_SIZES = (96, 97, 410)
MIX_SIZES = (50, 97, 330)          # (3, 1): one-workgroup, two block columns, six block columns
LIMIT_N, VAR_JAC_LDS_N = 4096, 4160
NOT_PD_CASES = ((90, 5, 70), (200, 2, 5), (200, 3, 195), (65, 10, 64))   # (N, a, b)
NOT_PD_MULTI = (60, 150)           # the healthy neighbours of (200, 3, 195) in a multi launch


def fit_cases():
    """The covering set of (a): every size at (2, 1) and at one other shape, every shape at FIT_SIZES_EVERY_SHAPE."""
    others = [sh for sh in SHAPES + WIDE_SHAPES if sh != (2, 1)]
    cases = []
    for k, n in enumerate(FIT_SIZES):
        cases += [((2, 1), n), (others[k % len(others)], n)]
    cases += [(sh, n) for sh in SHAPES + WIDE_SHAPES for n in FIT_SIZES_EVERY_SHAPE]
    return sorted(set(cases), key=lambda c: (c[1], c[0]))


def all_cases():
    """Every generated problem of the GPU tests, as arguments of problem()."""
    cases = {(*sh, n, 1e-2) for sh, n in fit_cases()}
    cases |= {(1, 1, LIMIT_N, 1e-2), (1, 1, VAR_JAC_LDS_N, 1e-2)}
    cases |= {(2, 1, n, r) for n in COND_SIZES for r in RATIOS} | {(2, 1, 1100, r) for r in RATIOS[1:]}
    cases |= {(*sh, n, 1e-2) for sh in SHAPES + WIDE_SHAPES for n in MLL_SIZES}
    cases |= {(3, 1, n, 1e-2) for n in MIX_SIZES} | {(2, 1, n, 1e-2) for n in NOT_PD_MULTI}
    cases |= {(*sh, n, 1e-2) for sh in PREDICT_SHAPES for n in PREDICT_SIZES}
    return sorted(cases)
