"""Reference for sx_gp_drop (tests/test_gp_drop_host.py, tests/test_gpu_gp_drop.py): the k oldest rows removed from an exact
GP's factorisation, stated in numpy in float64 and np.longdouble, none of the project's kernels.

Per output, given W = L^-1 with L L^T = K + noise I for N rows, partitioned after the first k, W = [ W11 0 ; W21 W22 ], and the
m = N - k kept rows' targets y2:
    K22 = L22 L22^T + L21 L21^T,  L11 = W11^-1,  V = L22^-1 L21 = -W21 L11 [m x k],  W' = chol(I + V V^T)^-1 W22,
    alpha' = W'^T (W' y2),  logdet' = -sum log diag W'.
chol(I + V V^T)^-1 is applied as k rank-1 stages in one pass over the rows: with U = V, t_s = 1, sV = 0, sX = 0, for row
i = 0 .. m - 1 and stage s = 0 .. k - 1
    u = U[i,s];  tn = t_s + u^2;  dinv = sqrt(t_s / tn);  coef = u / sqrt(tn t_s)
    U[i,q>s] = (U[i,q] - u sV[s][q]) dinv;  sV[s][q] += coef U[i,q];   X[i,c<=i] = (X[i,c] - u sX[s][c]) dinv;  sX[s][c] += coef X[i,c]
    t_s = tn.
No hyper-parameters and no inputs are needed.  The factorisation of the N rows comes from tests/warm_path_reference.py."""
from typing import NamedTuple

import numpy as np

import warm_path_reference as R


class Dropped(NamedTuple):
    linv: np.ndarray     # [n_s x m x m]
    alpha: np.ndarray    # [n_s x m]
    logdet: np.ndarray   # [n_s]


def tail(p, k):
    """The problem of p's rows beyond the first k, the hyper-parameters unchanged."""
    return R._frozen(R.Problem(('tail', k) + tuple(p.key), p.n_s, p.n_u, p.X[k:].copy(), p.Y[k:].copy(), p.ls, p.s, p.noise))


def window(p, lo, hi):
    """The problem of p's rows lo .. hi - 1."""
    return R._frozen(R.Problem(('window', lo, hi) + tuple(p.key), p.n_s, p.n_u, p.X[lo:hi].copy(), p.Y[lo:hi].copy(), p.ls,
                               p.s, p.noise))


def drop_output(W, y2, k, dtype, l11='inverse', K11=None):
    """One output: (W', alpha', logdet') from W [N x N] and the kept rows' targets y2 [N - k], in `dtype`.  l11: L11 as the
    inverse of W11 ('inverse'), or ('chol') as the Cholesky factor of K11, the dropped rows' own kernel block."""
    W, y2 = np.asarray(W, dtype), np.asarray(y2, dtype)
    n = W.shape[0]
    m = n - k
    W11 = W[:k, :k]
    if not (np.isfinite(W11.astype(R.F64)).all() and (np.diag(W11) > 0).all()):
        raise np.linalg.LinAlgError('W11 is not the inverse of a Cholesky factor')
    L11 = R.tri_inverse_ld(W11) if l11 == 'inverse' else R.cholesky_ld(np.asarray(K11, dtype))
    U = -(W[k:, :k] @ L11)                                  # V [m x k]
    X = W[k:, k:].copy()
    t = np.ones(k, dtype)
    sV = np.zeros((k, k), dtype)
    sX = np.zeros((k, m), dtype)
    for i in range(m):
        for s in range(k):
            u = U[i, s]
            tn = t[s] + u * u
            if not np.isfinite(R.F64(tn)):
                raise np.linalg.LinAlgError(f'row {i} stage {s}: t + u^2 is not finite')
            dinv, coef = np.sqrt(t[s] / tn), u / np.sqrt(tn * t[s])
            U[i, s + 1:] = (U[i, s + 1:] - u * sV[s, s + 1:]) * dinv
            sV[s, s + 1:] += coef * U[i, s + 1:]
            X[i, :i + 1] = (X[i, :i + 1] - u * sX[s, :i + 1]) * dinv
            sX[s, :i + 1] += coef * X[i, :i + 1]
            t[s] = tn
    alpha = X.T @ (X @ y2)
    return X, alpha, -np.log(np.diag(X)).sum()


def drop(p, k, dtype=R.F64, start=None, l11='inverse'):
    """All outputs: p's N rows factorised by warm_path_reference in `dtype` (or `start`, anything with .linv), then the
    first k rows dropped in one step."""
    if start is None:
        start = R.Reference(p, dtype)
    outs = []
    for d in range(p.n_s):
        K11 = R.kmat(window(p, 0, k), d, dtype) if l11 == 'chol' else None
        outs.append(drop_output(start.linv[d], p.Y[k:, d], k, dtype, l11, K11))
    return Dropped(np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.array([o[2] for o in outs], dtype))
