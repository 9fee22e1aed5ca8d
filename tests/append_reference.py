"""Reference for sx_gp_append (tests/test_gp_append_host.py, tests/test_gpu_gp_append.py): the update of an exact GP's
factorisation by k appended rows, stated in numpy in float64 and np.longdouble, none of the project's kernels.

Per output, given X [N x D], W = L^-1 with L L^T = K + noise I, alpha = (K + noise I)^-1 y, logdet = sum log diag L and the
k new rows (X_c, y_c):
    K_c = k(X, X_c),  K_cc = k(X_c, X_c) + noise I,  B = W K_c,  S = K_cc - B^T B = L_s L_s^T,  W_s = L_s^-1,
    W' = [ W 0 ; -W_s B^T W  W_s ],  alpha' = [alpha; 0] + W_bot^T (W_bot y'),  logdet' = logdet + sum log diag L_s.
The factorisation of the first N rows and every kernel value come from tests/warm_path_reference.py."""
from typing import NamedTuple

import numpy as np

import warm_path_reference as R


class Appended(NamedTuple):
    linv: np.ndarray     # [n_s x (N + k) x (N + k)]
    alpha: np.ndarray    # [n_s x (N + k)]
    logdet: np.ndarray   # [n_s]


def head(p, n):
    """The problem of the first n rows of p, the hyper-parameters unchanged."""
    return R._frozen(R.Problem(('head', n) + tuple(p.key), p.n_s, p.n_u, p.X[:n].copy(), p.Y[:n].copy(), p.ls, p.s, p.noise))


def append_output(p, d, n, W, alpha, logdet, dtype, b_dtype=None):
    """Output d of p's N + k rows from the factorisation (W, alpha, logdet) of its first n, in `dtype`.  b_dtype: the
    precision the one product B = W K_c is accumulated in before it is rounded to `dtype` (default: `dtype` itself)."""
    W, alpha = np.asarray(W, dtype), np.asarray(alpha, dtype)
    n2 = p.X.shape[0]
    Xc = p.X[n:]
    y2 = np.asarray(p.Y[:, d], dtype)
    Kc = dtype(p.s[d]) * np.exp(-0.5 * R.sqdist(p.X[:n], Xc, p.ls[d], dtype))            # [N x k]
    Kcc = dtype(p.s[d]) * np.exp(-0.5 * R.sqdist(Xc, Xc, p.ls[d], dtype))
    Kcc[np.diag_indices_from(Kcc)] += dtype(p.noise[d])
    B = W @ Kc if b_dtype is None else (np.asarray(W, b_dtype) @ np.asarray(Kc, b_dtype)).astype(dtype)
    S = Kcc - B.T @ B
    Ls = R.cholesky_ld(S)                         # (in S's own precision; LinAlgError at a pivot that is not positive)
    Ws = R.tri_inverse_ld(Ls)
    W2 = np.zeros((n2, n2), dtype)
    W2[:n, :n] = W
    W2[n:, :n] = -(Ws @ (B.T @ W))
    W2[n:, n:] = Ws
    bot = W2[n:]
    alpha2 = np.concatenate([alpha, np.zeros(n2 - n, dtype)]) + bot.T @ (bot @ y2)
    return W2, alpha2, dtype(logdet) + np.log(np.diag(Ls)).sum()


def append(p, n, dtype=R.F64, start=None, b_dtype=None):
    """All outputs: p's first n rows factorised by warm_path_reference in `dtype` (or `start`, an Appended or a Reference
    of those rows), then the remaining rows appended in one step."""
    if start is None:
        start = R.Reference(head(p, n), dtype)
    outs = [append_output(p, d, n, start.linv[d], start.alpha[d], start.logdet[d], dtype, b_dtype) for d in range(p.n_s)]
    return Appended(np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.array([o[2] for o in outs], dtype))


def chain(p, n, dtype=R.F64):
    """The rows beyond the first n appended one at a time."""
    cur = R.Reference(head(p, n), dtype)
    for m in range(n + 1, p.X.shape[0] + 1):
        cur = append(head(p, m), m - 1, dtype, start=cur)
    return cur
