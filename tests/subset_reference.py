"""Reference for the max-variance subset selection (sx_gp_select; tests/test_subset_select_host.py,
tests/test_gpu_subset_select.py): plain numpy, no GPU, none of the project's kernels.

`oracle` works from the definition: at every step the predictive variance (noise included) of every pool point given
the points chosen so far, by a FRESH Cholesky solve on the chosen set, summed over the outputs; the pivot is the
unchosen point where that is largest, the lowest index among equals.  `incremental` is the algorithm the kernel runs
(a jointly pivoted Cholesky factorisation, residuals updated column by column) in numpy.  Both form only the kernel
columns of the chosen points, never the n x n matrix."""
import functools

import numpy as np
import scipy.linalg as sla

import warm_path_reference as R

F64, LD = R.F64, R.LD

# (n_s, n_u, n, m, ratio).  A workgroup of the kernel owns 64 pool rows: 50 is one workgroup, 97 two, 193 / 257 / 1025
# end in a one-row workgroup, 4100 has 65 partials (more than the 64 one pass of a wave reduces) and a ragged last
# workgroup; m = n at 97 leaves the last steps one candidate.
CASES = ((1, 1, 97, 97, 1e-2), (2, 1, 193, 64, 1e-2), (4, 2, 193, 64, 1e-2), (3, 1, 257, 100, 1e-2),
         (2, 1, 300, 128, 1e-4), (4, 1, 330, 65, 1e-4), (2, 1, 410, 130, 1e-6), (2, 1, 1025, 33, 1e-2),
         (2, 1, 4100, 12, 1e-2), (2, 1, 50, 20, 1e-2))
SEEDS, SEEDS_M = (192, 7, 100, 55, 3), 40          # on (2, 1, 193)
TIE_ROWS, TIE_M = (20, 150), 30                    # on (2, 1, 193): both rows become the far point (3, 3, 3)
BATCH_N, BATCH_M = (97, 257, 193), 40              # three (2, 1) problems in one call
PYTHON_CASE = (2, 1, 300, 64, 1e-2)                # GpCemSSM with cem_gp_subset_size = 64
GAP_FLOOR = 1e-9                                   # x sum_d (s_d + noise_d): what every greedy step's gap must exceed
SEL_VAR_TOL = 1e-10                                # x sum_d (s_d + noise_d): a tenth of that


def prior(p):
    """sum_d (s_d + noise_d): the summed variance of any point before anything is chosen"""
    return float(np.sum(p.s + p.noise))


def tie_problem():
    """(2, 1, 193) with rows 20 and 150 at the same far point: they tie exactly at step 1, and 150 is never chosen"""
    p = R.problem(2, 1, 193, 1e-2)
    X = p.X.copy()
    X[list(TIE_ROWS)] = 3.0
    X.setflags(write=False)
    return p._replace(key=('subset_tie',) + p.key, X=X)


def copies_problem(n=40):
    """n copies of one point with noise = -0.01 s: step 0 succeeds (r = 0.99 s), and every residual is then
    0.99 s - s^2 / (0.99 s) < 0, so step 1 meets a variance that is not positive"""
    p = R.problem(2, 1, n, 1e-2)
    X = np.tile(p.X[:1], (n, 1))
    noise = -0.01 * p.s
    for a in (X, noise):
        a.setflags(write=False)
    return p._replace(key=('subset_copies',) + p.key, X=X, noise=noise)


def _columns(p, d, rows, dtype):
    """[len(rows) x n]  rows `rows` of K_d + noise_d I"""
    K = R.kstar(p, d, p.X[rows], dtype)
    K[np.arange(len(rows)), rows] += dtype(p.noise[d])
    return K


def _forward(L, B):
    """L^-1 B by forward substitution in L's own precision"""
    out = np.empty_like(B)
    for r in range(L.shape[0]):
        out[r] = (B[r] - L[r, :r] @ out[:r]) / L[r, r]
    return out


def variances(p, chosen, dtype=F64):
    """[n]  sum_d var_d(x_i | chosen), noise included, by a fresh Cholesky solve on the chosen set"""
    n = p.X.shape[0]
    tot = np.zeros(n, dtype)
    rows = np.asarray(chosen, dtype=np.int64)
    for d in range(p.n_s):
        tot += dtype(p.s[d]) + dtype(p.noise[d])
        if len(rows):
            Kc = _columns(p, d, rows, dtype)
            Kcc = Kc[:, rows]
            if dtype is F64:
                B = sla.solve_triangular(np.linalg.cholesky(Kcc), Kc, lower=True)
            else:
                B = _forward(R.cholesky_ld(Kcc), Kc)
            tot -= (B * B).sum(0)
    return tot


def _oracle(p, m, seeds, dtype):
    n = p.X.shape[0]
    chosen, sel, gaps = [], [], []
    for j in range(m):
        tot = variances(p, chosen, dtype)
        cand = tot.copy()
        cand[chosen] = -np.inf
        if j < len(seeds):
            pivot = int(seeds[j])
            gaps.append(np.inf)
        else:
            pivot = int(np.argmax(cand))                       # the first of equals: the lowest index
            order = np.sort(cand)[::-1]
            gaps.append(float(order[0] - order[1]) if n - j > 1 else np.inf)
        chosen.append(pivot)
        sel.append(tot[pivot])
    out = (np.array(chosen), np.array(sel, dtype), np.array(gaps))
    for a in out:
        a.setflags(write=False)
    return out


_oracles = {}


def oracle(p, m, seeds=(), dtype=F64):
    """(idx [m], sel_var [m] in `dtype`, gap [m]): gap[j] is the absolute difference between the best and the
    second-best candidate of greedy step j (inf at a seeded step and where one candidate is left).  Cached: computed
    once per (problem, m, seeds, precision), shared by the tests, never modified."""
    key = (p.key, m, tuple(seeds), dtype is LD)
    if key not in _oracles:
        _oracles[key] = _oracle(p, m, tuple(seeds), dtype)
    return _oracles[key]


def incremental(p, m, seeds=()):
    """(idx [m], sel_var [m]): the pivoted factorisation the kernel runs, in float64"""
    n = p.X.shape[0]
    r = np.stack([np.full(n, p.s[d] + p.noise[d]) for d in range(p.n_s)])
    C = np.zeros((p.n_s, m, n))
    chosen, sel, mask = [], [], np.zeros(n, bool)
    for j in range(m):
        tot = r.sum(0)
        pivot = int(seeds[j]) if j < len(seeds) else int(np.argmax(np.where(mask, -np.inf, tot)))
        sel.append(tot[pivot])
        chosen.append(pivot)
        mask[pivot] = True
        for d in range(p.n_s):
            k = _columns(p, d, np.array([pivot]), F64)[0]
            c = (k - C[d, :j, pivot] @ C[d, :j, :]) / np.sqrt(r[d, pivot])
            C[d, j] = c
            r[d] -= c * c
    return np.array(chosen), np.array(sel)


SOLVER_N, SOLVER_M = 300, 64                       # the pendulum pool a CemSafeMPC acts on


@functools.lru_cache(maxsize=None)
def solver_problem():
    """(spec, problem): the pendulum workload with SOLVER_N points and per-output hyper-parameters, and its inputs and
    hyper-parameters as a Problem"""
    from safe_exploration_amd import problems
    spec = problems.pendulum(n_train=SOLVER_N, ard=True)
    return spec, R._frozen(R.Problem(('subset_solver', SOLVER_N), spec.n_s, spec.n_u, spec.X.copy(), spec.Y.copy(),
                                     spec.lengthscale.copy(), spec.outputscale.copy(), spec.noise.copy()))


@functools.lru_cache(maxsize=None)
def gpu_problems():
    """Every (name, problem, m, seeds) the GPU tests select from"""
    out = [(f'case{c}', R.problem(*c[:3], c[4]), c[3], ()) for c in CASES]
    out.append(('tie', tie_problem(), TIE_M, ()))
    out.append(('seeds', R.problem(2, 1, 193, 1e-2), SEEDS_M, SEEDS))
    out += [(f'batch{n}', R.problem(2, 1, n, 1e-2), BATCH_M, ()) for n in BATCH_N]
    c = PYTHON_CASE
    out.append(('python', R.problem(*c[:3], c[4]), c[3], ()))
    out.append(('solver', solver_problem()[1], SOLVER_M, ()))
    return tuple(out)
