"""The numpy oracle of the PILCO saturating cost as a trajectory objective (test infrastructure; used by
test_sat_cost_host.py and test_gpu_sat_cost.py).  The augmentation and the loss are the reference's formulas
(utils_casadi.py trig_prop / trig_aug with a = 1, keep_radian = False, and loss_sat in its inverse / determinant form:
the non-symmetric I + S~ W is inverted as the reference does), written out for one Gaussian; `v_form` is the symmetric
form the kernels use, for comparison.  The trajectory sum prices the (mu_{t+1}, Sigma_{t+1}) of the existing oracles'
rollouts (generic_cost: stage and terminal cost are the same function), and the two CEM solves are theirs with that
objective."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from oracle import cem as ocem
from cautious_oracle import cautious_rollout
from perf_taylor_oracle import perf_taylor_rollout

# the reference's cart-pole constants (defaultconfig_episode.py:115-120): the angle is state 2, the target is the cart at
# x = 2.5 with the pole up (cos = l = 0.5 in the augmented state's last entry)
CARTPOLE_TRIG_IDX = 2
CARTPOLE_TARGET = np.array([2.5, 0.0, 0.0, 0.0, 0.5])
CARTPOLE_WEIGHT = np.diag([20.0, 0.0, 0.0, 0.0, 5.0]) / 100.0


@dataclass
class Cost:
    target: np.ndarray            # [n_a]
    weight: np.ndarray            # [n_a x n_a]
    trig_idx: Optional[int] = None


def augment(mu, cov, trig_idx):
    """(m~ [n_a], S~ [n_a x n_a]) of one Gaussian (mu [n_s], cov [n_s x n_s])."""
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    if trig_idx is None:
        return mu.copy(), cov.copy()
    i, n_s = trig_idx, mu.size
    keep = [j for j in range(n_s) if j != i]
    m, v = mu[i], cov[i, i]
    e0, e1 = np.exp(-v / 2.0), np.exp(-2.0 * v)
    s, c = e0 * np.sin(m), e0 * np.cos(m)
    vss = (1.0 - e1 * np.cos(2.0 * m)) / 2.0 - s * s
    vcc = (1.0 + e1 * np.cos(2.0 * m)) / 2.0 - c * c
    vsc = e1 * np.sin(2.0 * m) / 2.0 - s * c
    k = n_s - 1
    ma = np.concatenate((mu[keep], [s, c]))
    sa = np.zeros((k + 2, k + 2))
    sa[:k, :k] = cov[np.ix_(keep, keep)]
    sa[:k, k] = sa[k, :k] = cov[keep, i] * c
    sa[:k, k + 1] = sa[k + 1, :k] = -cov[keep, i] * s
    sa[k, k], sa[k + 1, k + 1] = vss, vcc
    sa[k, k + 1] = sa[k + 1, k] = vsc
    return ma, sa


def loss(cost: Cost, mu, cov):
    """1 - exp(-1/2 d^T W (I + S~ W)^-1 d) / sqrt(det(I + S~ W)) of one Gaussian."""
    ma, sa = augment(mu, cov, cost.trig_idx)
    d = ma - cost.target
    isw = np.eye(ma.size) + sa @ cost.weight
    q = d @ cost.weight @ np.linalg.solve(isw, d)
    return 1.0 - np.exp(-0.5 * q) / np.sqrt(np.linalg.det(isw))


def factor(weight, tol=1e-12):
    """V [n_a x k] with W = V V^T from the symmetric eigendecomposition, eigenvalues below tol * the largest dropped."""
    lam, vec = np.linalg.eigh(weight)
    keep = lam >= tol * lam[-1]
    return vec[:, keep] * np.sqrt(lam[keep])


def v_form(cost: Cost, mu, cov, v=None):
    """The loss in the symmetric form: y = V^T d, S = I + V^T S~ V, L = chol S, 1 - exp(-|L^-1 y|^2 / 2) / prod diag L."""
    v = factor(cost.weight) if v is None else v
    ma, sa = augment(mu, cov, cost.trig_idx)
    y = v.T @ (ma - cost.target)
    chol = np.linalg.cholesky(np.eye(v.shape[1]) + v.T @ sa @ v)
    z = np.linalg.solve(chol, y)
    return 1.0 - np.exp(-0.5 * (z @ z)) / np.prod(np.diag(chol))


def losses(cost: Cost, mu, cov):
    """`loss` over leading axes: mu [... x n_s], cov [... x n_s x n_s] -> [...]."""
    mu, cov = np.asarray(mu), np.asarray(cov)
    out = np.empty(mu.shape[:-1])
    for idx in np.ndindex(*out.shape):
        out[idx] = loss(cost, mu[idx], cov[idx])
    return out


def trajectory_cost(cost: Cost, result):
    """sum_t loss(mu_{t+1}, Sigma_{t+1}) over a CautiousResult / PerfTaylorResult (or anything with traj [P x T x n_s] and
    cov [P x T x n_s x n_s]) -> [P]."""
    return losses(cost, result.traj, result.cov).sum(axis=1)


def cem_solve_cautious(cost: Cost, prob, gp, x0, noise, num_elites, init_std, propagate=True):
    """cautious_oracle.cem_solve_cautious with the saturating cost as the objective.
    Returns (best row | None, per iteration (con, obj, elite indices))."""
    iters, P, T, n_u = noise.shape
    mean, std = np.zeros((T, n_u)), np.full((T, n_u), float(init_std))
    best, trace = None, []
    for it in range(iters):
        rows = mean[None] + std[None] * noise[it]
        r = cautious_rollout(prob, gp, x0, rows, propagate)
        obj = trajectory_cost(cost, r)
        idx = ocem.rank(r.con_cost, obj, num_elites)
        mean, std = ocem.refit(rows[idx])
        trace.append((r.con_cost, obj, idx))
        best = rows[idx[0]].copy() if r.con_cost[idx[0]] == 0 else None
    return best, trace


def cem_solve_perf_taylor(cost: Cost, prob, gp, x0, noise, num_elites, H, n_perf, r, init_std, terminal_safety=False):
    """perf_taylor_oracle.cem_solve_perf_taylor with the saturating cost as the objective of the performance trajectory.
    Returns (best row | None, per iteration (con, obj, elite indices))."""
    iters, P, steps, n_u = noise.shape
    assert steps == H + n_perf - r
    mean, std = np.zeros((steps, n_u)), np.full((steps, n_u), float(init_std))
    best, trace = None, []
    for it in range(iters):
        rows = mean[None] + std[None] * noise[it]
        safety = ocem.rollout(prob, gp, x0, rows[:, :H])
        perf = perf_taylor_rollout(prob, gp, x0, rows[:, :H], rows[:, H:], r, terminal_safety)
        con, obj = safety.con_cost + perf.con_cost, trajectory_cost(cost, perf)
        idx = ocem.rank(con, obj, num_elites)
        mean, std = ocem.refit(rows[idx])
        trace.append((con, obj, idx))
        best = rows[idx[0]].copy() if con[idx[0]] == 0 else None
    return best, trace


def elite_gaps(trace, num_elites):
    """Per iteration: the gap, in the ranking's order (con, then obj), between the last elite and the first non-elite:
    (con gap, obj gap where the constraint costs tie, else inf)."""
    gaps = []
    for con, obj, idx in trace:
        order = ocem.rank(con, obj, len(con))
        last, first = order[num_elites - 1], order[num_elites]
        gaps.append(abs(obj[first] - obj[last]) if con[first] == con[last] else np.inf)
    return gaps
