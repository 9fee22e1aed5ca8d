"""The numpy oracle of the CEM solver's performance trajectory with first-order (Taylor) uncertainty propagation (test
infrastructure; used by test_perf_taylor_host.py and test_gpu_perf_taylor.py).  Built on
``oracle.gp.ExactGP.predict(z, jacobians=True)``, ``oracle.cem.objective_cost`` and
``oracle.reachability.lin_ellipsoid_safety_distance``; inputs, rows, the action-box cost of the tail and the mean recursion
are perf_var_oracle.perf_var_rollout's.

Per particle, v_t = u^s_t (t < r), u^p_t (t >= r), mu_0 = x0, Sigma_0 = 0 and the fixed feedback K = prob.k_fb.  The
joint covariance of the GP's input z = [x, u], u = v_t + K (x - mu_t), and its output g is assembled as BLOCK matrices --
the kernel multiplies them out to a short form, which is what the tests check against this:
    sigma_z   = [[Sigma, Sigma K^T], [K Sigma, K Sigma K^T]]                  (D x D)
    sigma_zg  = sigma_z J^T                                                    (D x n_s),  J the mean Jacobian at [mu_t, v_t]
    sigma_g   = diag(var_t) + J sigma_z J^T                                    (n_s x n_s)
    sigma_all = [[sigma_z, sigma_zg], [sigma_zg^T, sigma_g]]                   ((D + n_s) x (D + n_s))
    mu_{t+1}    = a mu_t + b v_t + mean_t
    Sigma_{t+1} = [a b I] sigma_all [a b I]^T
    obj        += objective_cost(prob, mu_{t+1}, diag(sigma_g))
No zero or negative fix-up.  With `terminal_safety` the ellipsoid (mu_s, Sigma_s), s = H + 2, must lie inside the safe
polytope: a row distance >= 0 adds STATE_VIOLATION_COST once."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from oracle import cem as ocem
from oracle import reachability as oreach


@dataclass
class PerfTaylorResult:
    rows: np.ndarray         # [P x (H + T) x n_u]   [safety actions | tail]
    traj: np.ndarray         # [P x n_perf x n_s]    mu_1 .. mu_n_perf
    sigma: np.ndarray        # [P x n_perf x n_s]    diag(sigma_g) of step 0 .. n_perf - 1
    var: np.ndarray          # [P x n_perf x n_s]    the GP's own variance at [mu_t, v_t]
    cov: np.ndarray          # [P x n_perf x n_s x n_s]   Sigma_1 .. Sigma_n_perf
    queries: np.ndarray      # [P x n_perf x (n_s + n_u)]   [mu_t, v_t]
    obj_cost: np.ndarray     # [P]
    con_cost: np.ndarray     # [P]   the increment: the tail's action box, plus the terminal-safety cost
    violations: np.ndarray   # [P]   violating tail steps
    distances: Optional[np.ndarray] = None    # [P x m] polytope row distances of (mu_s, Sigma_s), where n_perf >= H + 2
    unsafe: Optional[np.ndarray] = None       # [P] bool: some distance >= 0


def block_step(prob, sigma_x, var, jac):
    """One covariance step from the block matrices: sigma_x [P x n_s x n_s], var [P x n_s], jac [P x n_s x D] ->
    (sigma_g [P x n_s x n_s], Sigma' [P x n_s x n_s])."""
    P, n_s = var.shape
    k = prob.k_fb
    sk = sigma_x @ k.T                                                          # [P x n_s x n_u]
    sigma_z = np.concatenate((np.concatenate((sigma_x, sk), axis=2),
                              np.concatenate((np.swapaxes(sk, 1, 2), k @ sk), axis=2)), axis=1)
    jt = np.swapaxes(jac, 1, 2)
    sigma_zg = sigma_z @ jt
    sigma_g = jac @ sigma_z @ jt
    sigma_g[:, np.arange(n_s), np.arange(n_s)] += var
    sigma_all = np.concatenate((np.concatenate((sigma_z, sigma_zg), axis=2),
                                np.concatenate((np.swapaxes(sigma_zg, 1, 2), sigma_g), axis=2)), axis=1)
    lin = np.concatenate((prob.a, prob.b, np.eye(n_s)), axis=1)                 # [a b I]
    return sigma_g, lin @ sigma_all @ lin.T


def perf_taylor_rollout(prob, gp, x0, safe_actions, tail, r, terminal_safety=False) -> PerfTaylorResult:
    """x0 [n_s]; safe_actions [P x H x n_u]; tail [P x T x n_u] (n_perf = r + T)."""
    P, H, n_u = safe_actions.shape
    T = tail.shape[1]
    n_perf, n_s = r + T, prob.n_s
    assert 1 <= r <= H and T >= 1
    if terminal_safety and n_perf < H + 2:
        raise ValueError('terminal_safety needs n_perf >= H + 2')
    v = np.concatenate((safe_actions[:, :r], tail), axis=1)                     # [P x n_perf x n_u]
    mu = np.broadcast_to(np.asarray(x0, dtype=np.float64).reshape(1, n_s), (P, n_s)).copy()
    sigma_x = np.zeros((P, n_s, n_s))
    out = PerfTaylorResult(np.concatenate((safe_actions, tail), axis=1), np.empty((P, n_perf, n_s)),
                           np.empty((P, n_perf, n_s)), np.empty((P, n_perf, n_s)), np.empty((P, n_perf, n_s, n_s)),
                           np.empty((P, n_perf, n_s + n_u)), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int64))
    for t in range(n_perf):
        z = np.concatenate((mu, v[:, t]), axis=1)
        mean, var, jac = gp.predict(z, jacobians=True)
        sigma_g, sigma_x = block_step(prob, sigma_x, var, jac)
        mu = mu @ prob.a.T + v[:, t] @ prob.b.T + mean                          # oracle/reachability.py:96
        diag_g = np.diagonal(sigma_g, axis1=1, axis2=2)
        out.queries[:, t], out.traj[:, t], out.sigma[:, t], out.var[:, t], out.cov[:, t] = z, mu, diag_g, var, sigma_x
        out.obj_cost += ocem.objective_cost(prob, mu, diag_g)
    out.violations = ((tail < prob.u_min[None, None]) | (tail > prob.u_max[None, None])).any(axis=2).sum(axis=1)
    out.con_cost = ocem.ACTION_VIOLATION_COST * out.violations
    if n_perf >= H + 2:
        s = H + 2                                                               # mu_s, Sigma_s sit in row s - 1
        out.distances = oreach.lin_ellipsoid_safety_distance(out.traj[:, s - 1], out.cov[:, s - 1], prob.h_mat, prob.h_vec)
        out.unsafe = (out.distances >= 0).any(axis=1)
        if terminal_safety:
            out.con_cost = out.con_cost + ocem.STATE_VIOLATION_COST * out.unsafe
    return out


def cem_solve_perf_taylor(prob, gp, x0, noise, num_elites, H, n_perf, r, init_std, terminal_safety=False):
    """perf_var_oracle.cem_solve_perf_var with the rollout above: noise [iters x P x (H + T) x n_u]; zero start mean,
    `init_std` everywhere; constraints from oracle.cem.rollout over the safety actions plus the performance trajectory's
    increment, the objective from the performance trajectory alone; oracle.cem.rank / refit over the long rows.
    Returns (best row [(H + T) x n_u] | None, per iteration (con, obj, elite indices, smallest variance))."""
    iters, P, steps, n_u = noise.shape
    assert steps == H + n_perf - r
    mean, std = np.zeros((steps, n_u)), np.full((steps, n_u), float(init_std))
    best, trace = None, []
    for it in range(iters):
        rows = mean[None] + std[None] * noise[it]
        safety = ocem.rollout(prob, gp, x0, rows[:, :H])
        perf = perf_taylor_rollout(prob, gp, x0, rows[:, :H], rows[:, H:], r, terminal_safety)
        con, obj = safety.con_cost + perf.con_cost, perf.obj_cost
        idx = ocem.rank(con, obj, num_elites)
        mean, std = ocem.refit(rows[idx])
        trace.append((con, obj, idx, float(perf.sigma.min())))
        best = rows[idx[0]].copy() if con[idx[0]] == 0 else None
    return best, trace
