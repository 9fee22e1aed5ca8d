"""The numpy oracle of the CEM solver's performance trajectory WITH the GP's posterior variance (test infrastructure; used by
test_perf_var_host.py and test_gpu_perf_var.py).  Built on ``oracle.gp.ExactGP.predict(z, jacobians=False)`` and
``oracle.cem.objective_cost``, like perf_traj_oracle.py, whose mean recursion it repeats statement by statement.

Per particle, v_t = u^s_t (t < r), u^p_t (t >= r), mu_0 = x0:
    (mean_t, var_t) = GP posterior at [mu_t, v_t]          (noise included)
    mu_{t+1}        = a mu_t + b v_t + mean_t
    obj            += objective_cost(prob, mu_{t+1}, var_t)        t = 0 .. n_perf - 1
so OBJ_NEG_VARIANCE gives -sum_t sum_d var_t[d] and OBJ_AFFINE_ABS the objective of perf_traj_oracle.perf_rollout.  No zero
fix-up of var_t, no variance propagation; every tail step whose action leaves [u_min, u_max] costs ACTION_VIOLATION_COST;
there is no state constraint."""
from dataclasses import dataclass

import numpy as np

from oracle import cem as ocem


@dataclass
class PerfVarResult:
    rows: np.ndarray         # [P x (H + T) x n_u]   [safety actions | tail]
    traj: np.ndarray         # [P x n_perf x n_s]    mu_1 .. mu_n_perf
    sigma: np.ndarray        # [P x n_perf x n_s]    var_0 .. var_{n_perf - 1}
    queries: np.ndarray      # [P x n_perf x (n_s + n_u)]   [mu_t, v_t], t = 0 .. n_perf - 1
    obj_cost: np.ndarray     # [P]
    con_cost: np.ndarray     # [P]   the increment: ACTION_VIOLATION_COST x violating tail steps
    violations: np.ndarray   # [P]   violating tail steps


def perf_var_rollout(prob, gp, x0, safe_actions, tail, r) -> PerfVarResult:
    """x0 [n_s]; safe_actions [P x H x n_u]; tail [P x T x n_u] (n_perf = r + T)."""
    P, H, n_u = safe_actions.shape
    T = tail.shape[1]
    n_perf = r + T
    assert 1 <= r <= H and T >= 1
    v = np.concatenate((safe_actions[:, :r], tail), axis=1)                     # [P x n_perf x n_u]
    mu = np.broadcast_to(np.asarray(x0, dtype=np.float64).reshape(1, prob.n_s), (P, prob.n_s)).copy()
    out = PerfVarResult(np.concatenate((safe_actions, tail), axis=1), np.empty((P, n_perf, prob.n_s)),
                        np.empty((P, n_perf, prob.n_s)), np.empty((P, n_perf, prob.n_s + n_u)), np.zeros(P), np.zeros(P),
                        np.zeros(P, dtype=np.int64))
    for t in range(n_perf):
        z = np.concatenate((mu, v[:, t]), axis=1)
        mean, var, _ = gp.predict(z, jacobians=False)
        mu = mu @ prob.a.T + v[:, t] @ prob.b.T + mean                          # oracle/reachability.py:96
        out.queries[:, t], out.traj[:, t], out.sigma[:, t] = z, mu, var
        out.obj_cost += ocem.objective_cost(prob, mu, var)
    out.violations = ((tail < prob.u_min[None, None]) | (tail > prob.u_max[None, None])).any(axis=2).sum(axis=1)
    out.con_cost = ocem.ACTION_VIOLATION_COST * out.violations
    return out


def cem_solve_perf_var(prob, gp, x0, noise, num_elites, H, n_perf, r, init_std):
    """perf_traj_oracle.cem_solve_perf with the rollout above: noise [iters x P x (H + T) x n_u]; zero start mean, `init_std`
    everywhere; constraints from oracle.cem.rollout over the safety actions plus the tail's action box, the objective from
    the performance trajectory alone; oracle.cem.rank / refit over the long rows.
    Returns (best row [(H + T) x n_u] | None, per iteration (con, obj, elite indices, smallest variance))."""
    iters, P, steps, n_u = noise.shape
    assert steps == H + n_perf - r
    mean, std = np.zeros((steps, n_u)), np.full((steps, n_u), float(init_std))
    best, trace = None, []
    for it in range(iters):
        rows = mean[None] + std[None] * noise[it]
        safety = ocem.rollout(prob, gp, x0, rows[:, :H])
        perf = perf_var_rollout(prob, gp, x0, rows[:, :H], rows[:, H:], r)
        con, obj = safety.con_cost + perf.con_cost, perf.obj_cost
        idx = ocem.rank(con, obj, num_elites)
        mean, std = ocem.refit(rows[idx])
        trace.append((con, obj, idx, float(perf.sigma.min())))
        best = rows[idx[0]].copy() if con[idx[0]] == 0 else None
    return best, trace
