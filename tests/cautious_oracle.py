"""The numpy oracle of the chance-constrained Taylor rollout of Cautious MPC (test infrastructure; used by
test_cautious_host.py and test_gpu_cautious.py).  Built on ``oracle.gp.ExactGP.predict(z, jacobians=True)``,
``perf_taylor_oracle.block_step`` (the block-matrix form of the covariance step: the kernel multiplies it out),
``oracle.reachability.lin_ellipsoid_safety_distance(..., c_safety=beta)`` and ``oracle.cem.objective_cost``.

Per particle a row k_ff_0 .. k_ff_{T-1}, mu_0 = x0, Sigma_0 = 0, K = prob.k_fb, beta = prob.beta; for t = 0 .. T - 1:
    control  t = 0: k_ff_0 outside [u_min, u_max];  t >= 1: the ellipsoid (k_ff_t, K Sigma_t K^T) against the box rows
             [I; -I] u <= [u_max; -u_min] (cautious_mpc.py:397-442); some distance >= 0 costs ACTION_VIOLATION_COST once
    (mean_t, var_t, J_t) at [mu_t, k_ff_t];  (sigma_g, Sigma_{t+1}) = block_step(Sigma_t)  (propagate False: block_step(0))
    mu_{t+1} = a mu_t + b k_ff_t + mean_t
    state    some row distance of (mu_{t+1}, Sigma_{t+1}) against (h_mat, h_vec) >= 0 costs STATE_VIOLATION_COST once
    obj     += objective_cost(prob, mu_{t+1}, diag sigma_g)
(cautious_mpc.py:337-395).  A NaN distance counts as inside."""
from dataclasses import dataclass

import numpy as np

from oracle import cem as ocem
from oracle import reachability as oreach
from perf_taylor_oracle import block_step


@dataclass
class CautiousResult:
    rows: np.ndarray           # [P x T x n_u]
    traj: np.ndarray           # [P x T x n_s]        mu_1 .. mu_T
    sigma: np.ndarray          # [P x T x n_s]        diag(sigma_g)
    var: np.ndarray            # [P x T x n_s]        the GP's own variance
    cov: np.ndarray            # [P x T x n_s x n_s]  Sigma_1 .. Sigma_T
    state_d: np.ndarray        # [P x T x m]          row distances of (mu_{t+1}, Sigma_{t+1})
    ctrl_d: np.ndarray         # [P x T x 2 n_u]      [k + s - u_max | u_min - k + s]; t = 0: s = 0
    spread: np.ndarray         # [P x T x n_u]        beta sqrt(K_c Sigma_t K_c^T); 0 at t = 0
    state_viol: np.ndarray     # [P x T] bool
    ctrl_viol: np.ndarray      # [P x T] bool
    obj_cost: np.ndarray       # [P]
    con_cost: np.ndarray       # [P]

    @property
    def margins(self):
        """[P x T x 2]: the largest state row distance (-inf without rows) and the largest control distance."""
        P, T = self.state_viol.shape
        state = self.state_d.max(axis=2) if self.state_d.shape[2] else np.full((P, T), -np.inf)
        return np.stack((state, self.ctrl_d.max(axis=2)), axis=2)


def box_rows(prob):
    """The action box as polytope rows [I; -I] u <= [u_max; -u_min] (cautious_mpc.py:433-434)."""
    n_u = prob.n_u
    return (np.vstack((np.eye(n_u), -np.eye(n_u))),
            np.concatenate((np.asarray(prob.u_max, dtype=np.float64), -np.asarray(prob.u_min, dtype=np.float64))).reshape(-1, 1))


def cautious_rollout(prob, gp, x0, rows, propagate=True) -> CautiousResult:
    """x0 [n_s]; rows [P x T x n_u]."""
    P, T, n_u = rows.shape
    n_s, m = prob.n_s, prob.h_mat.shape[0]
    mu = np.broadcast_to(np.asarray(x0, dtype=np.float64).reshape(1, n_s), (P, n_s)).copy()
    sigma_x = np.zeros((P, n_s, n_s))
    hu, bu = box_rows(prob)
    out = CautiousResult(rows.copy(), np.empty((P, T, n_s)), np.empty((P, T, n_s)), np.empty((P, T, n_s)),
                         np.empty((P, T, n_s, n_s)), np.empty((P, T, m)), np.empty((P, T, 2 * n_u)), np.zeros((P, T, n_u)),
                         np.zeros((P, T), dtype=bool), np.zeros((P, T), dtype=bool), np.zeros(P), np.zeros(P))
    for t in range(T):
        k = rows[:, t]
        if t == 0:
            out.ctrl_d[:, t] = np.concatenate((k - prob.u_max[None], prob.u_min[None] - k), axis=1)
            out.ctrl_viol[:, t] = ((k < prob.u_min[None]) | (k > prob.u_max[None])).any(axis=1)
        else:
            q_u = prob.k_fb @ sigma_x @ prob.k_fb.T                                 # [P x n_u x n_u]
            out.ctrl_d[:, t] = oreach.lin_ellipsoid_safety_distance(k, q_u, hu, bu, c_safety=prob.beta)
            out.spread[:, t] = prob.beta * np.sqrt(np.diagonal(q_u, axis1=1, axis2=2))
            out.ctrl_viol[:, t] = (out.ctrl_d[:, t] >= 0).any(axis=1)
        z = np.concatenate((mu, k), axis=1)
        mean, var, jac = gp.predict(z, jacobians=True)
        sigma_g, sigma_x = block_step(prob, sigma_x if propagate else np.zeros_like(sigma_x), var, jac)
        mu = mu @ prob.a.T + k @ prob.b.T + mean
        diag_g = np.diagonal(sigma_g, axis1=1, axis2=2)
        out.traj[:, t], out.sigma[:, t], out.var[:, t], out.cov[:, t] = mu, diag_g, var, sigma_x
        out.state_d[:, t] = oreach.lin_ellipsoid_safety_distance(mu, sigma_x, prob.h_mat, prob.h_vec, c_safety=prob.beta)
        out.state_viol[:, t] = (out.state_d[:, t] >= 0).any(axis=1)
        out.obj_cost += ocem.objective_cost(prob, mu, diag_g)
    out.con_cost = (ocem.ACTION_VIOLATION_COST * out.ctrl_viol.sum(axis=1)
                    + ocem.STATE_VIOLATION_COST * out.state_viol.sum(axis=1))
    return out


def distances_at(prob, x0, rows, traj, cov):
    """The margins [P x T x 2] from GIVEN means and covariances (a kernel's own outputs): the same formulas on the same
    inputs, so that only rounding differs."""
    P, T, n_u = rows.shape
    hu, bu = box_rows(prob)
    out = np.full((P, T, 2), -np.inf)
    for t in range(T):
        if prob.h_mat.shape[0]:
            out[:, t, 0] = oreach.lin_ellipsoid_safety_distance(traj[:, t], cov[:, t], prob.h_mat, prob.h_vec,
                                                                c_safety=prob.beta).max(axis=1)
        q_u = np.zeros((P, n_u, n_u)) if t == 0 else prob.k_fb @ cov[:, t - 1] @ prob.k_fb.T
        out[:, t, 1] = oreach.lin_ellipsoid_safety_distance(rows[:, t], q_u, hu, bu, c_safety=prob.beta).max(axis=1)
    return out


def cem_solve_cautious(prob, gp, x0, noise, num_elites, init_std, propagate=True, init_mean=None):
    """A numpy CEM over the rollout above, like perf_taylor_oracle.cem_solve_perf_taylor: noise [iters x P x T x n_u]; zero
    start mean (or `init_mean`), `init_std` everywhere; oracle.cem.rank / refit over the rows.
    Returns (best row [T x n_u] | None, per iteration (con, obj, elite indices, smallest variance))."""
    iters, P, T, n_u = noise.shape
    mean = np.zeros((T, n_u)) if init_mean is None else np.asarray(init_mean, dtype=np.float64).reshape(T, n_u)
    std = np.full((T, n_u), float(init_std))
    best, trace = None, []
    for it in range(iters):
        rows = mean[None] + std[None] * noise[it]
        r = cautious_rollout(prob, gp, x0, rows, propagate)
        idx = ocem.rank(r.con_cost, r.obj_cost, num_elites)
        mean, std = ocem.refit(rows[idx])
        trace.append((r.con_cost, r.obj_cost, idx, float(r.sigma.min())))
        best = rows[idx[0]].copy() if r.con_cost[idx[0]] == 0 else None
    return best, trace
