"""The numpy oracle of the SafeMPC constraint set on the safety trajectory of a CEM solve (test infrastructure; used by
test_conset_host.py and test_gpu_conset.py): what the set adds to the constraint cost of a row, from an
`oracle.cem.RolloutResult` (or any trajectory of ellipsoids) plus (x0, actions), through
`oracle.reachability.lin_ellipsoid_safety_distance` -- the function the goldens pin to the reference's, which is all the
reference's constraints are: that function on (k_ff, K Q K^T, [I; -I], [u_max; -u_min]) for the feedback bounds
(safempc_simple.py:492-536) and on (p, Q, h_mat_obs, h_obs) for the obstacle rows (:325-396) -- and a `cem_solve` that adds
it before `oracle.cem.rank`.  The inputs of the main case and of the solve are defined here, computed once and left unchanged.

The rule (include/sx_amd.h, sx_con_set).  Step t = 0 .. H-1 starts from (p_t, Q_t) (Q_0 = q0, or a point) with the action
u_t and reaches (p_{t+1}, Q_{t+1}).  It is ellipsoid-violated where it starts from an ellipsoid and some distance of
(u_t, K Q_t K^T) to the box is >= 0; the action cost 3 is paid ONCE per step that is box-violated or ellipsoid-violated, so
the set adds 3 where the step is ellipsoid-violated with the box satisfied.  Every step with t + 1 < H whose
(p_{t+1}, Q_{t+1}) has some distance to the obstacle rows >= 0 adds 10.  A NaN distance is not a violation."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from oracle import cem as ocem
from oracle import reachability as reach
from oracle.gp import ExactGP
from safe_exploration_amd import problems

GAP = 1e-6          # every elite set of the solve is decided by more than this
MARGIN = 1e-6       # no distance of the inputs sits closer to the boundary than this: the comparisons are exact
P, K, ITERS, SEED = 256, 20, 4, 11
H = 5
PENDULUM_X0 = np.array([0.02, -0.03])
INIT_STD = 0.5
OBSTACLE_SCALE = 0.9    # the first two safe-polytope rows (|d_theta| <= 0.8, one side each) pulled in to 0.72


@dataclass
class ConSet:
    h_mat_obs: np.ndarray          # [m_obs x n_s]
    h_obs: np.ndarray              # [m_obs]
    ctrl_ellipsoid: bool = True

    def struct(self, n_s):
        """The sx_con_set of this set."""
        from safe_exploration_amd.gp_reachability_pytorch import make_con_set
        rows = self.h_mat_obs if len(self.h_obs) else None
        return make_con_set(n_s, h_mat_obs=rows, h_obs=self.h_obs if len(self.h_obs) else None,
                            ctrl_ellipsoid=self.ctrl_ellipsoid)


def empty(n_s):
    return ConSet(np.zeros((0, n_s)), np.zeros(0), False)


@dataclass
class Signals:
    box: np.ndarray        # [P x H] bool: the step's action is outside the box (the parent's strict test)
    ell: np.ndarray        # [P x H] bool: the step is ellipsoid-violated
    obs: np.ndarray        # [P x H] bool: the step's reached ellipsoid violates the obstacle rows (never at t = H - 1)
    min_abs_d: float       # the smallest |d| over all control and obstacle rows of all particles and steps

    @property
    def extra(self):
        """[P]: what the set adds to con_cost."""
        return (ocem.ACTION_VIOLATION_COST * (self.ell & ~self.box).sum(axis=1)
                + ocem.STATE_VIOLATION_COST * self.obs.sum(axis=1))


def ctrl_distances(prob, u, q_start):
    """[P x 2 n_u]: the distances of the control ellipsoids (u, K q_start K^T) to the action box."""
    n_u = u.shape[1]
    k_fb = np.asarray(prob.k_fb, dtype=np.float64).reshape(n_u, prob.n_s)
    h_u, hv_u = np.vstack((np.eye(n_u), -np.eye(n_u))), np.concatenate((prob.u_max, -prob.u_min))
    with np.errstate(invalid='ignore'):
        return reach.lin_ellipsoid_safety_distance(u, np.einsum('ci,pij,dj->pcd', k_fb, q_start, k_fb), h_u, hv_u)


def obstacle_distances(con: ConSet, p, q):
    """[P x m_obs]: the distances of the ellipsoids (p, q) to the obstacle rows."""
    with np.errstate(invalid='ignore'):
        return reach.lin_ellipsoid_safety_distance(p, q, con.h_mat_obs, con.h_obs)


def box_violated(prob, u):
    return ((u < prob.u_min[None]) | (u > prob.u_max[None])).any(axis=1)


def _smallest(d, so_far):
    return min(so_far, float(np.nanmin(np.abs(d)))) if np.isfinite(d).any() else so_far


def signals(prob, con: ConSet, traj_p, traj_q, actions, q0=None) -> Signals:
    """The set's signals of the rows `actions` [P x H x n_u] along the ellipsoids (traj_p [P x H x n_s], traj_q
    [P x H x n_s x n_s]: (p_{t+1}, Q_{t+1}) at index t) they reach from a point (q0 None) or from (., q0)."""
    Pn, Hn, _ = actions.shape
    n_s = prob.n_s
    box, ell, obs = (np.zeros((Pn, Hn), dtype=bool) for _ in range(3))
    smallest = np.inf
    for t in range(Hn):
        u = actions[:, t]
        box[:, t] = box_violated(prob, u)
        q_start = (None if q0 is None else np.broadcast_to(q0, (Pn, n_s, n_s))) if t == 0 else traj_q[:, t - 1]
        if con.ctrl_ellipsoid and q_start is not None:
            d = ctrl_distances(prob, u, q_start)
            ell[:, t] = (d >= 0).any(axis=1)
            smallest = _smallest(d, smallest)
        if t + 1 < Hn and len(con.h_obs):
            d = obstacle_distances(con, traj_p[:, t], traj_q[:, t])
            obs[:, t] = (d >= 0).any(axis=1)
            smallest = _smallest(d, smallest)
    return Signals(box, ell, obs, smallest)


def extra_cost(prob, con: ConSet, result, actions, q0=None):
    """[P]: what the set adds to the con_cost of an `oracle.cem.RolloutResult` of `actions`."""
    return signals(prob, con, result.traj_p, result.traj_q, actions, q0).extra


def step_cost(prob, con: ConSet, u, q_start, p_next, q_next, check_obstacle):
    """[P]: sx_conset_eval -- the action cost of a step (box or ellipsoid) plus the obstacle cost of what it reaches."""
    viol = box_violated(prob, u)
    if con.ctrl_ellipsoid and q_start is not None:
        viol = viol | (ctrl_distances(prob, u, q_start) >= 0).any(axis=1)
    cost = ocem.ACTION_VIOLATION_COST * viol
    if check_obstacle and len(con.h_obs):
        cost = cost + ocem.STATE_VIOLATION_COST * (obstacle_distances(con, p_next, q_next) >= 0).any(axis=1)
    return cost


def cem_solve(prob, con: Optional[ConSet], gp, x0, noise, num_elites, init_std):
    """oracle.cem.cem_solve with the set's cost added to the constraint cost before the ranking (con None: without).
    Returns (best row | None, per iteration (con, obj, elite indices, smallest |d|))."""
    iters, _, Hn, n_u = noise.shape
    mean, std = np.zeros((Hn, n_u)), np.full((Hn, n_u), float(init_std))
    best, trace = None, []
    for it in range(iters):
        rows = mean[None] + std[None] * noise[it]
        r = ocem.rollout(prob, gp, x0, rows)
        s = None if con is None else signals(prob, con, r.traj_p, r.traj_q, rows)
        cost = r.con_cost if s is None else r.con_cost + s.extra
        idx = ocem.rank(cost, r.obj_cost, num_elites)
        mean, std = ocem.refit(rows[idx])
        trace.append((cost, r.obj_cost, idx, np.inf if s is None else s.min_abs_d))
        best = rows[idx[0]].copy() if cost[idx[0]] == 0 else None
    return best, trace


def elite_gaps(trace, k):
    """Per iteration: the gap that decides the elite set -- between the k-th and the (k+1)-th ranked row, in the objective
    where their constraint costs are equal (inf where they differ: whole penalties apart)."""
    gaps = []
    for cost, obj, _idx, _ in trace:
        order = ocem.rank(cost, obj, k + 1)
        a, b = order[k - 1], order[k]
        gaps.append(abs(obj[a] - obj[b]) if cost[a] == cost[b] else np.inf)
    return gaps


def gp_of(spec):
    return ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)


def pendulum_spec():
    """The main case's problem: the pendulum with |theta_target - theta| as its objective (a target the rows tell apart)."""
    from safe_exploration_amd import _lib
    return problems.pendulum(n_train=200, seed=0, obj_mode=_lib.SX_OBJ_AFFINE_ABS)


def pendulum_set(spec):
    """The feedback bounds and, as the obstacle, the first two safe-polytope rows pulled in by OBSTACLE_SCALE."""
    return ConSet(spec.h_mat[:2].copy(), OBSTACLE_SCALE * spec.h_vec[:2, 0], True)


_DONE = {}


def main_case():
    """(spec, set, x0, rows [P x H x n_u], the oracle's rollout of them, its signals): 256 rows drawn with std 0.5."""
    if 'main' not in _DONE:
        spec = pendulum_spec()
        con = pendulum_set(spec)
        rows = INIT_STD * np.random.default_rng(SEED).normal(size=(P, H, spec.n_u))
        prob = problems.oracle_problem(spec, ocem)
        r = ocem.rollout(prob, gp_of(spec), PENDULUM_X0, rows)
        _DONE['main'] = (spec, con, PENDULUM_X0, rows, r, signals(prob, con, r.traj_p, r.traj_q, rows))
    return _DONE['main']


def solve():
    """(spec, set, H, x0, init_std, noise [iters x P x H x n_u], best row with the set, its trace, best row and trace of
    the same solve without the set)."""
    if 'solve' not in _DONE:
        spec = pendulum_spec()
        con = pendulum_set(spec)
        noise = np.random.default_rng(SEED).normal(size=(ITERS, P, H, spec.n_u))
        prob, gp = problems.oracle_problem(spec, ocem), gp_of(spec)
        best, trace = cem_solve(prob, con, gp, PENDULUM_X0, noise, K, INIT_STD)
        plain_best, plain_trace = cem_solve(prob, None, gp, PENDULUM_X0, noise, K, INIT_STD)
        _DONE['solve'] = (spec, con, H, PENDULUM_X0, INIT_STD, noise, best, trace, plain_best, plain_trace)
    return _DONE['solve']
