"""The numpy oracle of static exploration in the CEM solver (test infrastructure; used by test_static_explore_host.py and
test_gpu_static_explore.py).  Built on ``oracle.cem.rollout / rank / refit`` and
``oracle.reachability.is_ellipsoid_inside_polytope``.

The CEM row of a particle is [x0 (n_s) | u_0 .. u_{H-1} (H n_u)], L = n_s + H n_u entries with one Gaussian each.  A
particle is rolled out from the point x0 of its own row (``oracle.cem.rollout`` with x0 [P x n_s]: reach_point at t = 0)
under the problem's own constraint mode, action box and polytope, with the variance objective whatever the problem's
obj_mode says; a start outside the safe polytope (h_mat x0 - h_vec >= 0 in any row: the ellipsoid test with Q = 0) adds
STATE_VIOLATION_COST once, in either constraint mode.  The solve starts from mean [start_mean | 0] and std [start_std |
init_std], ranks by (con, obj, index) and refits over the long rows; its answer per problem is the first-ranked row of the
last iteration with its (con, obj).  Restarts are problems with the same start distribution and their own noise; the
answer is the feasible one of lowest objective, the lowest index on a tie, None where none is feasible."""
import dataclasses

import numpy as np

from oracle import cem as ocem
from oracle import reachability as oreach


def start_outside(prob, x0):
    """[P] bool: the start x0 [P x n_s] is not inside the safe polytope."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, prob.n_s)
    return ~oreach.is_ellipsoid_inside_polytope(x0, np.zeros((len(x0), prob.n_s, prob.n_s)), prob.h_mat, prob.h_vec)


def split(prob, rows):
    """rows [P x L] -> (x0 [P x n_s], actions [P x H x n_u])."""
    P, L = rows.shape
    return rows[:, :prob.n_s], rows[:, prob.n_s:].reshape(P, (L - prob.n_s) // prob.n_u, prob.n_u)


def rollout(prob, gp, rows, variance_objective=True):
    """oracle.cem.rollout from every row's own start, plus the start constraint.  `variance_objective=False` keeps the
    problem's obj_mode (the C entry honours env->obj_mode; the solver always passes the variance objective).  The result
    gains `start_cost` [P], the part of con_cost that the starts added."""
    if variance_objective:
        prob = dataclasses.replace(prob, obj_mode=ocem.OBJ_NEG_VARIANCE)
    x0, actions = split(prob, rows)
    res = ocem.rollout(prob, gp, x0, actions)
    res.start_cost = ocem.STATE_VIOLATION_COST * start_outside(prob, x0)
    res.con_cost = res.con_cost + res.start_cost
    return res


def cem_solve(prob, gp, noise, num_elites, start_mean, start_std, init_std=1.0):
    """One problem.  noise [iters x P x L].  Returns (best row [L], (con, obj) of it, best_ok, per iteration
    (con [P], obj [P], elite indices))."""
    iters, P, L = noise.shape
    n_s = prob.n_s
    mean = np.concatenate((np.broadcast_to(np.asarray(start_mean, dtype=np.float64).reshape(-1), (n_s,)), np.zeros(L - n_s)))
    std = np.concatenate((np.broadcast_to(np.asarray(start_std, dtype=np.float64).reshape(-1), (n_s,)),
                          np.broadcast_to(np.asarray(init_std, dtype=np.float64).reshape(-1, 1) * np.ones((1, prob.n_u)),
                                          ((L - n_s) // prob.n_u, prob.n_u)).reshape(-1)))
    best, costs, trace = None, None, []
    for it in range(iters):
        rows = mean[None] + std[None] * noise[it]
        res = rollout(prob, gp, rows)
        idx = ocem.rank(res.con_cost, res.obj_cost, num_elites)
        mean, std = ocem.refit(rows[idx])
        trace.append((res.con_cost, res.obj_cost, idx))
        best, costs = rows[idx[0]].copy(), (float(res.con_cost[idx[0]]), float(res.obj_cost[idx[0]]))
    return best, costs, costs[0] == 0, trace


def choose(found, objectives):
    """The restart whose answer is kept: feasible, lowest objective, lowest index on a tie; None where none is feasible."""
    chosen = None
    for e, (ok, obj) in enumerate(zip(found, objectives)):
        if ok and (chosen is None or obj < objectives[chosen]):
            chosen = e
    return chosen


def find(prob, gp, noise, num_elites, start_mean, start_std, init_std=1.0):
    """The restarts: noise [iters x E x P x L].  Returns ((x0 [n_s], actions [H x n_u], objective) | None, the chosen
    restart | None, per restart (best, costs, ok, trace))."""
    per = [cem_solve(prob, gp, noise[:, e], num_elites, start_mean, start_std, init_std) for e in range(noise.shape[1])]
    e = choose([p[2] for p in per], [p[1][1] for p in per])
    if e is None:
        return None, None, per
    x0, actions = split(prob, per[e][0][None])
    return (x0[0], actions[0], per[e][1][1]), e, per
