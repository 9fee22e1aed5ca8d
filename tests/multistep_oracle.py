"""The numpy oracle of multi-step reachability under a feedback gain per rollout and step (test infrastructure; used by
test_multistep_host.py and test_gpu_multistep.py).

``multistep`` chains ``oracle.reachability.onestep_reachability`` per rollout and step with that step's gain -- P = 1,
k_fb = None at step 0 (a point start), k_fb[t - 1] at step t >= 1 -- which is the reference's
gp_reachability.multistep_reachability (:168-221) with q_0 = k_fb_init = None.  ``rollout`` adds what sx_cem_rollout_starts
charges around it, as tests/static_explore_oracle.py does: the objective, the action box, the polytope in the problem's
constraint mode, and STATE_VIOLATION_COST once for a start outside the polytope.  A rollout whose chain raises (a NaN at one
of the reference's checks) has NaN outputs from that step on and STATUS_NAN in its status."""
import dataclasses

import numpy as np

from oracle import cem as ocem
from oracle import reachability as oreach


def multistep(gp, p_0, k_fb, k_ff, l_mu, l_sigma, c_safety, a=None, b=None):
    """p_0 [R x n_s], k_fb [R x (n - 1) x n_u x n_s], k_ff [R x n x n_u] -> (p_all [R x n x n_s], q_all [R x n x n_s x n_s],
    sigma [R x n x n_s], status [R])."""
    p_0, k_fb, k_ff = np.asarray(p_0, dtype=np.float64), np.asarray(k_fb, dtype=np.float64), np.asarray(k_ff, dtype=np.float64)
    R, n_s = p_0.shape
    n = k_ff.shape[1]
    p_all, q_all = np.full((R, n, n_s), np.nan), np.full((R, n, n_s, n_s), np.nan)
    sigma, status = np.full((R, n, n_s), np.nan), np.zeros(R, dtype=np.int64)
    for i in range(R):
        p, q = p_0[i:i + 1], None
        for t in range(n):
            try:
                with np.errstate(invalid='ignore'):
                    p, q, sig, st = oreach.onestep_reachability(p, gp, k_ff[i:i + 1, t], l_mu, l_sigma, q,
                                                                None if t == 0 else k_fb[i, t - 1], c_safety, a=a, b=b)
            except (ValueError, AssertionError, np.linalg.LinAlgError):
                status[i] |= oreach.STATUS_NAN
                break
            status[i] |= st
            p_all[i, t], q_all[i, t], sigma[i, t] = p[0], q[0], sig[0]
    return p_all, q_all, sigma, status


def rollout(prob, gp, rows, gains, variance_objective=False):
    """One problem of sx_cem_rollout_gains: rows [P x (n_s + H n_u)] = [x0 | k_ff], gains [P x (H - 1) x n_u x n_s];
    prob.k_fb is not read.  An oracle.cem.RolloutResult with per-particle status [P] and `start_cost` [P]."""
    if variance_objective:
        prob = dataclasses.replace(prob, obj_mode=ocem.OBJ_NEG_VARIANCE)
    rows = np.asarray(rows, dtype=np.float64)
    P, n_s, n_u = rows.shape[0], prob.n_s, prob.n_u
    H = (rows.shape[1] - n_s) // n_u
    x0, k_ff = rows[:, :n_s], rows[:, n_s:].reshape(P, H, n_u)
    p_all, q_all, sigma, status = multistep(gp, x0, gains, k_ff, prob.l_mu, prob.l_sigma, prob.beta, prob.a, prob.b)
    out = ocem.RolloutResult(p_all, q_all, sigma, np.zeros(P), np.zeros(P), status)
    for t in range(H):
        out.obj_cost += ocem.objective_cost(prob, p_all[:, t], sigma[:, t])
        u = k_ff[:, t]
        out.con_cost += ocem.ACTION_VIOLATION_COST * ((u < prob.u_min[None]) | (u > prob.u_max[None])).any(axis=1)
        if prob.con_mode == ocem.CON_ALL_STATES or t == H - 1:
            with np.errstate(invalid='ignore'):
                inside = oreach.is_ellipsoid_inside_polytope(p_all[:, t], q_all[:, t], prob.h_mat, prob.h_vec)
            out.con_cost += ocem.STATE_VIOLATION_COST * (~inside)
    inside0 = oreach.is_ellipsoid_inside_polytope(x0, np.zeros((P, n_s, n_s)), prob.h_mat, prob.h_vec)
    out.start_cost = ocem.STATE_VIOLATION_COST * (~inside0)
    out.con_cost = out.con_cost + out.start_cost
    return out


def rel_err(got, want, q_all):
    """max |got - want| relative to max(1, max |Q_t|) of the oracle's shape matrices: the convention of the multi-step checks
    (|Q| grows to ~12 at the pendulum fixture and ~120 at the cart-pole one)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(q_all))))
    return float(np.max(np.abs(got - want))) / scale if got.size else 0.0


def load_golden(path):
    """A multistep_*.npz fixture and the oracle GP over its training set."""
    from oracle.gp import ExactGP
    g = np.load(path)
    return g, ExactGP(g['X'], g['Y'], g['ls'], g['s'], g['noise'])
