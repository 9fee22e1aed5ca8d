"""Is the ellipsoidal over-approximation sound for a fitted model?  The reference's third task runner
(``safe_exploration/uncertainty_propagation_runner.py:14-73``) in its ``random_actions`` mode, the only one it runs (the
flag is hard-coded there; the other branch is the casadi solver's ``solve``).

Per rollout, in the reference's draw order, a random feedback law is drawn -- ``k_fb = .1 randn(n_safe - 1, n_u, n_s)``,
``k_ff = .1 randn(n_safe, n_u)`` -- and a start ``x_0 = env.reset()``.  The ellipsoids of ALL rollouts are then propagated
by one ``gp_reachability_pytorch.multistep_reachability`` call (one launch on an exact RBF GP), where the reference makes
one ``multistep_reachability`` call per rollout and one ``onestep_reachability`` per step inside it.  The closed loop
``u_i = K_{i-1} (x_i - p_{i-1}) + k_ff_i`` on the true system (``env.simulate_onestep``, host code as in the reference) and
the test ``(x - p)^T Q^{-1} (x - p) < 1`` per step follow, per rollout, in numpy.

``simulate_trajectory`` and ``trajectory_inside_ellipsoid`` stand where the reference's ``gp_reachability.py:272-302,342-375``
do; written for this module.
"""
import numpy as np
import torch

from . import gp_reachability_pytorch
from .utils import get_device

RESULT_KEYS = ('inside_ellipsoid_per_step', 'inside_ellipsoid_all', 'x_all', 'p_all', 'q_all')


def simulate_trajectory(env, x_0, k_fb, k_ff, p_ctrl):
    """The true system under the feedback law: x_all [(n + 1) x n_s] with x_all[0] = x_0, the first action k_ff[0] and from
    then on u_i = k_fb[i - 1] (x_i - p_ctrl[i - 1]) + k_ff[i], each step one ``env.simulate_onestep(x, u)[0]``.
    k_fb [(n - 1) x n_u x n_s] (unused for n = 1), k_ff [n x n_u], p_ctrl [>= (n - 1) x n_s]: the centres the law refers to."""
    k_ff = np.asarray(k_ff, dtype=np.float64)
    n, n_u = k_ff.shape
    x = np.asarray(x_0, dtype=np.float64).reshape(-1)
    n_s = x.size
    k_fb = np.asarray(k_fb, dtype=np.float64).reshape(n - 1, n_u, n_s)
    p_ctrl = np.asarray(p_ctrl, dtype=np.float64).reshape(-1, n_s)
    x_all = np.empty((n + 1, n_s))
    x_all[0] = x
    for i in range(n):
        u = k_ff[i] if i == 0 else k_fb[i - 1] @ (x - p_ctrl[i - 1]) + k_ff[i]
        x = np.asarray(env.simulate_onestep(x, u)[0], dtype=np.float64).reshape(n_s)
        x_all[i + 1] = x
    return x_all


def inside_ellipsoid(x, p, q):
    """(x - p)^T q^{-1} (x - p) < 1 for one state, centre and shape matrix."""
    d = np.asarray(x, dtype=np.float64).reshape(-1) - np.asarray(p, dtype=np.float64).reshape(-1)
    return bool(d @ np.linalg.solve(np.asarray(q, dtype=np.float64), d) < 1.0)


def trajectory_inside_ellipsoid(env, x_0, p_all, q_all, k_fb, k_ff, return_states=False):
    """bool [n]: is the state the true system reaches after action i inside the ellipsoid (p_all[i], q_all[i])?  p_all
    [n x n_s], q_all [n x n_s x n_s] (or [n x n_s^2]).  `return_states`: also x_all [(n + 1) x n_s] of the simulation."""
    p_all = np.asarray(p_all, dtype=np.float64)
    n, n_s = p_all.shape
    q_all = np.asarray(q_all, dtype=np.float64).reshape(n, n_s, n_s)
    x_all = simulate_trajectory(env, x_0, k_fb, k_ff, p_all)
    inside = np.array([inside_ellipsoid(x_all[i + 1], p_all[i], q_all[i]) for i in range(n)], dtype=bool)
    return (inside, x_all) if return_states else inside


def run_uncertainty_propagation(env, safempc, conf):
    """The reference's runner: `conf.n_rollouts` random feedback laws over `conf.n_safe` steps on `safempc.ssm`, with the
    solver's linear prior (`safempc.lin_model`), `env.l_mu`, `env.l_sigm` and `conf.beta_safety`.  Returns (and with
    `conf.save_results` saves as ``<conf.save_path>/res_data.npy``) the reference's dictionary: inside_ellipsoid_per_step
    [R x n], inside_ellipsoid_all [R], x_all [R x (n + 1) x n_s], p_all [R x n x n_s], q_all [R x n x n_s x n_s]."""
    R, n, n_s, n_u = int(conf.n_rollouts), int(conf.n_safe), env.n_s, env.n_u
    k_fb_all, k_ff_all, x_0_all = np.empty((R, n - 1, n_u, n_s)), np.empty((R, n, n_u)), np.empty((R, n_s))
    for i in range(R):
        k_fb_all[i] = .1 * np.random.randn(n - 1, n_u, n_s)
        k_ff_all[i] = .1 * np.random.randn(n, n_u)
        x_0_all[i] = np.asarray(env.reset()).reshape(n_s)

    ssm = safempc.ssm
    x_train = getattr(ssm, 'x_train', None)
    dev = x_train.device if x_train is not None else torch.device(get_device(conf))
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
    a, b = safempc.lin_model
    _, _, p_all, q_all = gp_reachability_pytorch.multistep_reachability(
        t(x_0_all), ssm, t(k_fb_all), t(k_ff_all), t(np.asarray(env.l_mu).reshape(n_s)),
        t(np.asarray(env.l_sigm).reshape(n_s)), c_safety=conf.beta_safety, verbose=0, a=t(a), b=t(b))
    p_all = np.asarray(p_all.detach().cpu().numpy() if torch.is_tensor(p_all) else p_all, dtype=np.float64)
    q_all = np.asarray(q_all.detach().cpu().numpy() if torch.is_tensor(q_all) else q_all, dtype=np.float64)

    x_all = np.empty((R, n + 1, n_s))
    per_step = np.empty((R, n))
    inside_all = np.empty((R,))
    for i in range(R):
        inside, x_all[i] = trajectory_inside_ellipsoid(env, x_0_all[i], p_all[i], q_all[i], k_fb_all[i], k_ff_all[i],
                                                       return_states=True)
        per_step[i] = inside
        inside_all[i] = np.all(inside)
    results = dict(zip(RESULT_KEYS, (per_step, inside_all, x_all, p_all, q_all)))
    if getattr(conf, 'save_results', False):
        np.save('{}/res_data'.format(conf.save_path), results)
    print_results(per_step, inside_all, conf)
    return results


def print_results(inside_ellipsoid_per_step, inside_ellipsoid_all, conf):
    """The share of rollouts inside their ellipsoid, per step and over the whole trajectory (conf.verbosity > 0)."""
    if getattr(conf, 'verbosity', 0) <= 0:
        return
    R = float(len(inside_ellipsoid_all))
    per_step = np.sum(inside_ellipsoid_per_step, axis=0) / R
    print('\n=====Uncertainty propagation=====')
    print('Per step percentage of system states inside ellipsoid:')
    print('Step              ' + ''.join('| {}  '.format(i) for i in range(len(per_step))))
    print('Inside Percentage ' + ''.join('| {} '.format(v) for v in per_step))
    print(' Trajectory safety percentage: {}'.format(float(np.sum(inside_ellipsoid_all)) / R))
