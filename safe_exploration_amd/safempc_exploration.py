"""Exploration modules over a ready-made SafeMPC: the reference's ``DynamicSafeMPCExploration``
(``safe_exploration/safempc_exploration.py:357-393``) and ``StaticSafeMPCExploration`` (``:56-334``, over the CEM solver
with the start state as a decision variable), plus the multi-episode form of ``find_max_variance`` that
``exploration_runner`` can call once per iteration for all of its parallel explorations."""
from typing import List, Optional, Sequence, Tuple

import numpy as np
from numpy import ndarray

from .safempc import SafeMPC


class DynamicSafeMPCExploration:
    def __init__(self, safempc: SafeMPC, env):
        self.safempc = safempc
        self.env = env
        self.n_s = safempc.state_dimen
        self.n_u = safempc.action_dimen
        self.n_safe = safempc.safety_trajectory_length
        self.n_perf = safempc.performance_trajectory_length
        self.safempc.init_solver(None)

    def find_max_variance(self, x_0: ndarray, sol_verbose: bool = False) -> Tuple[ndarray, ndarray]:
        """(x_0 [n_s x 1], u_apply [n_u x 1]) -- reference :372-374."""
        u_apply, _ = self.safempc.get_action(x_0)
        return x_0[:, None], u_apply[:, None]

    def find_max_variance_batch(self, x_0: ndarray) -> Tuple[ndarray, ndarray, List]:
        """E start states [E x n_s] -> (x_0 [E x n_s], u_apply [E x n_u], one MpcResult per episode): ONE fused solve."""
        u_apply, results = self.safempc.get_action_batch(np.atleast_2d(x_0))
        return np.atleast_2d(x_0), u_apply, results

    def find_max_variance_verbose(self, x_0: ndarray, sol_verbose: bool = False):
        return self.safempc.get_action_verbose(x_0)      # (raises NotImplementedError for the CEM solver, as the reference)

    def update_model(self, x, y, train=False, replace_old=False):
        self.safempc.update_model(x, y, train, replace_old)

    def get_information_gain(self):
        return self.safempc.information_gain()

    @property
    def x_train(self) -> ndarray:
        return self.safempc.x_train

    def ssm_predict(self, z: ndarray) -> Tuple[ndarray, ndarray]:
        return self.safempc.ssm_predict(z)


class StaticSafeMPCExploration:
    """Static exploration (reference :56-334): every sample is a distinct (x, u), so the start state is optimised with
    the actions.  Where the reference solves ``n_restarts_optimizer`` casadi NLPs over ``[p_0, u_0, k_ff]`` from random
    guesses and keeps the best feasible one (:281-330), this class runs ``n_restarts_optimizer`` CEM problems over the rows
    ``[x0 | actions]`` side by side (``CemSafeMPC.static_solver``, DESIGN.md sections 3.10 and 5) and keeps the feasible one
    with the lowest variance objective.  The start distribution is the reference's ``env._sample_start_state(sample_mean,
    sample_std)`` (normalised); a start outside the safe polytope is infeasible (this library's rule)."""

    def __init__(self, safempc: SafeMPC, env, n_restarts_optimizer: int = 1, sample_mean=None, sample_std=None,
                 verbosity: int = 1):
        if not hasattr(safempc, 'static_solver'):
            raise NotImplementedError('static exploration needs a CemSafeMPC (static_solver): the casadi solver is outside '
                                      'the accelerated path')
        self.safempc = safempc
        self.env = env
        self.n_s = safempc.state_dimen
        self.n_u = safempc.action_dimen
        self.T = safempc.safety_trajectory_length
        self.n_restarts_optimizer = n_restarts_optimizer
        self.sample_mean = sample_mean
        self.sample_std = sample_std
        self.verbosity = verbosity
        # env._sample_start_state(mean, std, normalize=True): std * randn + mean, scaled by inv_norm[0]
        scale = np.asarray(env.inv_norm[0], dtype=np.float64)
        mean = np.asarray(env.init_m if sample_mean is None else sample_mean, dtype=np.float64) * np.ones(self.n_s)
        std = np.asarray(env.init_std if sample_std is None else sample_std, dtype=np.float64) * np.ones(self.n_s)
        self.start_mean, self.start_std = mean * scale, std * np.abs(scale)
        self.safempc.init_solver(None)
        self._solver = safempc.static_solver(n_restarts_optimizer, self.start_mean, self.start_std)

    def find_max_variance(self, x0=None, sol_verbose: bool = False) -> Tuple[Optional[ndarray], Optional[ndarray]]:
        """(x_best [n_s x 1], u_best [n_u x 1]), or (None, None) where no restart found a feasible sample -- reference
        :281-330.  `x0` is unused, as in the reference ("in static setting we optimize over x_i")."""
        found = self._solver.find()
        if found is None:
            return None, None
        x_best, actions, obj = found
        if self.verbosity > 1:
            print(f'New feasible solution with sigma sum {-obj} found')
        return np.asarray(x_best, dtype=np.float64).reshape(self.n_s, 1), np.asarray(actions[0], dtype=np.float64).reshape(
            self.n_u, 1)

    def find_max_variance_verbose(self, x0=None, sol_verbose: bool = False):
        raise NotImplementedError('static exploration has no verbose solve: the runner disables verification in static mode')

    def update_model(self, x, y, train=False, replace_old=False):
        self.safempc.update_model(x, y, train, replace_old)

    def get_information_gain(self):
        return self.safempc.information_gain()

    @property
    def x_train(self) -> ndarray:
        return self.safempc.x_train

    def ssm_predict(self, z: ndarray) -> Tuple[ndarray, ndarray]:
        return self.safempc.ssm_predict(z)


def find_max_variance_multi(explorations: Sequence[DynamicSafeMPCExploration], x_0: ndarray
                            ) -> Tuple[ndarray, ndarray, List]:
    """``find_max_variance`` of E independent explorations -- the reference's scenarios, each with its own model -- at
    once: exploration e starts from x_0[e] ([E x n_s]).  One ``safempc_cem.get_actions_multi`` over their solvers (with
    ``cem_n_perf`` / ``cem_perf_variance`` the multi-model solve looks n_perf steps ahead for every scenario in the same
    launches; explorations whose solvers all carry one constraint set -- ``cem_ctrl_ellipsoid_constraint`` /
    ``cem_obstacle_constraint`` -- go through the multi-model launch with the set, unchanged here).  Returns (x_0 [E x n_s], u_apply [E x n_u], one MpcResult per exploration): row e is what
    ``explorations[e].find_max_variance(x_0[e])`` returns."""
    from .safempc_cem import get_actions_multi
    x_0 = np.atleast_2d(x_0)
    u_apply, results = get_actions_multi([x.safempc for x in explorations], x_0)
    return x_0, u_apply, results


def find_max_variance_static_multi(explorations: Sequence[StaticSafeMPCExploration]
                                   ) -> List[Tuple[Optional[ndarray], Optional[ndarray]]]:
    """``find_max_variance`` of S independent static explorations -- the reference's scenarios, each with its own model --
    at once: entry s is what ``explorations[s].find_max_variance()`` returns, (x [n_s x 1], u [n_u x 1]) or (None, None).
    One ``MultiModelStaticCemMpc`` over their solvers: every scenario with all of its restarts in one rollout launch and one
    ranking launch per CEM iteration (with ``cem_static_ctrl_ellipsoid_constraint`` / ``cem_static_obstacle_constraint`` on
    all of them, the launch with their one constraint set), each scenario drawing its own solver's noise.  The multi-model
    solver is kept on the first exploration between calls and rebuilt when the list of solvers changes.  The models are
    updated in lockstep with ``safempc_cem.update_models_multi([x.safempc for x in explorations], ...)``."""
    from .cem_mpc import MultiModelStaticCemMpc, keep_multi
    explorations = list(explorations)
    if not explorations:
        raise ValueError('find_max_variance_static_multi needs at least one exploration')
    for x in explorations:
        if not isinstance(x, StaticSafeMPCExploration):
            raise TypeError(f'find_max_variance_static_multi takes StaticSafeMPCExploration instances, got '
                            f'{type(x).__name__} (find_max_variance_multi serves the dynamic explorations)')
    solvers = [x._solver for x in explorations]
    explorations[0]._static_multi = cached = keep_multi(getattr(explorations[0], '_static_multi', None),
                                                        MultiModelStaticCemMpc, solvers)
    out = []
    for x, found in zip(explorations, cached.find()):
        if found is None:
            out.append((None, None))
            continue
        x_best, actions, obj = found
        if x.verbosity > 1:
            print(f'New feasible solution with sigma sum {-obj} found')
        out.append((np.asarray(x_best, dtype=np.float64).reshape(x.n_s, 1),
                    np.asarray(actions[0], dtype=np.float64).reshape(x.n_u, 1)))
    return out
