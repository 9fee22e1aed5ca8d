"""Cautious MPC over the constrained cross-entropy optimiser, solved on the GPU by libsxamd.

Stands where the reference has ``safe_exploration/cautious_mpc.py``'s ``CautiousMPC`` (the ``cautious_mpc`` branch of
``utils_config.create_solver``): one trajectory under the fixed feedback ``k_fb``, propagated to first order
(``type_perf_traj = 'taylor'``) or mean-equivalent, with chance constraints at ``beta_safety`` on every control and every
state (``generate_safety_constraints``, cautious_mpc.py:337-442).  The surface -- ``get_action``'s ladder
(``_get_old_solution``), the warm start (``_get_init_controls``), ``update_model``, ``n_fail``, ``k_fb`` -- is the
reference's; the NLP is not: ``CautiousCemMpc`` ranks sampled rows by (constraint cost, objective) where the reference hands
IPOPT one NLP, and the objective is the environment's separable objective or ``-tr G_t`` (DESIGN.md sections 3.11, 7).
"""
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from numpy import ndarray

from . import _lib
from .cem_mpc import CautiousCemMpc, MultiModelCautiousCemMpc, Rollouts, keep_multi
from .costs import SaturatingCost
from .gp_reachability_pytorch import make_env
from .safempc import SafeMPC
from .ssm_cem import gp_ssm_cem
from .safempc_cem import LqrFeedbackController, MpcResult, _update_models_multi, objective_spec
from .utils import assert_shape, get_device

PERF_TRAJECTORIES = ('taylor', 'mean_equivalent')
STATE_POLYTOPES = ('obs', 'safe')


class CautiousCemMPC(SafeMPC):
    """Cautious MPC whose trajectory optimisation is the fused constrained CEM on the GPU.

    Read from ``conf``: ``T`` (the horizon), ``beta_safety`` (the constructor's argument where it is not None),
    ``type_perf_traj`` ('taylor' | 'mean_equivalent'), ``cautious_state_polytope`` ('obs', the reference's: ``h_mat_obs`` /
    ``h_obs`` of ``opt_env``, no rows when None; or 'safe': ``h_mat_safe`` / ``h_safe``) and the ``cem_*`` settings of
    ``CemSafeMPC``.  The action bounds are ``opt_env['ctrl_bounds']`` [n_u x 2]."""

    def __init__(self, ssm, env, conf, opt_env, wx_feedback_cost, wu_feedback_cost, beta_safety: Optional[float] = None,
                 safe_policy: Optional[Callable[[ndarray], ndarray]] = None, lqr: Optional[LqrFeedbackController] = None,
                 mpc=None) -> None:
        super().__init__()
        self._device = get_device(conf)
        self._env, self._conf, self._ssm = env, conf, ssm
        self._state_dimen, self._action_dimen = env.n_s, env.n_u
        self.T = int(conf.T)
        if self.T < 1:
            raise ValueError(f'conf.T={conf.T} must be at least 1')
        self.beta_safety = float(beta_safety if beta_safety is not None else conf.beta_safety)
        self._perf_trajectory = getattr(conf, 'type_perf_traj', None) or 'mean_equivalent'
        if self._perf_trajectory not in PERF_TRAJECTORIES:
            raise NotImplementedError(f'type_perf_traj must be one of {PERF_TRAJECTORIES}, got {self._perf_trajectory!r}')
        self._polytope = getattr(conf, 'cautious_state_polytope', None) or 'obs'
        if self._polytope not in STATE_POLYTOPES:
            raise ValueError(f'cautious_state_polytope must be one of {STATE_POLYTOPES}, got {self._polytope!r}')
        n_s, n_u = env.n_s, env.n_u
        h_mat, h_vec = ((opt_env.get('h_mat_obs'), opt_env.get('h_obs')) if self._polytope == 'obs'
                        else (opt_env['h_mat_safe'], opt_env['h_safe']))
        if h_mat is None:
            h_mat, h_vec = np.zeros((0, n_s)), np.zeros((0, 1))
        self._h_mat = np.asarray(h_mat, dtype=np.float64).reshape(-1, n_s)
        self._h_vec = np.asarray(h_vec, dtype=np.float64).reshape(-1, 1)
        if self._h_mat.shape[0] != self._h_vec.shape[0]:
            raise ValueError('the state polytope\'s matrix and vector must have one row each per inequality')
        bounds = opt_env.get('ctrl_bounds')
        if bounds is None:
            raise ValueError("opt_env['ctrl_bounds'] is needed: the CEM samples unbounded rows")
        self.ctrl_bounds = np.asarray(bounds, dtype=np.float64)
        if self.ctrl_bounds.shape != (n_u, 2):
            raise ValueError(f'ctrl_bounds must be [{n_u} x 2] (lower, upper), got {self.ctrl_bounds.shape}')
        self.lin_model = opt_env['lin_model']
        self._a = np.asarray(self.lin_model[0], dtype=np.float64)
        self._b = np.asarray(self.lin_model[1], dtype=np.float64)
        if lqr is None:
            lqr = LqrFeedbackController(wx_feedback_cost, wu_feedback_cost, n_s, n_u, self._a, self._b, conf=conf)
        self._lqr = lqr
        self._safe_policy = safe_policy
        self._record_rollouts = bool(getattr(conf, 'plot_cem_optimisation', False))
        self._injected_mpc = mpc is not None
        self._mpc = mpc
        self._cost = None      # init_solver's SaturatingCost
        self._env_key = None
        self._objective_probe = torch.tensor([[0.3] * n_s, [-0.7] * n_s], dtype=torch.float64)
        # the reference's ladder state (cautious_mpc.py:64, 273-275): no solution yet, so the first failure is answered by k_fb
        self.n_fail = self.T - 1
        self.k_ff_old = np.zeros((self.T, n_u))
        self._batch_old: Optional[List[ndarray]] = None      # per-episode ladder state of get_action_batch
        self._batch_fail: Optional[List[int]] = None
        self.last_rollouts: List[Rollouts] = []

    # ---- the reference's members ----------------------------------------------------------------------------------
    @property
    def k_fb(self) -> ndarray:
        return self._lqr.get_control_matrix()

    @property
    def ssm(self):
        return self._ssm

    @property
    def state_dimen(self) -> int:
        return self._state_dimen

    @property
    def action_dimen(self) -> int:
        return self._action_dimen

    @property
    def safety_trajectory_length(self) -> int:
        return self.T

    @property
    def performance_trajectory_length(self) -> int:
        return 0

    @property
    def x_train(self) -> ndarray:
        x_train = self._ssm.x_train
        if x_train is None:
            return np.empty((0, self._state_dimen + self._action_dimen))
        return x_train.detach().cpu().numpy()

    def init_solver(self, cost_func=None) -> None:
        """A `costs.SaturatingCost` becomes the optimiser's objective, priced in the rollout kernel on every (mean,
        covariance) of the plan (what the reference's casadi configs hand over here); any other value is ignored: the
        objective is then the environment's."""
        if isinstance(cost_func, SaturatingCost):
            self._cost = cost_func
            if self._mpc is not None:
                self._mpc.set_cost(cost_func)

    # ---- the fused optimiser --------------------------------------------------------------------------------------
    def _build_env(self) -> Tuple[_lib.SxEnv, bool]:
        """sx_env for the current problem (the polytope is the chosen one); the bool says whether the objective must be
        evaluated through the hook."""
        spec = objective_spec(self._env)
        mode, w_abs, target, w_lin = spec if spec is not None else (_lib.SX_OBJ_AFFINE_ABS, None, None, None)
        n_s = self._state_dimen
        env = make_env(n_s, self._action_dimen, a=self._a, b=self._b, k_fb=self.k_fb, l_mu=np.asarray(self._env.l_mu),
                       l_sigma=np.asarray(self._env.l_sigm), beta=self.beta_safety, h_mat=self._h_mat, h_vec=self._h_vec,
                       u_min=self.ctrl_bounds[:, 0], u_max=self.ctrl_bounds[:, 1], obj_mode=mode, obj_w_abs=w_abs,
                       obj_target=target, obj_w_lin=w_lin)
        return env, spec is None

    def _solver(self):
        if self._injected_mpc:
            return self._mpc
        probe = self._env.objective_cost_function(self._objective_probe)
        key = None if probe is None else tuple(float(v) for v in probe.reshape(-1))
        if self._mpc is not None and key == self._env_key:
            return self._mpc
        env, needs_hook = self._build_env()
        if self._mpc is None:
            self._mpc = CautiousCemMpc(self._ssm, env, self.T, self._conf.cem_num_rollouts, self._conf.cem_num_elites,
                                       self._conf.cem_num_iterations, propagate=self._perf_trajectory == 'taylor',
                                       device=self._device, seed=int(getattr(self._conf, 'cem_seed', 0)),
                                       init_std=getattr(self._conf, 'cem_init_std', 1.0),
                                       record_rollouts=self._record_rollouts)
            if self._cost is not None:
                self._mpc.set_cost(self._cost)
        self._mpc.set_env(env, objective_hook=self._env.objective_cost_function if needs_hook else None)
        self._env_key = key
        return self._mpc

    def _flat_points(self, states: ndarray) -> torch.Tensor:
        n_s = self._state_dimen
        flat = np.zeros((states.shape[0], n_s + n_s * n_s), dtype=np.float64)
        flat[:, :n_s] = states
        return torch.tensor(flat, device=self._device)

    # ---- the reference's ladder and warm start --------------------------------------------------------------------
    @staticmethod
    def _init_controls(n_fail: int, k_ff_old: ndarray) -> ndarray:
        """_get_init_controls (cautious_mpc.py:320-335): the previous row shifted by one step, its last entry repeated,
        where the previous solve succeeded; zeros otherwise."""
        if n_fail == 0:
            return np.vstack((k_ff_old[1:], k_ff_old[-1:]))
        return np.zeros_like(k_ff_old)

    def _old_solution(self, n_fail: int, k_ff_old: ndarray, state: ndarray) -> Tuple[ndarray, MpcResult]:
        """_get_old_solution (cautious_mpc.py:290-318) after n_fail failures: the kept row's entry n_fail, then k_fb x."""
        if n_fail < self.T:
            return k_ff_old[n_fail].reshape(self._action_dimen), MpcResult.PREVIOUS_SOLUTION
        u = self._safe_policy(state) if self._safe_policy is not None else np.dot(self.k_fb, state)
        return np.asarray(u, dtype=np.float64).reshape(self._action_dimen), MpcResult.SAFE_CONTROLLER

    def _rung(self, n_fail: int, k_ff_old: ndarray, state: ndarray, row: Optional[ndarray]):
        """(action, result, n_fail, k_ff_old) after a solve that found `row` [T x n_u], or None."""
        if row is not None:
            return row[0].copy(), MpcResult.FOUND_SOLUTION, 0, row
        n_fail += 1
        action, result = self._old_solution(n_fail, k_ff_old, state)
        return action, result, n_fail, k_ff_old

    def _warm(self, starts: List[ndarray]) -> torch.Tensor:
        return torch.tensor(np.stack(starts), dtype=torch.float64, device=self._device)

    def get_action(self, state: ndarray) -> Tuple[ndarray, MpcResult]:
        state = np.asarray(state, dtype=np.float64)
        assert_shape(state, (self._state_dimen,))
        init = self._warm([self._init_controls(self.n_fail, self.k_ff_old)])
        row, rollouts = self._solver().get_actions(self._flat_points(state[None]), init_mean=init)
        self.last_rollouts = rollouts
        row = row.detach().cpu().numpy() if row is not None else None
        action, result, self.n_fail, self.k_ff_old = self._rung(self.n_fail, self.k_ff_old, state, row)
        return action, result

    def get_action_batch(self, states: ndarray, episode_ids=None, num_episodes: Optional[int] = None
                         ) -> Tuple[ndarray, List[MpcResult]]:
        """``get_action`` for independent episodes in lockstep, with ``CemSafeMPC.get_action_batch``'s signature: states
        [A x n_s] -> (actions [A x n_u], one MpcResult per row); every episode keeps its own ladder and warm start."""
        states = np.asarray(states, dtype=np.float64)
        if states.ndim != 2 or states.shape[1] != self._state_dimen:
            raise ValueError(f'Wanted shape (E, {self._state_dimen}), got {states.shape}')
        A = states.shape[0]
        ids = list(range(A)) if episode_ids is None else [int(e) for e in episode_ids]
        E = int(num_episodes) if num_episodes is not None else max(max(ids) + 1, A)
        if len(ids) != A or len(set(ids)) != A or min(ids) < 0 or max(ids) >= E:
            raise ValueError(f'episode_ids must name {A} distinct episodes out of {E}, got {ids}')
        if self._batch_old is None or len(self._batch_old) != E:
            self._batch_old = [np.zeros((self.T, self._action_dimen)) for _ in range(E)]
            self._batch_fail = [self.T - 1] * E
        init = self._warm([self._init_controls(self._batch_fail[e], self._batch_old[e]) for e in ids])
        best, found, rollouts = self._solver().get_actions_batch(self._flat_points(states), init_mean=init)
        best = best.detach().cpu().numpy()
        self.last_rollouts = rollouts
        actions, results = [], []
        for k, e in enumerate(ids):
            action, result, self._batch_fail[e], self._batch_old[e] = self._rung(
                self._batch_fail[e], self._batch_old[e], states[k], best[k].copy() if bool(found[k]) else None)
            actions.append(action)
            results.append(result)
        return np.stack(actions), results

    def reset_batch(self) -> None:
        self._batch_old = self._batch_fail = None

    def get_action_verbose(self, state: ndarray):
        """(action, result, means [(T + 1) x n_s] with the start prepended, covariances Sigma_1 .. Sigma_T [T x n_s x n_s],
        row [T x n_u], margins [T x 2]: per step the largest state and the largest control distance) of the best row; the
        last four are None where no row was found (cautious_mpc.py:277-287)."""
        action, result = self.get_action(state)
        if result != MpcResult.FOUND_SOLUTION:
            return action, result, None, None, None, None
        x0 = torch.tensor(np.asarray(state, dtype=np.float64)[None], device=self._device)
        row = torch.tensor(self.k_ff_old[None, None], dtype=torch.float64, device=self._device)
        out = self._solver().evaluate(x0, row)
        means = np.vstack((np.asarray(state, dtype=np.float64)[None], out['traj'][0, 0].cpu().numpy()))
        return action, result, means, out['cov'][0, 0].cpu().numpy(), self.k_ff_old.copy(), out['margins'][0, 0].cpu().numpy()

    # ---- model maintenance ----------------------------------------------------------------------------------------
    def update_model(self, x: ndarray, y: ndarray, opt_hyp=False, replace_old=True, reinitialize_solver=True) -> None:
        """The model learns the error to the linear prior (cautious_mpc.py:444-479; there is no solver to reinitialise)."""
        x_s, x_u = x[:, :self._state_dimen], x[:, self._state_dimen:]
        y_error = y - self.eval_prior(x_s, x_u)
        self._ssm.update_model(torch.tensor(x, device=self._device), torch.tensor(y_error, device=self._device), opt_hyp,
                               replace_old)

    def information_gain(self):
        if hasattr(self._ssm, 'information_gain'):
            return self._ssm.information_gain()
        return np.full(self._state_dimen, np.nan)

    def ssm_predict(self, z: ndarray) -> Tuple[ndarray, ndarray]:
        mean, sigma = self._ssm.predict_raw(torch.tensor(z, device=self._device))
        return mean.detach().cpu().numpy(), sigma.detach().cpu().numpy()

    def eval_prior(self, states: ndarray, actions: ndarray):
        return np.dot(states, self._a.T) + np.dot(actions, self._b.T)

    def collect_metrics(self) -> Dict[str, float]:
        return self._ssm.collect_metrics()


def get_actions_multi(solvers: Sequence[CautiousCemMPC], states: ndarray) -> Tuple[ndarray, List[MpcResult]]:
    """``get_action`` of several independent Cautious MPC solvers at once -- the cautious arm of the reference's
    experiments, each scenario with its own model and data (episode_runner.py:40-123) -- where solver e acts in states[e]
    ([E x n_s]).  Returns (actions [E x n_u], one MpcResult per solver).

    Over ``CautiousCemMpc`` optimisers that is ONE solve for all of them (``MultiModelCautiousCemMpc``: one rollout launch
    per CEM iteration, each problem with its own GP; where the single launch does not apply, one solve per solver); injected
    optimisers of another kind solve one at a time.  Either way problem e draws solver e's noise, and every solver keeps its
    own ladder (``n_fail``, ``k_ff_old``) and warm start (``_init_controls``), exactly as its own ``get_action`` would.  The
    solvers must agree on the CEM settings, the environment constants (sx_env) and the cost; ValueError otherwise."""
    solvers = list(solvers)
    states = np.asarray(states, dtype=np.float64)
    if not solvers:
        raise ValueError('get_actions_multi needs at least one solver')
    n_s, n_u = solvers[0].state_dimen, solvers[0].action_dimen
    if states.ndim != 2 or states.shape != (len(solvers), n_s):
        raise ValueError(f'Wanted shape ({len(solvers)}, {n_s}), got {states.shape}')
    for s in solvers:
        if not isinstance(s, CautiousCemMPC):
            raise ValueError(f'cautious_mpc.get_actions_multi takes CautiousCemMPC solvers, got {type(s).__name__}')
        if (s.state_dimen, s.action_dimen, s.T) != (n_s, n_u, solvers[0].T):
            raise ValueError('the solvers of get_actions_multi must share (n_s, n_u) and T')
    mpcs = [s._solver() for s in solvers]
    MultiModelCautiousCemMpc.check_solvers(mpcs)
    starts = [s._init_controls(s.n_fail, s.k_ff_old) for s in solvers]
    flat = torch.cat([s._flat_points(states[e:e + 1]) for e, s in enumerate(solvers)])
    if all(isinstance(m, CautiousCemMpc) for m in mpcs):
        multi = keep_multi((getattr(solvers[0], '_multi', None) or (None, None))[1], MultiModelCautiousCemMpc, mpcs)
        solvers[0]._multi = (tuple(id(m) for m in mpcs), multi)
        best, found = multi.get_actions_multi(flat, init_mean=solvers[0]._warm(starts))
        rows = [best[e].detach().cpu().numpy().copy() if bool(found[e]) else None for e in range(len(solvers))]
    else:
        rows = []
        for e, (s, m) in enumerate(zip(solvers, mpcs)):
            row, _ = m.get_actions(flat[e:e + 1], init_mean=s._warm(starts[e:e + 1]))
            rows.append(row.detach().cpu().numpy() if row is not None else None)
    actions: List[ndarray] = []
    results: List[MpcResult] = []
    for e, s in enumerate(solvers):
        s.last_rollouts = []
        action, result, s.n_fail, s.k_ff_old = s._rung(s.n_fail, s.k_ff_old, states[e], rows[e])
        actions.append(action)
        results.append(result)
    return np.stack(actions), results


def update_models_multi(solvers: Sequence[CautiousCemMPC], xs: Sequence[ndarray], ys: Sequence[ndarray], opt_hyp=False,
                        replace_old=True) -> None:
    """``update_model`` of several independent Cautious MPC solvers at once, the counterpart of ``get_actions_multi`` for
    the reference's retraining of every scenario's model after an episode (episode_runner.py:55,123): solver e's model
    learns the error of (xs[e], ys[e]) to its linear prior, as ``CautiousCemMPC.update_model``, and the exact GPs train in
    lockstep (``gp_ssm_cem.update_models_multi``)."""
    _update_models_multi(solvers, xs, ys, opt_hyp, replace_old, lambda s, x_s, x_u, y: y - s.eval_prior(x_s, x_u))
