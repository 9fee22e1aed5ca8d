"""Safe MPC with the constrained cross-entropy optimiser, solved on the GPU by libsxamd.

Drop-in for the reference's ``safe_exploration/safempc_cem.py``: same class names, constructor signature, members and
fallback ladder (``CemSafeMPC.get_action`` :231-263), so ``utils_config.create_solver``'s ``safempc_cem`` branch and the
task runners work unchanged.  What differs is underneath: instead of handing Python callbacks to the third-party
``ConstrainedCemMpc`` (H sequential dynamics calls + one constraint call per trajectory per iteration), the solver hands
the GP operands and the environment constants to ``FusedCemMpc`` (two kernel launches per CEM iteration).
"""
from enum import Enum
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from numpy import ndarray
from torch import Tensor

from . import _lib, gp_reachability_pytorch
from .costs import SaturatingCost
from .cem_mpc import (CONF_NAMES, FusedCemMpc, MultiModelCemMpc, MultiModelConsCemMpc, MultiModelPerfCemMpc, PerfSpec,
                      Rollouts, StaticCemMpc, keep_multi, multi_family, perf_spec_of)
from .gp_reachability_pytorch import make_con_set, make_env, onestep_reachability
from .safempc import SafeMPC
from .ssm_cem import gp_ssm_cem
from .ssm_cem.gp_ssm_cem import GpCemSSM
from .ssm_cem.ssm_cem import CemSSM, JunkDimensionsSSM
from .utils import assert_shape, dlqr, get_device


class MpcResult(Enum):
    """How get_action arrived at the action it returned (reference safempc_cem.py:23-27)."""
    FOUND_SOLUTION = 1
    PREVIOUS_SOLUTION = 2
    SAFE_CONTROLLER = 3


class PQFlattener:
    """(p [N x n_s], Q [N x n_s x n_s]) <-> flat [N x (n_s + n_s^2)], Q row-major; an all-zero Q block over the whole
    batch stands for "every state is a point" (reference safempc_cem.py:30-76)."""

    def __init__(self, state_dimen: int):
        self._n = state_dimen

    def get_flat_state_dimen(self) -> int:
        return self._n + self._n * self._n

    def flatten(self, p: Tensor, q: Optional[Tensor]) -> Tensor:
        n_batch = p.size(0)
        if q is None:
            q = torch.zeros((n_batch, self._n, self._n), dtype=p.dtype, device=p.device)
        assert_shape(p, (n_batch, self._n))
        assert_shape(q, (n_batch, self._n, self._n))
        return torch.cat((p.reshape(n_batch, -1), q.reshape(n_batch, -1)), dim=1)

    def unflatten(self, flat: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        n_batch = flat.size(0)
        assert_shape(flat, (n_batch, self.get_flat_state_dimen()))
        p = flat[:, :self._n]
        q = flat[:, self._n:].reshape(n_batch, self._n, self._n)
        if not bool((q != 0).any()):
            q = None
        return p, q


class ActionConstraint:
    """Box constraint on the actions; costs 3 per violating time step (reference test_safempc_cem.py:59-71)."""
    COST = 3.0

    def __init__(self, u_min, u_max):
        self.u_min = np.asarray(u_min, dtype=np.float64).reshape(-1)
        self.u_max = np.asarray(u_max, dtype=np.float64).reshape(-1)

    def __call__(self, trajectory: Tensor, actions: Tensor) -> float:
        lo = torch.as_tensor(self.u_min, dtype=actions.dtype, device=actions.device)
        hi = torch.as_tensor(self.u_max, dtype=actions.dtype, device=actions.device)
        bad = ((actions < lo) | (actions > hi)).any(dim=-1)
        return float(bad.sum().item()) * self.COST


def box2torchpoly(box) -> Tuple[np.ndarray, np.ndarray]:
    """[[lo, hi], ...] -> (u_min, u_max); stands in for constrained_cem_mpc.box2torchpoly at the reference call site
    safempc_cem.py:139."""
    box = np.asarray(box, dtype=np.float64)
    return box[:, 0], box[:, 1]


class EllipsoidStateConstraint:
    """Every state ellipsoid must lie in the polytope ``a x <= b``; cost 10 per ellipsoid that does not
    (reference safempc_cem.py:116-132).  Like the reference it looks at the LAST row of the trajectory it is given."""
    COST = 10.0
    mode = _lib.SX_CON_ALL_STATES

    def __init__(self, state_dimen: int, safe_polytope_a: np.ndarray, safe_polytope_b: np.ndarray, device: str):
        self._pq = PQFlattener(state_dimen)
        self.polytope_a = np.asarray(safe_polytope_a, dtype=np.float64)
        self.polytope_b = np.asarray(safe_polytope_b, dtype=np.float64).reshape(-1, 1)
        self._device = device
        self._polytope_a = torch.tensor(self.polytope_a, device=device)
        self._polytope_b = torch.tensor(self.polytope_b, device=device)

    def __call__(self, trajectory: Tensor, actions: Tensor) -> float:
        p, q = self._pq.unflatten(trajectory.unsqueeze(0)[:, -1])
        if q is None:
            q = torch.zeros((p.size(0), p.size(1), p.size(1)), dtype=p.dtype, device=p.device)
        inside = gp_reachability_pytorch.is_ellipsoid_inside_polytope(p.contiguous(), q.contiguous(), self._polytope_a,
                                                                      self._polytope_b)
        return float((inside.size(0) - inside.sum()).item()) * self.COST


class EllipsoidTerminalConstraint:
    """Only the terminal ellipsoid must lie in the polytope (reference safempc_cem.py:102-113)."""
    mode = _lib.SX_CON_TERMINAL

    def __init__(self, state_dimen: int, safe_polytope_a: np.ndarray, safe_polytope_b: np.ndarray, device: str):
        self._constraint = EllipsoidStateConstraint(state_dimen, safe_polytope_a, safe_polytope_b, device)
        self.polytope_a = self._constraint.polytope_a
        self.polytope_b = self._constraint.polytope_b
        self._polytope_a = self._constraint._polytope_a
        self._polytope_b = self._constraint._polytope_b

    def __call__(self, trajectory: Tensor, actions: Tensor) -> float:
        return self._constraint(trajectory[-1:, :], actions[-1:, :])


def construct_constraints(conf, env):
    """[action box, state/terminal polytope] from the environment (reference safempc_cem.py:135-146)."""
    h_mat_safe, h_safe, _, _ = env.get_safety_constraints(normalize=True)
    action_constraint = ActionConstraint(*box2torchpoly(np.array([np.array(xs) for xs in zip(env.u_min_norm,
                                                                                            env.u_max_norm)])))
    cls = EllipsoidStateConstraint if conf.use_state_constraint else EllipsoidTerminalConstraint
    return [action_constraint, cls(env.n_s, h_mat_safe, h_safe, get_device(conf))]


class LqrFeedbackController:
    """k_fb = -K_lqr for the linear prior, computed once on the host (reference safempc_simple.py:1105-1129)."""

    def __init__(self, wx_feedback_cost, wu_feedback_cost, n_s: int, n_u: int, linearized_model_a, linearized_model_b,
                 conf=None):
        self._device = get_device(conf)
        self._args = (linearized_model_a, linearized_model_b, wx_feedback_cost, wu_feedback_cost)
        self._k_fb = None

    def get_control_matrix(self) -> np.ndarray:
        if self._k_fb is None:
            self._k_fb = -dlqr(*self._args)[0]
        return self._k_fb

    def get_control_matrix_pytorch(self) -> Tensor:
        return torch.tensor(self.get_control_matrix(), device=self._device)


def objective_spec(env) -> Optional[Tuple[int, np.ndarray, np.ndarray, np.ndarray]]:
    """Maps the environment's objective hook (reference environments.py:149-156) onto the forms the rollout kernel
    evaluates: (mode, w_abs, target, w_lin).  Returns None for a hook this module does not recognise (the solver then
    evaluates the hook itself on the recorded trajectory centres)."""
    n_s = env.n_s
    zeros = np.zeros(n_s)
    probe = torch.zeros((1, n_s), dtype=torch.float64)
    if env.objective_cost_function(probe) is None:          # default: maximise the predicted variance
        return _lib.SX_OBJ_NEG_VARIANCE, zeros, zeros, zeros
    # Any hook of the separable form  sum_i w_i |t_i - p_i| + v . p  -- the pendulum's |theta_target - theta|
    # (environments.py:505-510), the lunar lander's -height (lunarlander.py:111-113) -- is identified by probing the public
    # hook alone: far from the kinks the cost along axis i is a line on either side, with slopes v_i -+ w_i that meet at t_i.
    hook = lambda x: np.asarray(env.objective_cost_function(torch.as_tensor(x, dtype=torch.float64)), dtype=np.float64).reshape(-1)
    w_abs, target, w_lin = np.zeros(n_s), np.zeros(n_s), np.zeros(n_s)
    for i in range(n_s):
        far = 1024.0
        for _ in range(2):       # second pass: probes just outside the kink found by the first (rounding ~ far * 2^-53)
            x = np.zeros((4, n_s))
            x[:, i] = [-2 * far, -far, far, 2 * far]
            c = hook(x)
            if not np.all(np.isfinite(c)):
                return None          # a hook that is not finite far out is not of this form: evaluate it as given
            s_lo, s_hi = (c[1] - c[0]) / far, (c[3] - c[2]) / far
            w_abs[i], w_lin[i] = 0.5 * (s_hi - s_lo), 0.5 * (s_hi + s_lo)
            if abs(w_abs[i]) <= 1e-12:
                w_abs[i] = 0.0
                break
            # the two lines c_lo + s_lo x and c_hi + s_hi x cross at the kink
            target[i] = ((c[1] + s_lo * far) - (c[2] - s_hi * far)) / (s_hi - s_lo)
            far = float(2.0 ** np.ceil(np.log2(2.0 * abs(target[i]) + 2.0)))
        if abs(w_lin[i]) < 1e-12 * max(1.0, abs(w_abs[i])):    # (rounding of the two slopes)
            w_lin[i] = 0.0
        if w_abs[i] != 0.0:
            # Third pass: the kink to the LAST BIT.  With a < t < b close to it, cost(b) - cost(a) = w (a + b - 2 t) + v (b - a)
            # holds exactly in a, b (the doubles actually probed), so t follows with an error of a few ulp of w * delta --
            # far below half an ulp of t: rounding the result gives the double the environment holds (the pendulum's
            # target angle), where the crossing of two lines fitted at |x| ~ 2048 was only good to ~1e-15.
            delta = 2.0 ** -8 * max(1.0, abs(target[i]))
            a, b = float(target[i] - delta), float(target[i] + delta)
            x = np.zeros((2, n_s))
            x[:, i] = [a, b]
            ca, cb = hook(x)
            if np.isfinite(ca) and np.isfinite(cb):
                target[i] = 0.5 * (a + b) - ((cb - ca) - w_lin[i] * (b - a)) / (2.0 * w_abs[i])
    test = np.random.default_rng(0).normal(size=(16, n_s))
    want = (np.abs(target[None] - test) * w_abs[None]).sum(1) + test @ w_lin
    if np.allclose(hook(test), want, rtol=1e-9, atol=1e-9):
        return _lib.SX_OBJ_AFFINE_ABS, w_abs, target, w_lin
    return None


class CemSafeMPC(SafeMPC):
    """Safe MPC whose trajectory optimisation is the fused constrained CEM on the GPU."""

    def __init__(self, ssm: CemSSM, constraints, env, conf, opt_env, wx_feedback_cost, wu_feedback_cost,
                 beta_safety: float, safe_policy: Callable[[ndarray], ndarray],
                 lqr: Optional[LqrFeedbackController] = None, mpc=None) -> None:
        super().__init__()
        self._device = get_device(conf)
        self._env = env
        self._conf = conf
        self._state_dimen = env.n_s
        self._action_dimen = env.n_u
        self._l_mu = torch.tensor(env.l_mu, device=self._device)
        self._l_sigma = torch.tensor(env.l_sigm, device=self._device)
        self._get_random_action = env.random_action
        self._pq_flattener = PQFlattener(env.n_s)
        self._ssm = ssm
        self._constraints = constraints
        self._mpc_time_horizon = conf.mpc_time_horizon
        self._beta_safety = beta_safety
        self._safe_policy = safe_policy
        self._use_prior_model = conf.use_prior_model
        self._env_objective_cost_func = env.objective_cost_function
        self._record_rollouts = bool(getattr(conf, 'plot_cem_optimisation', False)
                                     or getattr(conf, 'plot_cem_terminal_states', False))
        # The performance trajectory (FusedCemMpc): cem_n_perf steps (0 = off) sharing their first
        # cem_perf_r actions with the safety trajectory.  Settings of their own: the reference's CEM configs inherit
        # n_perf / r / type_perf_traj from the casadi defaults and must keep solving without one.
        # cem_perf_variance: the trajectory carries the GP's posterior variance (sx_cem_perf_rollout_var), and with it the
        # exploration objective of an environment without an objective_cost_function.  cem_perf_type: 'mean_equivalent' (a
        # point is propagated) or 'taylor' (sx_cem_perf_rollout_taylor: the state covariance is propagated to first order
        # under the LQR feedback, and the variance objective includes it); cem_perf_terminal_safety: the performance
        # ellipsoid at step mpc_time_horizon + 2 must lie in the safe polytope.  The casadi solver's type_perf_traj /
        # perf_safety_constr stay unread.  One PerfSpec, validated here in the settings' names and handed to the optimiser.
        self._perf = PerfSpec(getattr(conf, 'cem_n_perf', 0) or 0, getattr(conf, 'cem_perf_r', 1),
                              getattr(conf, 'cem_perf_variance', False),
                              getattr(conf, 'cem_perf_type', None) or 'mean_equivalent',
                              getattr(conf, 'cem_perf_terminal_safety', False)).checked(self._mpc_time_horizon,
                                                                                        names=CONF_NAMES)
        if self._perf.on:
            family = getattr(ssm, 'kernel_family', None)
            if mpc is None and family != 'rbf':
                raise NotImplementedError(f'cem_n_perf > 0 needs an exact RBF GP (GpCemSSM); kernel_family {family!r} has no '
                                          f'performance trajectory')
            if (self._perf.kind == 'mean'
                    and env.objective_cost_function(torch.zeros((1, env.n_s), dtype=torch.float64)) is None):
                raise ValueError('cem_n_perf > 0 needs an environment objective: the performance trajectory propagates '
                                 'means only and cannot carry the variance objective (set cem_perf_variance or '
                                 "cem_perf_type='taylor' for one that does)")

        # cem_cost_on_safety: without a performance trajectory (cem_n_perf = 0, the reference's nperf=0 configs) init_solver's
        # SaturatingCost prices the safety ellipsoids in the rollout kernel (FusedCemMpc(cost_on_safety=True), DESIGN.md
        # section 3.13).  The cost belongs to one trajectory, chosen by cem_n_perf as the reference's config chooses.
        self._cem_cost_on_safety = bool(getattr(conf, 'cem_cost_on_safety', False))
        if self._cem_cost_on_safety and self._perf.on:
            raise ValueError(f'cem_cost_on_safety prices the safety trajectory, which carries the objective only without a '
                             f'performance trajectory: got cem_n_perf={self._perf.n_perf}')
        if self._cem_cost_on_safety and mpc is None and getattr(ssm, 'kernel_family', None) != 'rbf':
            raise NotImplementedError(f'cem_cost_on_safety needs an exact RBF GP (GpCemSSM), not kernel_family '
                                      f'{getattr(ssm, "kernel_family", None)!r}')

        # cem_ctrl_ellipsoid_constraint / cem_obstacle_constraint: the reference SafeMPC's feedback bounds on the control
        # ellipsoids (k_ff_t, K Q_t K^T) and its obstacle polytope (opt_env['h_mat_obs'] / ['h_obs']; None: no rows) on the
        # intermediate safety ellipsoids, as penalties of the rollout kernel (FusedCemMpc(con_set=...), DESIGN.md section
        # 3.15).  Both off by default: the solver then calls exactly what it called without them.
        ctrl_ellipsoid = bool(getattr(conf, 'cem_ctrl_ellipsoid_constraint', False))
        obstacle = bool(getattr(conf, 'cem_obstacle_constraint', False))
        self._con_set = None
        if ctrl_ellipsoid or obstacle:
            setting = ' / '.join(name for name, on in (('cem_ctrl_ellipsoid_constraint', ctrl_ellipsoid),
                                                       ('cem_obstacle_constraint', obstacle)) if on)
            if self._perf.on:
                raise NotImplementedError(f'{setting} constrains the safety trajectory of a solve without a performance '
                                          f'trajectory: got cem_n_perf={self._perf.n_perf}')
            if mpc is None and getattr(ssm, 'kernel_family', None) != 'rbf':
                raise NotImplementedError(f'{setting} needs an exact RBF GP (GpCemSSM), not kernel_family '
                                          f'{getattr(ssm, "kernel_family", None)!r}')
            h_mat_obs = opt_env.get('h_mat_obs') if obstacle else None
            self._con_set = make_con_set(env.n_s, h_mat_obs=h_mat_obs, h_obs=None if h_mat_obs is None else opt_env['h_obs'],
                                         ctrl_ellipsoid=ctrl_ellipsoid)
            self._con_set_setting = setting

        # cem_static_ctrl_ellipsoid_constraint / cem_static_obstacle_constraint: the same two constraint groups in static
        # exploration (static_solver: StaticCemMpc(con_set=...)), where they are the reference NLP's own
        # (its gain is a fixed parameter).  Settings of their own, both off by default and independent of the two above,
        # which remain the dynamic solver's; the set is built, and a model it is not built for refused, at static_solver.
        self._static_ctrl_ellipsoid = bool(getattr(conf, 'cem_static_ctrl_ellipsoid_constraint', False))
        self._static_obstacle = bool(getattr(conf, 'cem_static_obstacle_constraint', False))
        self._static_obs_rows = ((opt_env.get('h_mat_obs'), opt_env.get('h_obs')) if self._static_obstacle
                                 else (None, None))

        linearized_model_a, linearized_model_b = opt_env['lin_model']
        self.lin_model = opt_env['lin_model']
        self._linearized_model_a = torch.tensor(linearized_model_a, device=self._device)
        self._linearized_model_b = torch.tensor(linearized_model_b, device=self._device)
        if lqr is None:
            lqr = LqrFeedbackController(wx_feedback_cost, wu_feedback_cost, env.n_s, env.n_u, linearized_model_a,
                                        linearized_model_b, conf=conf)
        self._lqr = lqr
        self._injected_mpc = mpc is not None
        self._mpc = mpc
        self._cost = None      # init_solver's SaturatingCost
        self._env_key = None
        self._objective_probe = torch.tensor([[0.3] * env.n_s, [-0.7] * env.n_s], dtype=torch.float64)
        self._last_mpc_actions = np.empty((0, self.action_dimen))
        self._mpc_actions_executed = 0
        self._batch_last_actions: Optional[List[ndarray]] = None   # per-episode ladder state of get_action_batch
        self._batch_executed: Optional[List[int]] = None
        self.last_rollouts: List[Rollouts] = []

    # ---- the reference's read-only members -----------------------------------------------------------------------
    @property
    def ssm(self) -> CemSSM:
        """exploration_runner saves ``safempc.ssm`` (reference exploration_runner.py:205-206)."""
        return self._ssm

    @property
    def state_dimen(self) -> int:
        return self._state_dimen

    @property
    def action_dimen(self) -> int:
        return self._action_dimen

    @property
    def safety_trajectory_length(self) -> int:
        return self._mpc_time_horizon

    @property
    def performance_trajectory_length(self) -> int:
        """conf.cem_n_perf: 0 (the reference's CEM solver has none, safempc_cem.py:212-215) unless that setting asks."""
        return self._perf.n_perf

    @property
    def x_train(self) -> ndarray:
        x_train = self._ssm.x_train
        if x_train is None:
            return np.empty((0, self._state_dimen + self._action_dimen))
        return x_train.detach().cpu().numpy()

    def init_solver(self, cost_func=None) -> None:
        """A `costs.SaturatingCost` becomes the objective of the performance trajectory, priced in the rollout kernel on
        every (mean, covariance) of it (what the reference's casadi configs hand over here); it needs the propagated
        covariance.  With conf.cem_cost_on_safety and no performance trajectory (cem_n_perf = 0) it becomes the objective of
        the safety trajectory, priced on every ellipsoid (p_t, Q_t) as a mean and a covariance (the reference's nperf=0
        configs).  Any other value is ignored: the objective is then the environment's."""
        if not isinstance(cost_func, SaturatingCost):
            return
        perf = perf_spec_of(self)
        on_safety = getattr(self, '_cem_cost_on_safety', False) and not perf.on
        if not on_safety and perf.kind != 'taylor':
            raise ValueError("a SaturatingCost prices (mean, covariance) pairs of the performance trajectory: it needs "
                             f"cem_perf_type='taylor' with cem_n_perf > 0, got cem_perf_type={perf.type!r}, "
                             f'cem_n_perf={perf.n_perf}; without a performance trajectory, cem_cost_on_safety prices '
                             f'the safety ellipsoids')
        self._cost = cost_func
        if self._mpc is not None:
            self._mpc.set_cost(cost_func)

    # ---- the fused optimiser -------------------------------------------------------------------------------------
    def _prior(self) -> Tuple[np.ndarray, np.ndarray]:
        a = self._linearized_model_a.cpu().numpy()
        b = self._linearized_model_b.cpu().numpy()
        if not self._use_prior_model:   # reference safempc_cem.py:291-296
            a, b = np.zeros_like(a), np.zeros_like(b)
        return a, b

    def _build_env(self) -> Tuple[_lib.SxEnv, bool]:
        """sx_env for the current problem; the bool says whether the objective must be evaluated through the hook."""
        a, b = self._prior()
        action_c = next(c for c in self._constraints if isinstance(c, ActionConstraint))
        state_c = next(c for c in self._constraints if hasattr(c, 'polytope_a'))
        spec = objective_spec(self._env)
        mode, w_abs, target, w_lin = spec if spec is not None else (_lib.SX_OBJ_NEG_VARIANCE, None, None, None)
        if spec is None and self._perf.on:
            # the hook is evaluated on the performance trajectory's recorded means; the kernels' own objective (all-zero
            # weights here) is overwritten
            mode = _lib.SX_OBJ_AFFINE_ABS
        env = make_env(self._state_dimen, self._action_dimen, a=a, b=b, k_fb=self._lqr.get_control_matrix(),
                       l_mu=self._l_mu.cpu().numpy(), l_sigma=self._l_sigma.cpu().numpy(), beta=self._beta_safety,
                       h_mat=state_c.polytope_a, h_vec=state_c.polytope_b, u_min=action_c.u_min, u_max=action_c.u_max,
                       obj_mode=mode, obj_w_abs=w_abs, obj_target=target, obj_w_lin=w_lin, con_mode=state_c.mode)
        return env, spec is None

    def _solver(self):
        if self._injected_mpc:
            return self._mpc
        if getattr(self._ssm, 'kernel_family', None) not in ('rbf', 'feature', 'mlp', 'stepwise', 'rbf_junk',
                                                                'feature_junk', 'mlp_junk'):
            raise NotImplementedError('the fused CEM solver needs a HIP-backed CemSSM (GpCemSSM, McDropoutSSM, '
                                      'GalConcreteDropoutSSM, or JunkDimensionsSSM over one of them); other CemSSMs are outside '
                                      'the accelerated path')
        # the problem constants only change when the environment moves its objective (the pendulum's target angle,
        # environments.py:505-510): probe the hook at two fixed points and rebuild sx_env only when the answers change
        probe = self._env_objective_cost_func(self._objective_probe)
        key = None if probe is None else tuple(float(v) for v in probe.reshape(-1))
        if self._mpc is not None and key == self._env_key:
            return self._mpc
        env, needs_hook = self._build_env()
        if self._mpc is None:
            # cem_init_std: a scalar or one value per step; cem_warm_start: 'zero' (the reference's cold start) or
            # 'safe_policy' (FusedCemMpc.safe_policy_plan) -- both optional additions to the reference's config
            self._mpc = FusedCemMpc(self._ssm, env, self._mpc_time_horizon, self._conf.cem_num_rollouts,
                                    self._conf.cem_num_elites, self._conf.cem_num_iterations, device=self._device,
                                    seed=int(getattr(self._conf, 'cem_seed', 0)),
                                    init_std=getattr(self._conf, 'cem_init_std', 1.0),
                                    warm_start=getattr(self._conf, 'cem_warm_start', None) or 'zero',
                                    record_rollouts=self._record_rollouts, **self._perf.keywords(),
                                    **({'cost_on_safety': True} if getattr(self, '_cem_cost_on_safety', False) else {}),
                                    **({} if getattr(self, '_con_set', None) is None else {'con_set': self._con_set}))
            if self._cost is not None:
                self._mpc.set_cost(self._cost)
        self._mpc.set_env(env, objective_hook=self._env_objective_cost_func if needs_hook else None)
        self._env_key = key
        return self._mpc

    def static_solver(self, n_restarts: int, sample_mean, sample_std) -> StaticCemMpc:
        """The solver of static exploration (StaticSafeMPCExploration): the start state is optimised with the actions, from
        the distribution (sample_mean, sample_std) [n_s], in `n_restarts` problems side by side.  Built over this solver's
        model, its constraint set with the variance objective, mpc_time_horizon and the cem_num_* settings.  The model is
        read at solve time, so the solver stays valid across update_model.  conf.cem_static_ctrl_ellipsoid_constraint /
        conf.cem_static_obstacle_constraint add the feedback bounds and the obstacle rows (opt_env['h_mat_obs'] / ['h_obs'];
        None: no rows) to it: StaticCemMpc(con_set=...)."""
        ctrl_ellipsoid = getattr(self, '_static_ctrl_ellipsoid', False)
        obstacle = getattr(self, '_static_obstacle', False)
        con_kw = {}
        if ctrl_ellipsoid or obstacle:
            setting = ' / '.join(name for name, on in (('cem_static_ctrl_ellipsoid_constraint', ctrl_ellipsoid),
                                                       ('cem_static_obstacle_constraint', obstacle)) if on)
            if getattr(self._ssm, 'kernel_family', None) != 'rbf':
                raise NotImplementedError(f'{setting} needs an exact RBF GP (GpCemSSM), not kernel_family '
                                          f'{getattr(self._ssm, "kernel_family", None)!r}')
            h_mat_obs, h_obs = self._static_obs_rows
            con_kw['con_set'] = make_con_set(self._state_dimen, h_mat_obs=h_mat_obs,
                                             h_obs=None if h_mat_obs is None else h_obs, ctrl_ellipsoid=ctrl_ellipsoid)
        elif getattr(self, '_con_set', None) is not None:
            # (the dynamic solver's set says nothing about the static solve: its settings are the two above)
            raise NotImplementedError(f'static exploration is not built for {self._con_set_setting}')
        if isinstance(self._ssm, JunkDimensionsSSM):
            raise NotImplementedError('static exploration is not built for JunkDimensionsSSM')
        env, _ = self._build_env()
        return StaticCemMpc(self._ssm, env, self._mpc_time_horizon, self._conf.cem_num_rollouts, self._conf.cem_num_elites,
                            self._conf.cem_num_iterations, start_mean=sample_mean, start_std=sample_std,
                            n_restarts=n_restarts, seed=int(getattr(self._conf, 'cem_seed', 0)),
                            init_std=getattr(self._conf, 'cem_init_std', 1.0), device=self._device,
                            record_rollouts=self._record_rollouts, **con_kw)

    def _flat_points(self, states: ndarray) -> Tensor:
        """Point states [E x n_s] as the optimiser's flat states [E x (n_s + n_s^2)] (PQFlattener.flatten(p, None): an
        all-zero Q block), assembled on the host: ONE host->device copy instead of a copy, a fill and a concatenation."""
        flat = np.zeros((states.shape[0], self._pq_flattener.get_flat_state_dimen()), dtype=np.float64)
        flat[:, :self._state_dimen] = states
        return torch.tensor(flat, device=self._device)

    def get_action(self, state: ndarray) -> Tuple[ndarray, MpcResult]:
        assert_shape(state, (self._state_dimen,))
        mpc_actions, rollouts = self._solver().get_actions(self._flat_points(np.asarray(state)[None]))
        mpc_actions = mpc_actions.detach().cpu().numpy() if mpc_actions is not None else mpc_actions
        self.last_rollouts = rollouts
        # the reference's ladder (safempc_cem.py:243-263): fresh solution, else the rest of the previous one, else the
        # safe controller
        if mpc_actions is not None:
            action = mpc_actions[0]
            self._last_mpc_actions = mpc_actions
            self._mpc_actions_executed = 1
            result = MpcResult.FOUND_SOLUTION
        elif self._mpc_actions_executed < self._last_mpc_actions.shape[0]:
            action = self._last_mpc_actions[self._mpc_actions_executed]
            self._mpc_actions_executed += 1
            result = MpcResult.PREVIOUS_SOLUTION
        else:
            action = self._safe_policy(state)
            result = MpcResult.SAFE_CONTROLLER
        return action, result

    def get_action_batch(self, states: ndarray, episode_ids=None, num_episodes: Optional[int] = None
                         ) -> Tuple[ndarray, List[MpcResult]]:
        """``get_action`` for independent episodes in lockstep (BASELINE config 5): states [A x n_s] ->
        (actions [A x n_u], one MpcResult per row).  One fused solve serves all rows; each episode keeps its own
        PREVIOUS_SOLUTION / SAFE_CONTROLLER ladder (reference safempc_cem.py:243-263).  `episode_ids` names the episode
        of each row (default 0 .. A-1) out of `num_episodes` -- a lockstep runner passes the episodes that are still
        running, and their ladders carry on where they were.  The ladder state is allocated by the first call and
        whenever `num_episodes` changes (``reset_batch`` starts over)."""
        states = np.asarray(states)
        if states.ndim != 2 or states.shape[1] != self._state_dimen:
            raise ValueError(f'Wanted shape (E, {self._state_dimen}), got {states.shape}')
        A = states.shape[0]
        ids = list(range(A)) if episode_ids is None else [int(e) for e in episode_ids]
        E = int(num_episodes) if num_episodes is not None else max(max(ids) + 1, A)
        if len(ids) != A or len(set(ids)) != A or min(ids) < 0 or max(ids) >= E:
            raise ValueError(f'episode_ids must name {A} distinct episodes out of {E}, got {ids}')
        if self._batch_last_actions is None or len(self._batch_last_actions) != E:
            self._batch_last_actions = [np.empty((0, self.action_dimen)) for _ in range(E)]
            self._batch_executed = [0] * E
        best, found, rollouts = self._solver().get_actions_batch(self._flat_points(states))
        best = best.detach().cpu().numpy()
        self.last_rollouts = rollouts
        actions: List[ndarray] = []
        results: List[MpcResult] = []
        for k, e in enumerate(ids):
            action, result = self._batch_ladder(e, states[k], best[k], bool(found[k]))
            actions.append(action)
            results.append(result)
        return np.stack(actions), results

    def _batch_ladder(self, e: int, state: ndarray, best: ndarray, found: bool) -> Tuple[ndarray, MpcResult]:
        """Episode e's rung of the reference's ladder (safempc_cem.py:243-263) for a solve that returned `best` [H x n_u]
        (`found`): fresh solution, else the rest of the previous one, else the safe controller."""
        if found:
            self._batch_last_actions[e] = best
            self._batch_executed[e] = 1
            return best[0], MpcResult.FOUND_SOLUTION
        if self._batch_executed[e] < self._batch_last_actions[e].shape[0]:
            action = self._batch_last_actions[e][self._batch_executed[e]]
            self._batch_executed[e] += 1
            return action, MpcResult.PREVIOUS_SOLUTION
        return np.asarray(self._safe_policy(state)), MpcResult.SAFE_CONTROLLER

    def reset_batch(self) -> None:
        self._batch_last_actions = None
        self._batch_executed = None

    def get_action_verbose(self, state: ndarray):
        raise NotImplementedError

    # ---- the reference's dynamics callback, kept for callers that step the model themselves ------------------------
    def _dynamics_func(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor]:
        """One particle-batch step on flat states (reference safempc_cem.py:288-302)."""
        ps, qs = self._pq_flattener.unflatten(states)
        a, b = self._prior()
        a, b = torch.tensor(a, device=states.device), torch.tensor(b, device=states.device)
        p_next, q_next, sigma = onestep_reachability(ps.contiguous(), self._ssm, actions, self._l_mu, self._l_sigma, qs,
                                                     k_fb=self._lqr.get_control_matrix_pytorch(), a=a, b=b, verbose=0,
                                                     c_safety=self._beta_safety)
        return self._pq_flattener.flatten(p_next, q_next), self._compute_objective_cost(p_next, sigma)

    def _compute_objective_cost(self, p_next: Tensor, sigma: Tensor) -> Tensor:
        objective_cost = self._env_objective_cost_func(p_next)
        if objective_cost is None:
            objective_cost = -torch.sum(sigma, dim=1)
        return objective_cost

    # ---- model maintenance ---------------------------------------------------------------------------------------
    def update_model(self, x: ndarray, y: ndarray, opt_hyp=False, replace_old=True, reinitialize_solver=True) -> None:
        """The model learns the error to the linear prior (reference safempc_cem.py:314-327)."""
        x_s, x_u = x[:, :self.state_dimen], x[:, self.state_dimen:]
        y_error = y - self.eval_prior(x_s, x_u) if self._use_prior_model else y
        self._ssm.update_model(torch.tensor(x, device=self._device), torch.tensor(y_error, device=self._device), opt_hyp,
                               replace_old)

    def information_gain(self) -> Union[ndarray, List[None]]:
        """Per-output information gain 1/2 log det(I + K / noise) when the model can report it (the reference returns
        a list of None, which exploration_runner.py:192 cannot store)."""
        if hasattr(self._ssm, 'information_gain'):
            return self._ssm.information_gain()
        return np.full(self.state_dimen, np.nan)

    def ssm_predict(self, z: ndarray) -> Tuple[ndarray, ndarray]:
        mean, sigma = self._ssm.predict_raw(torch.tensor(z, device=self._device))
        return mean.detach().cpu().numpy(), sigma.detach().cpu().numpy()

    def eval_prior(self, states: ndarray, actions: ndarray):
        a = self._linearized_model_a.cpu().numpy()
        b = self._linearized_model_b.cpu().numpy()
        return np.dot(states, a.T) + np.dot(actions, b.T)

    def collect_metrics(self) -> Dict[str, float]:
        return self._ssm.collect_metrics()


def multi_solve_applies(mpcs: Sequence) -> bool:
    """Do these single-model optimisers go through one MultiModelCemMpc (get_actions_multi)?  Unsharded FusedCemMpc
    instances without an objective hook whose models share one kernel_family with a multi-model rollout: exact RBF GPs,
    feature-space GPs ('linear', 'nn') or MC-dropout ensembles.  (Whether one launch then serves the models -- no workspace
    path, one architecture -- is MultiModelCemMpc.fused_applies: a solve per model otherwise.  A hook is never evaluated
    beside a cost on the safety trajectory, cost_on_safety: such solvers go through it with the cost.)"""
    return (all(isinstance(m, FusedCemMpc) and (m._objective_hook is None or m._safety_cost is not None) and m._world == 1
                for m in mpcs)
            and multi_family([m._ssm for m in mpcs]) is not None)


def get_actions_multi(solvers: Sequence[CemSafeMPC], states: ndarray) -> Tuple[ndarray, List[MpcResult]]:
    """``get_action`` of several independent solvers at once -- the reference's exploration scenarios, each with its own
    model and data (episode_runner.py:40-123) -- where solver e acts in states[e] ([E x n_s]).  Returns (actions
    [E x n_u], one MpcResult per solver).

    Over models of one family -- exact RBF GPs, feature-space GPs or MC-dropout ensembles -- that is ONE solve for all of
    them (``MultiModelCemMpc``: one rollout launch per CEM iteration, each problem with its own model; solvers that all
    have a performance trajectory with one ``cem_n_perf``, ``cem_perf_r``, ``cem_perf_variance``, ``cem_perf_type`` and
    ``cem_perf_terminal_safety`` go through ``MultiModelPerfCemMpc``, which adds one performance-rollout launch per
    iteration for all of them, ``cem_perf_type='taylor'`` included; solvers that all have
    ``cem_ctrl_ellipsoid_constraint`` / ``cem_obstacle_constraint`` on, with one constraint set, go through
    ``MultiModelConsCemMpc``, whose launch carries the set); otherwise (mixed families, JunkDimensionsSSM, ...),
    and where the single launch does not apply, one solve per solver.  Either way
    problem e draws solver e's noise, and each solver keeps its own PREVIOUS_SOLUTION / SAFE_CONTROLLER ladder, the one
    ``get_action_batch`` keeps for a single episode.  The solvers must agree on the environment constants (sx_env) and
    the CEM settings; ValueError otherwise."""
    solvers = list(solvers)
    states = np.asarray(states)
    if not solvers:
        raise ValueError('get_actions_multi needs at least one solver')
    # the constraint set (cem_ctrl_ellipsoid_constraint / cem_obstacle_constraint): all solvers or none, with one set
    with_set = [s for s in solvers if getattr(s, '_con_set', None) is not None]
    if with_set and len(with_set) != len(solvers):
        raise NotImplementedError(f'get_actions_multi takes solvers that all have a constraint set or all have none: '
                                  f'{len(with_set)} of {len(solvers)} have {with_set[0]._con_set_setting}; those act one at '
                                  f'a time (get_action), or together in a call of their own')
    # the performance trajectory (cem_n_perf > 0): all solvers or none, with one spec
    perf = [perf_spec_of(s) for s in solvers]
    with_perf = any(p.on for p in perf)
    if with_perf and not all(p.on for p in perf):
        raise NotImplementedError('get_actions_multi takes solvers that all have a performance trajectory or all have none: '
                                  f'got cem_n_perf = {[p.n_perf for p in perf]}; the ones with cem_n_perf > 0 act one at a time '
                                  f'(get_action), or together in a call of their own')
    if with_perf and len(set(perf)) != 1:
        raise ValueError('the solvers of get_actions_multi must share the performance trajectory\'s settings: got '
                         f'(cem_n_perf, cem_perf_r, cem_perf_variance, cem_perf_type, cem_perf_terminal_safety) = '
                         f'{[tuple(p) for p in perf]}')
    n_s, n_u = solvers[0].state_dimen, solvers[0].action_dimen
    if states.ndim != 2 or states.shape != (len(solvers), n_s):
        raise ValueError(f'Wanted shape ({len(solvers)}, {n_s}), got {states.shape}')
    for s in solvers:
        if (s.state_dimen, s.action_dimen) != (n_s, n_u):
            raise ValueError('the solvers of get_actions_multi must share (n_s, n_u)')
        if s._batch_last_actions is None or len(s._batch_last_actions) != 1:
            s._batch_last_actions = [np.empty((0, n_u))]
            s._batch_executed = [0]
    mpcs = [s._solver() for s in solvers]
    (MultiModelConsCemMpc if with_set else MultiModelCemMpc).check_solvers(mpcs)
    flat = torch.cat([s._flat_points(states[e:e + 1]) for e, s in enumerate(solvers)])
    if multi_solve_applies(mpcs):
        cls = MultiModelPerfCemMpc if with_perf else MultiModelConsCemMpc if with_set else MultiModelCemMpc
        multi = keep_multi((getattr(solvers[0], '_multi', None) or (None, None))[1], cls, mpcs)
        solvers[0]._multi = (tuple(id(m) for m in mpcs), multi)
        best, found = multi.get_actions_multi(flat)
        best = best.detach().cpu().numpy()
    else:
        per = [m.get_actions_batch(flat[e:e + 1]) for e, m in enumerate(mpcs)]
        best = np.concatenate([p[0].detach().cpu().numpy() for p in per])
        found = [bool(p[1][0]) for p in per]
    actions: List[ndarray] = []
    results: List[MpcResult] = []
    for e, s in enumerate(solvers):
        s.last_rollouts = []
        action, result = s._batch_ladder(0, states[e], best[e], bool(found[e]))
        actions.append(action)
        results.append(result)
    return np.stack(actions), results


def update_models_multi(solvers: Sequence[CemSafeMPC], xs: Sequence[ndarray], ys: Sequence[ndarray], opt_hyp=False,
                        replace_old=True) -> None:
    """``update_model`` of several independent solvers at once -- the counterpart of ``get_actions_multi`` for the
    reference's retraining of every scenario's model after an episode (episode_runner.py:55,123): solver e's model learns
    the error of (xs[e], ys[e]) to its linear prior, as ``CemSafeMPC.update_model``.  Exact RBF GPs of one shape train in
    lockstep (``gp_ssm_cem.update_models_multi``: one fit and one MLL-gradient launch sequence per Adam step for all of
    them), with the results of one update_model per solver; other models are updated one at a time."""
    _update_models_multi(solvers, xs, ys, opt_hyp, replace_old,
                         lambda s, x_s, x_u, y: y - s.eval_prior(x_s, x_u) if s._use_prior_model else y)


def _update_models_multi(solvers, xs, ys, opt_hyp, replace_old, prior_error) -> None:
    """`update_models_multi` of this module and of cautious_mpc: solver e's model learns `prior_error(solver, states,
    actions, targets)` of (xs[e], ys[e])."""
    solvers, xs, ys = list(solvers), list(xs), list(ys)
    if not len(solvers) == len(xs) == len(ys):
        raise ValueError(f'{len(solvers)} solvers, {len(xs)} input sets, {len(ys)} target sets')
    xs_t, ys_t = [], []
    for s, x, y in zip(solvers, xs, ys):
        xs_t.append(torch.tensor(x, device=s._device))
        ys_t.append(torch.tensor(prior_error(s, x[:, :s.state_dimen], x[:, s.state_dimen:], y), device=s._device))
    gp_ssm_cem.update_models_multi([s._ssm for s in solvers], xs_t, ys_t, opt_hyp, replace_old)
