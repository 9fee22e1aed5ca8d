"""State-space-model interface consumed by the CEM safe-MPC solver (torch tensors in, torch tensors out).

Mirrors the surface of the reference's ``safe_exploration/ssm_cem/ssm_cem.py:11-131`` so a model written against one
works with the other.
"""
from abc import ABC, abstractmethod
from typing import Any, Callable, Dict, Optional, Tuple

import torch
from torch import Tensor

from ..utils import assert_shape

# (n_s, n_u, query shift) that sx_cem_rollout_junk rolls out in one launch per iteration: shift 0 is sx_cem_rollout's
# shapes, shift > 0 the query-shifted ones (n_s + n_u + shift <= SX_MAX_D): SX_ROLLOUT_SHAPES in csrc/sx_stream_launch.hpp
JUNK_FUSED_SHAPES = frozenset({(2, 1, 0), (4, 1, 0), (2, 2, 0), (4, 2, 0), (3, 1, 0), (1, 1, 0),
                               (2, 1, 1), (4, 1, 1), (3, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 1), (1, 1, 1)})
# (n_s, n_u, query shift) that sx_cem_rollout_feat_junk / sx_cem_rollout_mlp_junk roll out in one launch per iteration: shift
# 0 is sx_cem_rollout_feat's / sx_cem_rollout_mlp's shapes, shift > 0 every shape a padded feature-GP or MC-dropout model
# can be built for (n_s + J_s <= 4, n_u + J_a <= 2): SX_MODEL_JUNK_SHAPES in csrc/sx_model_shapes.hpp
JUNK_MODEL_FUSED_SHAPES = frozenset({(2, 1, 0), (4, 1, 0), (2, 2, 0), (4, 2, 0), (3, 1, 0), (1, 1, 0),
                                     (1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 1)})


class CemSSM(ABC):
    def __init__(self, state_dimen: int, action_dimen: int):
        self.num_states = state_dimen
        self.num_actions = action_dimen
        self._x_train: Optional[Tensor] = None
        self._y_train: Optional[Tensor] = None

    # ---- training data -------------------------------------------------------------------------------------------
    @property
    def x_train(self) -> Optional[Tensor]:
        return self._x_train

    @property
    def y_train(self) -> Optional[Tensor]:
        return self._y_train

    def update_model(self, train_x: Tensor, train_y: Tensor, opt_hyp=False, replace_old=False) -> None:
        """train_x [N x (n_s+n_u)], train_y [N x n_s]; merges with the stored data unless replace_old.

        Hyper-parameters are re-fitted when opt_hyp is set or the model is parametric.
        """
        n = train_x.size(0)
        assert_shape(train_x, (n, self.num_states + self.num_actions))
        assert_shape(train_y, (n, self.num_states))
        if not replace_old and self._x_train is not None and self._y_train is not None:
            train_x = torch.cat((self._x_train, train_x), dim=0)
            train_y = torch.cat((self._y_train, train_y), dim=0)
        self._x_train, self._y_train = train_x, train_y
        self._update_model(train_x, train_y)
        if opt_hyp or self.parametric:
            self._train_model(train_x, train_y)

    @abstractmethod
    def _update_model(self, x_train: Tensor, y_train: Tensor) -> None:
        ...

    @abstractmethod
    def _train_model(self, x_train: Tensor, y_train: Tensor) -> None:
        ...

    # ---- prediction ----------------------------------------------------------------------------------------------
    @abstractmethod
    def predict_with_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        """states [N x n_s], actions [N x n_u] -> mean [N x n_s], var [N x n_s], jac [N x n_s x (n_s+n_u)]."""

    @abstractmethod
    def predict_without_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor]:
        """states [N x n_s], actions [N x n_u] -> mean [N x n_s], var [N x n_s]."""

    @abstractmethod
    def predict_raw(self, z: Tensor) -> Tuple[Tensor, Tensor]:
        """z [N x (n_s+n_u)] -> mean [n_s x N], var [n_s x N] (outputs first, as the reference's GpCemSSM)."""

    def _join_states_actions(self, states: Tensor, actions: Tensor) -> Tensor:
        n = states.size(0)
        assert_shape(states, (n, self.num_states))
        assert_shape(actions, (n, self.num_actions))
        return torch.cat((states, actions), dim=1)

    # ---- bookkeeping ---------------------------------------------------------------------------------------------
    @abstractmethod
    def collect_metrics(self) -> Dict[str, Any]:
        ...

    @property
    @abstractmethod
    def parametric(self) -> bool:
        ...


class JunkDimensionsSSM(CemSSM):
    """Wraps an SSM, padding every call with zero-valued junk state / action dimensions (the reference's way of trying
    an SSM in a higher-dimensional setting, ssm_cem/ssm_cem.py:134-210; created by utils_config._create_cem_ssm:46-47).

    Mirrors the reference exactly, including where the junk goes: states -> [states, junk], actions -> [actions, junk],
    raw inputs -> [z, all junk]; outputs are cut back to the leading real dimensions (the Jacobian to its leading
    n_s + n_u columns, as the reference does).  It works with any CemSSM at this surface -- the HIP-backed GpCemSSM
    directly while the padded sizes stay within its limits (n_s <= 4, n_u <= 2), and beyond them in a FOLDED form that gives
    the padded model's numbers (`_construct_folded`).

    The CEM solver (CemSafeMPC / FusedCemMpc) takes the wrapper too.  The wrapper's placement of the junk is not a GP over
    the real dimensions -- training rows are [z, junk] but queries [states, junk, actions, junk], so with junk states the
    action meets training columns that only ever held zeros, and the "action" columns of the returned Jacobian are
    derivatives with respect to junk STATE inputs -- but over an exact RBF GP it is an exact GP over the columns that are
    ever non-zero, [0, n_s + n_u) and [n_s + J_s, n_s + J_s + n_u): training rows [x, u, 0_s], queries [x, 0_s, u],
    s = `query_shift` = min(J_s, n_u), real outputs only.  That model (`real_output_view`) is what the fused rollout
    sx_cem_rollout_junk takes (`kernel_family = 'rbf_junk'`, one launch per CEM iteration).  The same reduction holds for
    a feature-space GP ('linear', 'nn') and an MC-dropout model, whose inputs meet the junk only in the first linear layer:
    `kernel_family = 'feature_junk'` / 'mlp_junk' (sx_cem_rollout_feat_junk / sx_cem_rollout_mlp_junk,
    ssm_cem/kept_columns.py).  Every other inner model, and shapes the kernels are not instantiated for, are rolled out
    STEP BY STEP (`kernel_family = 'stepwise'`: H x (predict through this wrapper + sx_onestep_reach) per CEM iteration, the way the reference's optimiser
    drives its dynamics callback).  Both reproduce the reference's numbers, the Jacobian's "action" block included.
    """

    def __init__(self, constructor: Callable[..., CemSSM], state_dimen: int, action_dimen: int, junk_states: int,
                 junk_actions: int):
        super().__init__(state_dimen, action_dimen)
        self._junk_states = junk_states
        self._junk_actions = junk_actions
        self._cols: Optional[Tensor] = None      # folded form: the padded input columns the inner model keeps
        self._constructor = constructor
        self._view: Optional[CemSSM] = None      # real-output model of the fused rollout (built on first use)
        self._view_of = None                     # ... and the inner device model it was built from
        try:
            self._ssm = constructor(state_dimen=state_dimen + junk_states, action_dimen=action_dimen + junk_actions)
        except ValueError as too_large:
            self._ssm = self._construct_folded(constructor, too_large)

    def _construct_folded(self, constructor: Callable[..., CemSSM], too_large: Exception) -> CemSSM:
        """Padded sizes beyond the inner model's limits (the reference's experiment goes to 5 junk states,
        notebooks/results.ipynb cell 15: 7 states for the pendulum).  For an exact GP with an ARD RBF kernel the padded model
        FOLDS exactly: an input column that is zero in every training row AND in every query adds nothing to any kernel value,
        the outputs are independent GPs (the junk outputs are cut off anyway), and a length-scale that never meets a non-zero
        difference has no gradient.  Training rows are [z, junk] (non-zero columns 0 .. n_s + n_u), queries [states, junk,
        actions, junk] (non-zero columns 0 .. n_s and n_s + J .. n_s + J + n_u): the inner model is built over the union of
        those columns with the real outputs only -- for J >= n_u that is n_s states and 2 n_u "actions" -- and gives the
        padded model's numbers for the real outputs, the returned Jacobian's leading n_s + n_u columns included."""
        n_s, n_u, js = self.num_states, self.num_actions, self._junk_states
        keep = sorted(set(range(n_s + n_u)) | set(range(n_s + js, n_s + js + n_u)))
        try:
            inner = constructor(state_dimen=n_s, action_dimen=len(keep) - n_s)
        except ValueError:
            raise too_large from None
        if getattr(inner, 'kernel_family', None) != 'rbf':
            raise too_large     # (only the RBF exact GP is known to fold exactly)
        self._cols = torch.tensor(keep, dtype=torch.long)
        return inner

    @property
    def query_shift(self) -> int:
        """s = min(J_s, n_u): the junk columns between the states and the actions of a query in the real-output model."""
        return min(self._junk_states, self.num_actions)

    def _kept_columns(self) -> Tuple[int, ...]:
        n_s, n_u, js = self.num_states, self.num_actions, self._junk_states
        return tuple(sorted(set(range(n_s + n_u)) | set(range(n_s + js, n_s + js + n_u))))

    def _model_junk_family(self) -> Optional[str]:
        """'feature_junk' / 'mlp_junk' for an inner model that IS a FeatureGpCemSSM / McDropoutSSM (GalConcreteDropoutSSM
        included): decided on the class, since only these classes' device models are known to reduce to the kept columns."""
        from .dropout_ssm_cem import McDropoutSSM
        from .feature_gp_ssm_cem import FeatureGpCemSSM
        if isinstance(self._ssm, FeatureGpCemSSM):
            return 'feature_junk'
        if isinstance(self._ssm, McDropoutSSM):
            return 'mlp_junk'
        return None

    @property
    def kernel_family(self) -> str:
        """'rbf_junk' (fused rollout, sx_cem_rollout_junk) over an RBF exact GP, 'feature_junk' (sx_cem_rollout_feat_junk)
        over a feature-space GP and 'mlp_junk' (sx_cem_rollout_mlp_junk) over an MC-dropout model, where the kernel is
        instantiated for (n_s, n_u, query_shift); 'stepwise' otherwise."""
        shape = (self.num_states, self.num_actions, self.query_shift)
        if getattr(self._ssm, 'kernel_family', None) == 'rbf':
            return 'rbf_junk' if shape in JUNK_FUSED_SHAPES else 'stepwise'
        family = self._model_junk_family()
        if family is None or shape not in JUNK_MODEL_FUSED_SHAPES:
            return 'stepwise'
        return family

    def real_output_view(self) -> CemSSM:
        """The exact GP over the kept columns with the n_s real outputs (n_s states, n_u + query_shift "actions"): the
        model sx_cem_rollout_junk takes.  Folded wrappers: the inner model itself.  Otherwise a GpCemSSM built through the
        wrapper's constructor on first use, with the inner model's hyper-parameters of the first n_s outputs at the kept
        columns (K over the kept columns is K over the padded ones entry for entry), rebuilt whenever the inner model's
        device model changes (new training data or hyper-parameters).  Over a feature-space GP or an MC-dropout model: a
        `kept_columns.KeptColumnView` (`_model_view`)."""
        if self._cols is not None:
            return self._ssm
        family = self._model_junk_family()
        if family is not None:
            return self._model_view(family)
        inner_model = self._ssm.device_model
        if self._view is None or self._view_of is not inner_model:
            n_s, cols = self.num_states, list(self._kept_columns())
            view = self._constructor(state_dimen=n_s, action_dimen=len(cols) - n_s, wide_inputs=True)
            state = self._ssm.state_dict()
            view.load_state_dict({'gp_model': {'raw_lengthscale': state['gp_model']['raw_lengthscale'][:n_s][:, cols],
                                               'raw_outputscale': state['gp_model']['raw_outputscale'][:n_s]},
                                  'gp_likelihood': {'raw_noise': state['gp_likelihood']['raw_noise'][:n_s],
                                                    'noise_floor': state['gp_likelihood']['noise_floor']}})
            x = self._x_train
            view.update_model(torch.cat((x, x.new_zeros((x.size(0), self.query_shift))), dim=1), self._y_train,
                              opt_hyp=False, replace_old=True)
            self._view, self._view_of = view, inner_model
        return self._view

    def _model_view(self, family: str) -> CemSSM:
        """real_output_view over a feature-space GP or an MC-dropout model (ssm_cem/kept_columns.py): the inner model's
        current parameters at the kept columns, rebuilt whenever its device model changes (new data, training, a
        re-initialised or re-frozen ensemble)."""
        from . import kept_columns
        inner_model = self._ssm.feat_model if family == 'feature_junk' else self._ssm.mlp_model
        if self._view is None or self._view_of is not inner_model:
            n_s, cols = self.num_states, list(self._kept_columns())
            if family == 'feature_junk':
                x = self._x_train
                view = kept_columns.feature_view(self._ssm, cols, n_s,
                                                 torch.cat((x, x.new_zeros((x.size(0), self.query_shift))), dim=1),
                                                 self._y_train)
            else:
                view = kept_columns.mlp_view(self._ssm, cols, n_s)
            self._view, self._view_of = view, inner_model
        return self._view

    @property
    def folded_columns(self) -> Optional[Tuple[int, ...]]:
        """The padded input columns the inner model sees (None: the inner model is the padded one, as in the reference)."""
        return None if self._cols is None else tuple(int(c) for c in self._cols)

    def _query(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor]:
        es = self._expand(states, self.num_states, self._junk_states)
        ea = self._expand(actions, self.num_actions, self._junk_actions)
        if self._cols is None:
            return es, ea
        z = torch.cat((es, ea), dim=1)[:, self._cols.to(es.device)]
        return z[:, :self.num_states], z[:, self.num_states:]

    def predict_with_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        means, variances, jacs = self._ssm.predict_with_jacobians(*self._query(states, actions))
        return (means[:, :self.num_states], variances[:, :self.num_states],
                jacs[:, :self.num_states, :(self.num_states + self.num_actions)])

    def predict_without_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor]:
        means, variances = self._ssm.predict_without_jacobians(*self._query(states, actions))
        return means[:, :self.num_states], variances[:, :self.num_states]

    def predict_raw(self, z: Tensor) -> Tuple[Tensor, Tensor]:
        ez = self._expand(z, self.num_states + self.num_actions, self._junk_states + self._junk_actions)
        if self._cols is not None:
            ez = ez[:, self._cols.to(ez.device)]
        means, variances = self._ssm.predict_raw(ez)
        return means[:, :self.num_states], variances[:, :self.num_states]

    def update_model(self, train_x: Tensor, train_y: Tensor, opt_hyp=False, replace_old=False) -> None:
        super().update_model(train_x, train_y, opt_hyp, replace_old)
        ex = self._expand(train_x, self.num_states + self.num_actions, self._junk_states + self._junk_actions)
        if self._cols is not None:
            self._ssm.update_model(ex[:, self._cols.to(ex.device)], train_y, opt_hyp, replace_old)
            return
        self._ssm.update_model(ex, self._expand(train_y, self.num_states, self._junk_states), opt_hyp, replace_old)

    @staticmethod
    def _expand(x: Tensor, real_dimen: int, junk_dimen: int) -> Tensor:
        n = x.size(0)
        assert_shape(x, (n, real_dimen))
        expanded = torch.zeros((n, real_dimen + junk_dimen), device=x.device, dtype=x.dtype)
        expanded[:, :real_dimen] = x
        return expanded

    def _update_model(self, x_train: Tensor, y_train: Tensor) -> None:
        pass

    def _train_model(self, x_train: Tensor, y_train: Tensor) -> None:
        pass

    def collect_metrics(self) -> Dict[str, Any]:
        return self._ssm.collect_metrics()

    @property
    def parametric(self) -> bool:
        return self._ssm.parametric
