"""Exact-GP state-space model for the CEM safe-MPC solver, predicted by the HIP kernels of libsxamd.

Same surface as the reference's ``GpCemSSM`` (``safe_exploration/ssm_cem/gp_ssm_cem.py:17-137``): ``n_s`` independent
exact GPs on shared inputs, zero mean, scaled ARD-RBF kernel, Gaussian likelihood whose noise is INCLUDED in the
predictive variance.  The reference delegates the arithmetic to gpytorch 0.3.2; here

* ``_update_model`` factorises ``K_d + noise_d I = L_d L_d^T`` and lays ``W_d = L_d^-1`` and ``alpha_d`` out for the
  f64 matrix cores (``sx_gp_pack``) -- this is the warm path, run once per ``update_model``;
* every ``predict_*`` is one ``sx_gp_predict`` launch (mean, variance and the analytic mean-Jacobian in one pass,
  where the reference needs two forward passes and a backward pass, ``gp_ssm_cem.py:59-73``).

Hyper-parameters follow gpytorch's parameterisation (softplus of a raw parameter that starts at 0; the noise has a
1e-4 floor).  gpytorch is not available to check these defaults against: "parity unpinned" (DESIGN.md).
"""
import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from .. import _lib
from ..utils import assert_shape, get_device
from .ssm_cem import CemSSM

_NOISE_FLOOR = 1e-4


# csrc/sx_fit.hpp kFitMaxN: the factorisation's last stage keeps one column of the system in LDS
MAX_TRAINING_POINTS = 4096


class GpCemSSM(CemSSM):
    kernel_family = 'rbf'   # 'feature' for the degenerate kernels ('linear', 'nn'): feature_gp_ssm_cem.FeatureGpCemSSM

    def __new__(cls, conf=None, *args, **kwargs):
        # one class name for every kernel, as in the reference (gp_ssm_cem.py:45-57): the 'linear' and 'nn' kernels are
        # served by the weight-space subclass
        if cls is GpCemSSM and getattr(conf, 'exact_gp_kernel', 'rbf') in ('linear', 'nn'):
            from .feature_gp_ssm_cem import FeatureGpCemSSM
            return super().__new__(FeatureGpCemSSM)
        return super().__new__(cls)

    def __init__(self, conf, state_dimen: int, action_dimen: int, model=None, *, wide_inputs: bool = False):
        """wide_inputs: the GP of JunkDimensionsSSM's fused rollout (sx_cem_rollout_junk), whose "action" inputs are the
        real actions plus the junk columns that queries fill: up to SX_MAX_D inputs in all, any split.  Such a model is fit
        and packed for the rollout kernel only; sx_gp_predict is not instantiated beyond SX_MAX_NU actions."""
        super().__init__(state_dimen, action_dimen)
        if model is not None:
            raise NotImplementedError('injecting a gpytorch model is not supported: the GP is evaluated by libsxamd')
        kernel = getattr(conf, 'exact_gp_kernel', 'rbf')
        if kernel != 'rbf':
            raise ValueError(f'Unknown kernel {kernel}')
        too_wide = (state_dimen + action_dimen > _lib.SX_MAX_D) if wide_inputs else (action_dimen > _lib.SX_MAX_NU)
        if state_dimen > _lib.SX_MAX_NS or too_wide:
            raise ValueError(f'state/action dimension ({state_dimen}, {action_dimen}) beyond the compiled limits')
        self._device = torch.device(get_device(conf))
        self._training_iterations = int(getattr(conf, 'exact_gp_training_iterations', 0))
        d_in = state_dimen + action_dimen
        self._raw_lengthscale = torch.zeros((state_dimen, d_in), dtype=torch.float64)
        self._raw_outputscale = torch.zeros((state_dimen,), dtype=torch.float64)
        self._raw_noise = torch.zeros((state_dimen,), dtype=torch.float64)
        self._noise_floor = _NOISE_FLOOR
        self._last_training_losses = []
        self._model: Optional[_lib.SxGpModel] = None
        self._buffers = ()  # keeps the device operands alive while the struct points at them
        self._workspace: Optional[Tensor] = None
        self._fit_ws = None
        self._linv_current = False   # does _fit_ws[1] hold W of the CURRENT model?

    # ---- hyper-parameters --------------------------------------------------------------------------------------
    @property
    def lengthscale(self) -> Tensor:
        return F.softplus(self._raw_lengthscale)

    @property
    def outputscale(self) -> Tensor:
        return F.softplus(self._raw_outputscale)

    @property
    def noise(self) -> Tensor:
        return F.softplus(self._raw_noise) + self._noise_floor

    @staticmethod
    def _inv_softplus(x: Tensor) -> Tensor:
        return x + torch.log(-torch.expm1(-x))

    def set_hyperparameters(self, lengthscale=None, outputscale=None, noise=None) -> None:
        """Explicit hyper-parameters: lengthscale [n_s x D] (or broadcastable), outputscale [n_s], noise [n_s]."""
        n_s, d_in = self.num_states, self.num_states + self.num_actions
        if lengthscale is not None:
            ls = torch.as_tensor(lengthscale, dtype=torch.float64).cpu().expand(n_s, d_in).clone()
            self._raw_lengthscale = self._inv_softplus(ls)
        if outputscale is not None:
            s = torch.as_tensor(outputscale, dtype=torch.float64).cpu().expand(n_s).clone()
            self._raw_outputscale = self._inv_softplus(s)
        if noise is not None:
            nz = torch.as_tensor(noise, dtype=torch.float64).cpu().expand(n_s).clone()
            if (nz <= 0).any():
                raise ValueError('noise must be positive')
            if (nz <= self._noise_floor).any():
                self._noise_floor = 0.0   # explicit values below gpytorch's default floor: drop the floor
            self._raw_noise = self._inv_softplus(nz - self._noise_floor)
        if self._x_train is not None:
            self._update_model(self._x_train, self._y_train)

    def state_dict(self) -> Dict[str, Dict[str, Tensor]]:
        """The hyper-parameter state, split the way the reference's failure dump stores it (model / likelihood:
        gp_reachability_pytorch.py:256-266); `load_state_dict` takes it back."""
        return {'gp_model': {'raw_lengthscale': self._raw_lengthscale.clone(), 'raw_outputscale': self._raw_outputscale.clone()},
                'gp_likelihood': {'raw_noise': self._raw_noise.clone(), 'noise_floor': torch.tensor(self._noise_floor)}}

    def load_state_dict(self, state: Dict[str, Dict[str, Tensor]]) -> None:
        self._raw_lengthscale = state['gp_model']['raw_lengthscale'].clone()
        self._raw_outputscale = state['gp_model']['raw_outputscale'].clone()
        self._raw_noise = state['gp_likelihood']['raw_noise'].clone()
        self._noise_floor = float(state['gp_likelihood']['noise_floor'])
        if self._x_train is not None:
            self._update_model(self._x_train, self._y_train)

    # ---- model (re)build: the warm path ------------------------------------------------------------------------
    def _fit_struct(self, x: Tensor, raw: Optional[Tuple[Tensor, Tensor, Tensor]] = None) -> _lib.SxGpModel:
        """The sx_gp_model sx_gp_fit takes: training inputs x (device, contiguous) and the hyper-parameters of the raw
        parameters `raw` = (lengthscale, outputscale, noise), the model's own by default."""
        raw_ls, raw_os, raw_noise = raw if raw is not None else (self._raw_lengthscale, self._raw_outputscale,
                                                                 self._raw_noise)
        m = _lib.SxGpModel()
        m.n_s, m.n_u, m.n_train = self.num_states, self.num_actions, x.size(0)
        _lib.fill(m.inv_ls2, (1.0 / F.softplus(raw_ls) ** 2).numpy())
        _lib.fill(m.outputscale, F.softplus(raw_os).numpy())
        _lib.fill(m.noise, (F.softplus(raw_noise) + self._noise_floor).numpy())
        m.x_train = x.data_ptr()
        return m

    def _fit_workspace(self, n: int, dev) -> Tuple[Tensor, Tensor]:
        """(work, linv) of sx_gp_fit for N = n, reused across fits of one size."""
        if self._fit_ws is None or self._fit_ws[0].size(1) != n or self._fit_ws[0].device != dev:
            self._fit_ws = (torch.empty((self.num_states, n, n), dtype=torch.float64, device=dev),
                            torch.empty((self.num_states, n, n), dtype=torch.float64, device=dev))
        self._linv_current = False   # (set again by _update_model, whose fit is the model's)
        return self._fit_ws

    def _fit(self, x: Tensor, y: Tensor):
        """sx_gp_fit for the current hyper-parameters.  Returns (model struct, linv, alpha, logdet); raises if the
        kernel matrix is not positive definite."""
        lib = _lib.lib()
        dev = x.device
        n_s, n = self.num_states, x.size(0)
        m = self._fit_struct(x)
        work, linv = self._fit_workspace(n, dev)
        alpha = torch.empty((n_s, n), dtype=torch.float64, device=dev)
        logdet = torch.empty((n_s,), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.sx_gp_fit(ctypes.byref(m), _lib.ptr(y), _lib.ptr(work), _lib.ptr(linv), _lib.ptr(alpha),
                                 _lib.ptr(logdet), _lib.ptr(status), _lib.stream_ptr(dev)), 'sx_gp_fit')
        return m, linv, alpha, logdet, status

    def _update_model(self, x_train: Tensor, y_train: Tensor) -> None:
        n = x_train.size(0)
        if n > MAX_TRAINING_POINTS:
            raise ValueError(f'{n} training points: the exact-GP kernels hold up to {MAX_TRAINING_POINTS} (sx_gp_fit); keep the '
                             f'most recent / most informative ones (update_model(..., replace_old=True))')
        _lib.require_gpu(x_train, 'train_x')
        _lib.require_gpu(y_train, 'train_y')
        x = x_train.detach().contiguous()
        y = y_train.detach().contiguous()
        # factorise on the device (sx_gp_fit), then lay the operands out for the matrix cores (sx_gp_pack)
        m, linv, alpha, logdet, status = self._fit(x, y)
        packed = self._pack(m, linv, alpha)
        if int(status.item()) & _lib.SX_STATUS_NOT_PD:
            raise RuntimeError('the kernel matrix K + noise I is not positive definite for the current hyper-parameters')
        self._install(x, m, packed, alpha, logdet.cpu())

    def _pack(self, m: _lib.SxGpModel, linv: Tensor, alpha: Tensor) -> Tuple[Tensor, Tensor]:
        """sx_gp_pack of a fitted model into new buffers: (a_pack, stage_tab), which `m` then points at."""
        lib = _lib.lib()
        dev = linv.device
        a_n, t_n = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(lib.sx_gp_pack_sizes(m.n_s, m.n_u, m.n_train, ctypes.byref(a_n), ctypes.byref(t_n)), 'sx_gp_pack_sizes')
        a_pack = torch.empty(a_n.value, dtype=torch.float64, device=dev)
        stage_tab = torch.empty(t_n.value, dtype=torch.int32, device=dev)
        m.a_pack, m.stage_tab = a_pack.data_ptr(), stage_tab.data_ptr()
        _lib.check(lib.sx_gp_pack(ctypes.byref(m), _lib.ptr(linv), _lib.ptr(alpha), _lib.stream_ptr(dev)), 'sx_gp_pack')
        return a_pack, stage_tab

    def _install(self, x: Tensor, m: _lib.SxGpModel, packed: Tuple[Tensor, Tensor], alpha: Tensor, logdet: Tensor) -> None:
        """Makes the packed fit of x the model's (logdet: host [n_s]); the fit workspace holds its W."""
        self._model = m
        self._buffers = (x,) + tuple(packed)
        self._alpha = alpha
        self._linv_current = True
        # 1/2 log det(I + K_d / noise_d) = sum log diag L_d - N/2 log noise_d
        self._info_gain = (logdet - 0.5 * x.size(0) * torch.log(self.noise)).numpy()

    def mll_and_grad(self, x_train: Tensor, y_train: Tensor):
        """Exact marginal log likelihood per output [n_s] and its gradient [n_s x (D + 2)] w.r.t.
        (lengthscale, outputscale, noise), at the current hyper-parameters (host tensors)."""
        x, y = x_train.detach().contiguous(), y_train.detach().contiguous()
        m, linv, alpha, logdet, status = self._fit(x, y)
        d_in = self.num_states + self.num_actions
        mll = torch.empty((self.num_states,), dtype=torch.float64, device=x.device)
        grad = torch.empty((self.num_states, d_in + 2), dtype=torch.float64, device=x.device)
        _lib.check(_lib.lib().sx_gp_mll_grad(ctypes.byref(m), _lib.ptr(y), _lib.ptr(linv), _lib.ptr(alpha), _lib.ptr(logdet),
                                             _lib.ptr(self._fit_ws[0]), _lib.ptr(mll), _lib.ptr(grad),
                                             _lib.stream_ptr(x.device)), 'sx_gp_mll_grad')
        host = torch.cat((mll, grad.reshape(-1), status.double())).cpu()
        if int(host[-1]) & _lib.SX_STATUS_NOT_PD:
            raise RuntimeError('the kernel matrix K + noise I is not positive definite for the current hyper-parameters')
        return host[:self.num_states], host[self.num_states:-1].reshape(self.num_states, d_in + 2)

    def information_gain(self):
        """[n_s] information gain of the training inputs, per output (zeros without data)."""
        import numpy as np
        return np.zeros(self.num_states) if self._model is None else self._info_gain.copy()

    def workspace(self, nbytes: int) -> Optional[Tensor]:
        """Scratch for the large-training-set rollout path (grown on demand, reused across calls)."""
        if nbytes <= 0:
            return None
        if self._workspace is None or self._workspace.numel() * 8 < nbytes:
            self._workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self._buffers[0].device)
        return self._workspace

    @property
    def device_model(self) -> _lib.SxGpModel:
        """The sx_gp_model the fused solver hands to sx_cem_rollout."""
        if self._model is None:
            raise RuntimeError('the GP has no training data yet: call update_model first')
        return self._model

    def _train_model(self, x_train: Tensor, y_train: Tensor) -> None:
        """Adam (lr 0.01) on the exact marginal log likelihood, the reference's recipe (gp_ssm_cem.py:103-129): the
        loss is -sum_d mll_d / N (gpytorch's ExactMarginalLogLikelihood divides by the number of data points).
        Value and gradient come from the device (sx_gp_fit + sx_gp_mll_grad); the few-parameter Adam step and the
        softplus chain rule stay on the host."""
        if self._training_iterations <= 0:
            return
        n = x_train.size(0)
        d_in = self.num_states + self.num_actions
        raw = [self._raw_lengthscale.clone().requires_grad_(True), self._raw_outputscale.clone().requires_grad_(True),
               self._raw_noise.clone().requires_grad_(True)]
        opt = torch.optim.Adam(raw, lr=0.01)
        losses = []
        for _ in range(self._training_iterations):
            self._raw_lengthscale, self._raw_outputscale, self._raw_noise = (t.detach() for t in raw)
            mll, grad = self.mll_and_grad(x_train, y_train)
            losses.append(float(-(mll / n).sum()))
            # d loss / d raw = -(1/N) d mll / d theta * sigmoid(raw)   (theta = softplus(raw) [+ floor])
            raw[0].grad = -(grad[:, :d_in] / n) * torch.sigmoid(raw[0].detach())
            raw[1].grad = -(grad[:, d_in] / n) * torch.sigmoid(raw[1].detach())
            raw[2].grad = -(grad[:, d_in + 1] / n) * torch.sigmoid(raw[2].detach())
            opt.step()
        self._raw_lengthscale, self._raw_outputscale, self._raw_noise = (t.detach().clone() for t in raw)
        self._last_training_losses = losses
        self._update_model(x_train, y_train)

    # ---- prediction: the hot path ------------------------------------------------------------------------------
    def _predict_z(self, z: Tensor, jacobians: bool) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
        n = z.size(0)
        d_in = self.num_states + self.num_actions
        assert_shape(z, (n, d_in))
        _lib.require_gpu(z, 'states/actions')
        z = z.detach().contiguous()
        mean = torch.empty((n, self.num_states), dtype=torch.float64, device=z.device)
        var = torch.empty_like(mean)
        jac = torch.empty((n, self.num_states, d_in), dtype=torch.float64, device=z.device) if jacobians else None
        if n == 0:
            return mean, var, jac
        if self._model is None:
            # no data: the prior (zero mean, s + noise variance, flat mean)
            mean.zero_()
            var.copy_((self.outputscale + self.noise).to(z.device).expand(n, -1))
            if jac is not None:
                jac.zero_()
            return mean, var, jac
        lib = _lib.lib()
        ws_bytes = int(lib.sx_gp_predict_workspace_bytes(ctypes.byref(self._model), n))
        _lib.check(lib.sx_gp_predict(ctypes.byref(self._model), _lib.ptr(z), n, _lib.ptr(mean), _lib.ptr(var),
                                     _lib.ptr(jac), _lib.ptr(self.workspace(ws_bytes)), ws_bytes,
                                     _lib.stream_ptr(z.device)), 'sx_gp_predict')
        return mean, var, jac

    def predict_with_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        return self._predict_z(self._join_states_actions(states, actions), True)

    def predict_without_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor]:
        mean, var, _ = self._predict_z(self._join_states_actions(states, actions), False)
        return mean, var

    def predict_variance_jacobian(self, states: Tensor, actions: Tensor) -> Tensor:
        """d var / d (state, action)  [N x n_s x (n_s + n_u)].  Not used by the CEM solver; the numpy adapter
        (state_space_models.HipGpStateSpaceModel) returns it where the reference's GPyTorchSSM returns
        ``compute_jacobian(pred_var, inp)`` (ssm_pytorch/gaussian_process.py:222-231)."""
        z = self._join_states_actions(states, actions)
        n, d_in = z.size(0), self.num_states + self.num_actions
        _lib.require_gpu(z, 'states/actions')
        z = z.detach().contiguous()
        out = torch.zeros((n, self.num_states, d_in), dtype=torch.float64, device=z.device)
        if n == 0 or self._model is None:   # the prior variance does not depend on z
            return out
        if not self._linv_current:
            # the fit workspace was reused since (hyper-parameter training): factorise once more
            self._fit(self._x_train.detach().contiguous(), self._y_train.detach().contiguous())
            self._linv_current = True
        _lib.check(_lib.lib().sx_gp_predict_var_jac(ctypes.byref(self._model), _lib.ptr(self._fit_ws[1]), _lib.ptr(z), n,
                                                   _lib.ptr(out), _lib.stream_ptr(z.device)), 'sx_gp_predict_var_jac')
        return out

    def predict_mean_hessian(self, states: Tensor, actions: Tensor) -> Tensor:
        """d^2 mean / d(state, action)^2  [N x n_s x (n_s + n_u) x (n_s + n_u)] (closed form, sx_gp_predict_mean_hessian).
        Not used by the CEM solver; the numpy adapter's linearize_predict returns it where the reference's GPyTorchSSM
        calls the `hessian` package (ssm_pytorch/gaussian_process.py:160-187)."""
        z = self._join_states_actions(states, actions)
        n, d_in = z.size(0), self.num_states + self.num_actions
        _lib.require_gpu(z, 'states/actions')
        z = z.detach().contiguous()
        out = torch.zeros((n, self.num_states, d_in, d_in), dtype=torch.float64, device=z.device)
        if n == 0 or self._model is None:   # the prior mean is flat
            return out
        _lib.check(_lib.lib().sx_gp_predict_mean_hessian(ctypes.byref(self._model), _lib.ptr(self._alpha), _lib.ptr(z), n,
                                                        _lib.ptr(out), _lib.stream_ptr(z.device)), 'sx_gp_predict_mean_hessian')
        return out

    def predict_raw(self, z: Tensor) -> Tuple[Tensor, Tensor]:
        mean, var, _ = self._predict_z(z, False)
        return mean.t(), var.t()

    def collect_metrics(self) -> Dict[str, Any]:
        return {'losses': self._last_training_losses}

    @property
    def parametric(self) -> bool:
        return False


# ---- E exact GPs trained in lockstep: the reference's n_scenarios models (episode_runner.py:55,123) -----------------------
def _multi_fit_applies(ssms: Sequence[CemSSM], xs: Sequence[Tensor]) -> bool:
    """Do these models train together (update_models_multi)?  Exact RBF GPs of one (n_s, n_u) and one training-iteration
    count, with their data on one device."""
    first = ssms[0]
    return (all(isinstance(m, GpCemSSM) and m.kernel_family == 'rbf' for m in ssms)
            and all((m.num_states, m.num_actions, m._training_iterations)
                    == (first.num_states, first.num_actions, first._training_iterations) for m in ssms)
            and all(x.device == xs[0].device for x in xs)
            and len({id(m) for m in ssms}) == len(ssms))


class _MultiFit:
    """The device side of a multi-model fit: problem e's fit buffers (its model's fit workspace, alpha, logdet), the
    stacked outputs (status [E], mll [E x n_s], grad [E x n_s x (D + 2)]) and the problem table, written by
    sx_gp_fit_table into pinned host memory and copied to the device on the stream without a wait."""

    def __init__(self, ssms: List['GpCemSSM'], xs: List[Tensor], ys: List[Tensor]):
        lib = _lib.lib()
        dev = xs[0].device
        self.ssms, self.xs, self.ys, self.E = ssms, xs, ys, len(ssms)
        n_s, d_in = ssms[0].num_states, ssms[0].num_states + ssms[0].num_actions
        self.ws = [m._fit_workspace(x.size(0), dev) for m, x in zip(ssms, xs)]
        self.alpha = [torch.empty((n_s, x.size(0)), dtype=torch.float64, device=dev) for x in xs]
        self.logdet = torch.empty((self.E, n_s), dtype=torch.float64, device=dev)
        self.status = torch.zeros(self.E, dtype=torch.int32, device=dev)
        self.mll = torch.empty((self.E, n_s), dtype=torch.float64, device=dev)
        self.grad = torch.empty((self.E, n_s, d_in + 2), dtype=torch.float64, device=dev)
        nbytes = int(lib.sx_gp_fit_table_bytes(self.E))
        self.host_table = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.stream = _lib.stream_ptr(dev)

    def new_alpha(self) -> None:
        """Fresh alpha buffers: the final fit's become the models' own."""
        self.alpha = [torch.empty_like(a) for a in self.alpha]

    def launch(self, raws: List[Tuple[Tensor, Tensor, Tensor]], mll: bool):
        """sx_gp_fit_multi (and sx_gp_mll_grad_multi) at the raw hyper-parameters raws[e]; returns the E model structs."""
        lib = _lib.lib()
        E = self.E
        models = (_lib.SxGpModel * E)(*[m._fit_struct(x, raw) for m, x, raw in zip(self.ssms, self.xs, raws)])
        arr = lambda ts: (ctypes.c_void_p * E)(*[t.data_ptr() for t in ts])
        _lib.check(lib.sx_gp_fit_table(models, E, arr(self.ys), arr([w[0] for w in self.ws]), arr([w[1] for w in self.ws]),
                                       arr(self.alpha), arr(list(self.logdet)), _lib.ptr(self.status), _lib.ptr(self.mll),
                                       _lib.ptr(self.grad), ctypes.c_void_p(self.host_table.data_ptr())), 'sx_gp_fit_table')
        # (the previous step's copy has completed: every step ends in a host read of its results)
        self.table.copy_(self.host_table, non_blocking=True)
        self.status.zero_()
        _lib.check(lib.sx_gp_fit_multi(models, E, _lib.ptr(self.table), self.stream), 'sx_gp_fit_multi')
        if mll:
            _lib.check(lib.sx_gp_mll_grad_multi(models, E, _lib.ptr(self.table), self.stream), 'sx_gp_mll_grad_multi')
        return models

    def check_status(self, status: Tensor) -> None:
        """Raises for the first problem whose kernel matrix is not positive definite (status: host [E])."""
        for e in range(self.E):
            if int(status[e]) & _lib.SX_STATUS_NOT_PD:
                raise RuntimeError(f'problem {e}: the kernel matrix K + noise I is not positive definite for the current '
                                   f'hyper-parameters')


def update_models_multi(ssms: Sequence[CemSSM], xs: Sequence[Tensor], ys: Sequence[Tensor], opt_hyp=False,
                        replace_old=False) -> None:
    """``m.update_model(x, y, opt_hyp, replace_old)`` for every (m, x, y) at once: the reference's n_scenarios models, each
    retrained on its own data after every episode (episode_runner.py:55,123).

    Exact RBF GPs of one (n_s, n_u) and one iteration count train in lockstep: per Adam step ONE sx_gp_fit_multi and ONE
    sx_gp_mll_grad_multi launch sequence for all of them and one host read, then one batched fit and an sx_gp_pack per
    model.  Adam is the recipe of GpCemSSM._train_model, one optimizer over every model's raw parameters; its update is
    elementwise, and each model keeps its own parameter tensors, so each follows the trajectory it would follow alone:
    the hyper-parameters, loss curves (``_last_training_losses``) and predictions equal those of per-model
    ``update_model`` bit for bit.  A kernel matrix that is not positive definite in problem e raises RuntimeError naming
    e, and then no model's data, hyper-parameters or predictions have changed.  (Each model's fit workspace serves the
    batch from the start, so after such a call its cached W = L^-1 is marked stale, and its next
    predict_variance_jacobian factorises once more -- as after a failed single-model update.)  Any other list of models (other families,
    JunkDimensionsSSM, differing shapes or iteration counts) is updated one model at a time."""
    ssms, xs, ys = list(ssms), list(xs), list(ys)
    if not len(ssms) == len(xs) == len(ys):
        raise ValueError(f'{len(ssms)} models, {len(xs)} input sets, {len(ys)} target sets')
    if not ssms:
        return
    if not _multi_fit_applies(ssms, xs):
        for m, x, y in zip(ssms, xs, ys):
            m.update_model(x, y, opt_hyp, replace_old)
        return
    # the merged training sets, checked before anything changes
    merged = []
    for m, x, y in zip(ssms, xs, ys):
        n = x.size(0)
        assert_shape(x, (n, m.num_states + m.num_actions))
        assert_shape(y, (n, m.num_states))
        if not replace_old and m._x_train is not None and m._y_train is not None:
            x, y = torch.cat((m._x_train, x), dim=0), torch.cat((m._y_train, y), dim=0)
        if x.size(0) > MAX_TRAINING_POINTS:
            raise ValueError(f'{x.size(0)} training points: the exact-GP kernels hold up to {MAX_TRAINING_POINTS}')
        _lib.require_gpu(x, 'train_x')
        _lib.require_gpu(y, 'train_y')
        merged.append((x, y))
    fit = _MultiFit(ssms, [x.detach().contiguous() for x, _ in merged], [y.detach().contiguous() for _, y in merged])
    E, n_s, d_in = len(ssms), ssms[0].num_states, ssms[0].num_states + ssms[0].num_actions
    raws = [(m._raw_lengthscale, m._raw_outputscale, m._raw_noise) for m in ssms]
    losses: Optional[List[List[float]]] = None
    iterations = ssms[0]._training_iterations
    if (opt_hyp or ssms[0].parametric) and iterations > 0:
        params = [[t.clone().requires_grad_(True) for t in raw] for raw in raws]
        opt = torch.optim.Adam([t for p in params for t in p], lr=0.01)
        losses = [[] for _ in ssms]
        for _ in range(iterations):
            step = [tuple(t.detach() for t in p) for p in params]
            fit.launch(step, mll=True)
            host = torch.cat((fit.mll.reshape(-1), fit.grad.reshape(-1), fit.status.double())).cpu()   # the step's one sync
            fit.check_status(host[-E:])
            grads = host[E * n_s:-E].reshape(E, n_s, d_in + 2)
            for e, (x, p) in enumerate(zip(fit.xs, params)):
                n = x.size(0)
                mll, grad = host[e * n_s:(e + 1) * n_s].clone(), grads[e]
                losses[e].append(float(-(mll / n).sum()))
                # d loss / d raw = -(1/N) d mll / d theta * sigmoid(raw), as GpCemSSM._train_model
                p[0].grad = -(grad[:, :d_in] / n) * torch.sigmoid(p[0].detach())
                p[1].grad = -(grad[:, d_in] / n) * torch.sigmoid(p[1].detach())
                p[2].grad = -(grad[:, d_in + 1] / n) * torch.sigmoid(p[2].detach())
            opt.step()
        raws = [tuple(t.detach().clone() for t in p) for p in params]
    # the final fit at the trained hyper-parameters; nothing is committed before it has succeeded everywhere
    fit.new_alpha()
    models = fit.launch(raws, mll=False)
    host = torch.cat((fit.status.double(), fit.logdet.reshape(-1))).cpu()
    fit.check_status(host[:E])
    logdets = host[E:].reshape(E, n_s)
    for e, m in enumerate(ssms):
        m._x_train, m._y_train = merged[e]
        m._raw_lengthscale, m._raw_outputscale, m._raw_noise = raws[e]
        if losses is not None:
            m._last_training_losses = losses[e]
        model = _lib.SxGpModel.from_buffer_copy(models[e])
        packed = m._pack(model, fit.ws[e][1], fit.alpha[e])
        m._install(fit.xs[e], model, packed, fit.alpha[e], logdets[e].clone())
