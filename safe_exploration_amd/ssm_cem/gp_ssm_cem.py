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
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from .. import _lib
from ..utils import assert_shape, get_device
from .ssm_cem import CemSSM

_NOISE_FLOOR = 1e-4


# csrc/sx_fit.hpp kFitMaxN: the factorisation's last stage keeps one column of the system in LDS
MAX_TRAINING_POINTS = 4096
# csrc/sx_gp_select.hpp kSelMaxN: the pool a max-variance subset is chosen from (conf.cem_gp_subset_size)
MAX_POOL_POINTS = 65536
# csrc/sx_gp_append.hpp kAppendMaxK: the rows one sx_gp_append call adds (conf.cem_gp_incremental)
MAX_APPEND_ROWS = 64
# csrc/sx_gp_drop.hpp kDropMaxK: the rows one sx_gp_drop call removes (conf.cem_gp_window)
MAX_DROP_ROWS = 64
# the rows a windowed model drops in one slide: the largest measured overflow at which drop + append beats the full fit of the
# window at every window size measured (200, 590, 2000).  Beyond it the update fits in full.
MAX_SLIDE_ROWS = 16
# conf.cem_gp_window_max_chain's default: the rows a windowed model appends and slides between two full fits.  The longest
# chain measured on the device, at which W and alpha still stay within the fit's own error allowance
WINDOW_MAX_CHAIN = 128


# ---- what the single-model and the lockstep calls share -------------------------------------------------------------------------
def _workspace_bytes(query, *args) -> int:
    """`query(*args)`, the size query of a library entry (`lib.sx_..._workspace_bytes`); a negative answer is a bad argument."""
    nbytes = int(query(*args))
    if nbytes < 0:
        raise _lib.SxError(f'{getattr(query, "__name__", "workspace_bytes")}: bad argument')
    return nbytes


def _grown(ws: Optional[Tensor], nbytes: int, dev, slack: int = 0) -> Tensor:
    """A workspace of at least nbytes on dev: `ws` where it is one already, else a new one with `slack` bytes to spare."""
    if ws is None or ws.numel() * 8 < nbytes or ws.device != dev:
        ws = torch.empty((nbytes + slack + 7) // 8, dtype=torch.float64, device=dev)
    return ws


def _ptr_array(ts: Sequence[Tensor]):
    """the tensors' device addresses as the void* array the table entries take"""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _outputs(n_s: int, ns: Sequence[int], dev, status: Optional[Tensor] = None):
    """Fresh output buffers of a factor update of E = len(ns) problems, problem e with ns[e] rows: (linv [E] of [n_s x n x n],
    alpha [E] of [n_s x n], logdet [E n_s] (problem e's n_s values at e n_s), status [E], zeroed).  status: the words of the
    call before, which this one shares so that one read decides for both (a slide's drop and append)."""
    linv = [torch.empty((n_s, n, n), dtype=torch.float64, device=dev) for n in ns]
    alpha = [torch.empty((n_s, n), dtype=torch.float64, device=dev) for n in ns]
    logdet = torch.empty(len(ns) * n_s, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(len(ns), dtype=torch.int32, device=dev)
    return linv, alpha, logdet, status


def _adam_grads(raw: Sequence[Tensor], grad: Tensor, n: int) -> None:
    """Sets the gradients of the loss -sum_d mll_d / n on the raw parameters `raw` = (lengthscale, outputscale, noise) from
    grad [n_s x (D + 2)] = d mll / d (lengthscale, outputscale, noise): d loss / d raw = -(1/n) d mll / d theta * sigmoid(raw)
    (theta = softplus(raw) [+ floor])."""
    d_in = grad.size(1) - 2
    raw[0].grad = -(grad[:, :d_in] / n) * torch.sigmoid(raw[0].detach())
    raw[1].grad = -(grad[:, d_in] / n) * torch.sigmoid(raw[1].detach())
    raw[2].grad = -(grad[:, d_in + 1] / n) * torch.sigmoid(raw[2].detach())


class GpCemSSM(CemSSM):
    kernel_family = 'rbf'   # 'feature' for the degenerate kernels ('linear', 'nn'): feature_gp_ssm_cem.FeatureGpCemSSM
    _subset_size: Optional[int] = None     # conf.cem_gp_subset_size (set by __init__; the weight-space subclass has none)
    _subset_idx: Optional[Tensor] = None
    _incremental = False                   # conf.cem_gp_incremental (set by __init__; the weight-space subclass has none)
    _append_ok = False
    _lockstep = False                      # conf.cem_gp_incremental_lockstep (set by __init__; the weight-space subclass has none)
    _window: Optional[int] = None          # conf.cem_gp_window (set by __init__; the weight-space subclass has none)

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
        # conf.cem_gp_subset_size: fit at most that many of the stored points, the max-variance subset (sx_gp_select); None:
        # fit them all.  A setting of its own: conf.m, which CEM configs inherit from the defaults, stays unread.
        subset = getattr(conf, 'cem_gp_subset_size', None)
        self._subset_size: Optional[int] = None if subset is None else int(subset)
        if self._subset_size is not None and not 1 <= self._subset_size <= MAX_TRAINING_POINTS:
            raise ValueError(f'cem_gp_subset_size={subset}: the fitted subset holds 1 .. {MAX_TRAINING_POINTS} points')
        self._subset_idx: Optional[Tensor] = None   # rows of the stored pool the device model is fitted on (None: all)
        # conf.cem_gp_incremental: an update whose data extend the fitted rows by 1 .. 64 under unchanged hyper-parameters
        # appends to the factorisation (sx_gp_append, O(N^2 k)) instead of refitting (O(N^3)); off: every update is a full fit.
        # conf.cem_gp_incremental_max_chain: at most that many rows are appended between two full fits (None: no limit --
        # 64 single-row appends stay within the fit's own error allowance).
        self._incremental = bool(getattr(conf, 'cem_gp_incremental', False))
        chain = getattr(conf, 'cem_gp_incremental_max_chain', None)
        self._max_chain: Optional[int] = None if chain is None else int(chain)
        if self._max_chain is not None and self._max_chain < 0:
            raise ValueError(f'cem_gp_incremental_max_chain={chain}: a row count, or None')
        # conf.cem_gp_incremental_lockstep: update_models_multi appends to the models that have it, qualify and share the
        # number of new rows in ONE sx_gp_append_multi call (`_increment_group`); off: model by model.  With conf.cem_gp_window
        # the models that overflow their windows by the same number of rows slide in ONE sx_gp_drop_multi and ONE
        # sx_gp_append_multi call
        self._lockstep = bool(getattr(conf, 'cem_gp_incremental_lockstep', False))
        if self._lockstep and not self._incremental:
            raise ValueError('cem_gp_incremental_lockstep needs cem_gp_incremental: there is nothing to append in lockstep '
                             'where every update is a full fit')
        # conf.cem_gp_window = m: the model keeps the most recent m rows.  Every update trims the stored data to them, and a
        # plain update that overflows the window by r rows slides it: sx_gp_drop of the r oldest rows, then sx_gp_append of the
        # new ones, O(N^2 (r + k)), instead of the full fit of the last m rows.  conf.cem_gp_window_max_chain: at most that many
        # rows are appended or slid between two full fits of a windowed model (None: no limit).
        window = getattr(conf, 'cem_gp_window', None)
        self._window: Optional[int] = None if window is None else int(window)
        if self._window is not None:
            if not 1 <= self._window <= MAX_TRAINING_POINTS:
                raise ValueError(f'cem_gp_window={window}: the window holds 1 .. {MAX_TRAINING_POINTS} rows')
            if not self._incremental:
                raise ValueError('cem_gp_window needs cem_gp_incremental: without it every update is a full fit, and there '
                                 'is nothing to slide')
            if self._subset_size is not None:
                raise ValueError('cem_gp_window excludes cem_gp_subset_size: the fitted rows are either the most recent or '
                                 'the max-variance subset')
        wchain = getattr(conf, 'cem_gp_window_max_chain', WINDOW_MAX_CHAIN)
        self._window_max_chain: Optional[int] = None if wchain is None else int(wchain)
        if self._window_max_chain is not None and self._window_max_chain < 0:
            raise ValueError(f'cem_gp_window_max_chain={wchain}: a row count, or None')
        self._drop_ws: Optional[Tensor] = None
        self._lockstep_bufs: Optional['_LockstepBuffers'] = None   # of the groups this model leads
        self._append_ok = False      # may the next update append to the installed fit?  (False after anything but a plain update)
        self._appended = 0           # rows appended since the last full fit
        self._fit_state = None       # the installed fit: (y, logdet on the device, the raw hyper-parameters and the floor)
        self._append_ws: Optional[Tensor] = None
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
        self._append_ok = False
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
        self._append_ok = False
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

    def _append_merged(self, new_x: Tensor, new_y: Tensor):
        """The merged training set (train_x, train_y) update_model(new_x, new_y) would store, where the shapes and devices
        alone allow an append; else None."""
        if not (self._incremental and self._append_ok and self._x_train is not None and self._y_train is not None
                and new_x.dim() == 2 and new_y.dim() == 2 and new_x.size(0) == new_y.size(0)
                and new_x.shape[1:] == self._x_train.shape[1:] and new_y.shape[1:] == self._y_train.shape[1:]
                and new_x.device == self._x_train.device and new_y.device == self._y_train.device):
            return None
        if not 1 <= new_x.size(0) <= MAX_APPEND_ROWS:
            return None
        return torch.cat((self._x_train, new_x), dim=0), torch.cat((self._y_train, new_y), dim=0)

    def _selects(self, n: int) -> bool:
        """Is a pool of n points cut down to conf.cem_gp_subset_size before it is fitted?"""
        return self._subset_size is not None and n > self._subset_size

    def _check_pool_size(self, n: int) -> None:
        if self._selects(n):
            if n > MAX_POOL_POINTS:
                raise ValueError(f'{n} training points: a subset is selected from up to {MAX_POOL_POINTS} (sx_gp_select)')
        elif n > MAX_TRAINING_POINTS:
            raise ValueError(f'{n} training points: the exact-GP kernels hold up to {MAX_TRAINING_POINTS} (sx_gp_fit); keep the '
                             f'most recent / most informative ones (update_model(..., replace_old=True), or '
                             f'conf.cem_gp_subset_size)')

    def select_subset(self, x: Tensor, m: int, seed_idx=None) -> Tuple[Tensor, Tensor]:
        """The max-variance subset of the pool x [n x D] (device, float64) under the current hyper-parameters
        (sx_gp_select): (idx LongTensor [m] in selection order, sel_var [m]), both on x's device.  seed_idx: up to m
        distinct rows that come first, in this order.  sel_var[j] is the predictive variance of x[idx[j]], noise included,
        given x[idx[:j]], summed over the outputs.  Raises RuntimeError where the selection meets a variance that is not
        positive (or a seed that is out of range or repeated)."""
        idx, sel_var = select_subsets_multi([self], [x], m, None if seed_idx is None else [seed_idx])
        return idx[0], sel_var[0]

    def _subset_of(self, x: Tensor, y: Tensor) -> Tuple[Tensor, Tensor]:
        """The rows of the pool (x, y) the model is fitted on, in selection order; remembers which (self._subset_idx)."""
        self._subset_idx = None
        if self._selects(x.size(0)):
            self._subset_idx = self.select_subset(x, self._subset_size)[0]
            x, y = x[self._subset_idx].contiguous(), y[self._subset_idx].contiguous()
        return x, y

    def update_model(self, train_x: Tensor, train_y: Tensor, opt_hyp=False, replace_old=False) -> None:
        # conf.cem_gp_incremental: only a plain update may append, and only to the fit a plain update left
        if opt_hyp or replace_old or self.parametric:
            self._append_ok = False
        super().update_model(train_x, train_y, opt_hyp, replace_old)
        if opt_hyp or self.parametric:
            self._append_ok = False

    def _hyper_state(self):
        return (self._raw_lengthscale, self._raw_outputscale, self._raw_noise, self._noise_floor)

    def _increment_rows_host(self, x: Tensor) -> Tuple[int, int]:
        """(r, k) where the update to the rows x (device, contiguous) may extend the installed fit by its last k rows after
        dropping the r oldest fitted ones (conf.cem_gp_incremental; r > 0: a slide of conf.cem_gp_window), as far as the host
        decides without reading from the device: all but the comparison of the kept fitted rows (`_compared`).  (0, 0): a
        full fit.
        One set of checks serves the append and the slide, and answers as the two separate ones would.  The limits on the
        total (N + k within the fit's size, no subset selected from it) are the append's, asked where r = 0; a windowed model
        below its window passes them as it always did, and a slide needs neither: a window excludes
        conf.cem_gp_subset_size and holds at most MAX_TRAINING_POINTS rows, and the slid fit has exactly that many.  The
        limits on r are the slide's; r > 0 exactly where the rows overflow the window."""
        if not (self._incremental and self._append_ok and self._linv_current and self._model is not None
                and self._fit_state is not None and self._subset_idx is None):
            return 0, 0
        fit_x = self._buffers[0]
        n, k = fit_x.size(0), x.size(0) - fit_x.size(0)
        r = 0 if self._window is None else max(0, n + k - self._window)
        if not 1 <= k <= MAX_APPEND_ROWS:
            return 0, 0
        if r == 0 and (n + k > MAX_TRAINING_POINTS or self._selects(n + k)):
            return 0, 0
        if r > 0 and not (r <= min(MAX_SLIDE_ROWS, MAX_DROP_ROWS) and r < n):
            return 0, 0
        if not self._chain_allows(k):
            return 0, 0
        if x.device != fit_x.device or self._fit_ws[1].size(1) != n or not self._hyper_unchanged():
            return 0, 0
        return r, k

    def _chain_allows(self, k: int) -> bool:
        """May k more rows be appended (or slid) before the next full fit?"""
        if self._max_chain is not None and self._appended + k > self._max_chain:
            return False
        return not (self._window is not None and self._window_max_chain is not None
                    and self._appended + k > self._window_max_chain)

    def _hyper_unchanged(self) -> bool:
        """Are the hyper-parameters those of the installed fit?  (host tensors, compared on the host)"""
        now, hyper = self._hyper_state(), self._fit_state[2]
        return now[3] == hyper[3] and all(a.shape == b.shape and bool((a == b).all()) for a, b in zip(now[:3], hyper[:3]))

    def _compared(self, x: Tensor, y: Tensor, r: int, k: int):
        """The row blocks (new x, fitted x, new y, fitted y) whose pairwise equality makes (x, y) the installed fit less its r
        oldest rows plus k new ones: the kept fitted rows themselves (the dropped ones no longer matter), compared where
        they live."""
        n = x.size(0) - k
        fit_x, fit_y = self._buffers[0], self._fit_state[0]
        if r:
            fit_x, fit_y = fit_x[r:], fit_y[r:]
        return x[r:n], fit_x, y[r:n], fit_y

    def _increment_rows(self, x: Tensor, y: Tensor) -> Tuple[int, int]:
        """`_increment_rows_host` and the comparison of the kept fitted rows, which reads from the device: (r, k) where the
        update to the merged data (x, y) (on the device; any strides) may drop the r oldest fitted rows and append its
        last k; (0, 0): a full fit."""
        r, k = self._increment_rows_host(x)
        if k == 0:
            return 0, 0
        new_x, fit_x, new_y, fit_y = self._compared(x, y, r, k)
        return (r, k) if torch.equal(new_x, fit_x) and torch.equal(new_y, fit_y) else (0, 0)

    def _append_rows(self, x: Tensor, y: Tensor) -> int:
        """k, the rows by which (x, y) (device) extend the installed fit where the update may append them
        (conf.cem_gp_incremental); 0: a full fit.  `_increment_rows` where nothing is dropped, which is all a model without
        a window can ask for."""
        r, k = self._increment_rows(x, y)
        return k if r == 0 else 0

    def _drop(self, y_kept: Tensor, r: int):
        """sx_gp_drop of the r oldest rows of the installed fit; y_kept: the kept rows' targets (device, contiguous).  Returns
        (linv, alpha, logdet, status) of the kept rows in fresh buffers, the status word not yet read."""
        lib = _lib.lib()
        dev = y_kept.device
        n_s, n = self.num_states, self._fit_ws[1].size(1)
        nbytes = _workspace_bytes(lib.sx_gp_drop_workspace_bytes, n_s, n, r)
        self._drop_ws = _grown(self._drop_ws, nbytes, dev)
        (linv,), (alpha,), logdet, status = _outputs(n_s, (n - r,), dev)
        _lib.check(lib.sx_gp_drop(n_s, n, r, _lib.ptr(y_kept), _lib.ptr(self._fit_ws[1]), _lib.ptr(linv), _lib.ptr(alpha),
                                  _lib.ptr(logdet), _lib.ptr(status), _lib.ptr(self._drop_ws), nbytes, _lib.stream_ptr(dev)),
                   'sx_gp_drop')
        return linv, alpha, logdet, status

    def _increment(self, x: Tensor, y: Tensor, r: int, k: int) -> bool:
        """The increment (r, k) of the installed fit to the rows x[r:] of (x, y) (device, contiguous) through the single-model
        entries: sx_gp_drop of the r oldest fitted rows (r > 0: a slide), then sx_gp_append of the last k rows onto its
        outputs (onto the installed fit where r = 0), into fresh buffers that become the fit workspace, and `_commit`.  The
        two calls share one status word, so that one read decides for both.  False (and nothing changed) where either
        answers SX_STATUS_NOT_PD."""
        lib = _lib.lib()
        dev = x.device
        n_s = self.num_states
        linv_old, alpha_old, logdet_old, status = self._fit_ws[1], self._alpha, self._fit_state[1], None
        if r:
            x, y = x[r:].contiguous(), y[r:].contiguous()
            linv_old, alpha_old, logdet_old, status = self._drop(y[:self._buffers[0].size(0) - r].contiguous(), r)
        n2 = x.size(0)
        m = self._fit_struct(x)
        nbytes = _workspace_bytes(lib.sx_gp_append_workspace_bytes, n_s, n2, k)
        self._append_ws = _grown(self._append_ws, nbytes, dev)
        (linv,), (alpha,), logdet, status = _outputs(n_s, (n2,), dev, status)
        _lib.check(lib.sx_gp_append(ctypes.byref(m), n2 - k, _lib.ptr(y), _lib.ptr(linv_old), _lib.ptr(alpha_old),
                                    _lib.ptr(logdet_old), _lib.ptr(linv), _lib.ptr(alpha), _lib.ptr(logdet),
                                    _lib.ptr(status), _lib.ptr(self._append_ws), nbytes, _lib.stream_ptr(dev)), 'sx_gp_append')
        # (the status first: where S is not positive definite the outputs are unspecified and nothing is packed from them)
        if int(status.item()) & _lib.SX_STATUS_NOT_PD:
            return False
        self._commit(x, y, m, linv, alpha, logdet, k)
        return True

    def _commit(self, x: Tensor, y: Tensor, m: _lib.SxGpModel, linv: Tensor, alpha: Tensor, logdet_dev: Tensor, k: int,
                logdet: Optional[Tensor] = None) -> None:
        """Makes the increment by k rows (m, linv, alpha, logdet_dev), checked to be positive definite, the model's fit of the
        rows (x, y): sx_gp_pack, the fresh linv as the fit workspace, `_install`, and k more rows counted since the last full
        fit.  logdet: the host copy of logdet_dev where the caller has read it already (the lockstep call's one read)."""
        packed = self._pack(m, linv, alpha)
        # (no `work` of this size exists: the next full fit allocates its own)
        self._fit_ws = (linv.new_empty((self.num_states, 0, 0)), linv)
        self._install(x, m, packed, alpha, logdet_dev.cpu() if logdet is None else logdet, y=y, logdet_dev=logdet_dev)
        self._appended += k

    def _apply(self, train_x: Tensor, train_y: Tensor, r: int = 0, k: int = 0) -> None:
        """The update to the merged data (train_x, train_y) whose verdict is (r, k), `_increment_rows`' or the lockstep
        decision's: the stored data are trimmed to the window's last m rows (conf.cem_gp_window), the increment is applied,
        and where there is none (k = 0), or it answers SX_STATUS_NOT_PD, the model is fitted in full on exactly the stored
        rows.  The caller has checked the data (`_check_data`)."""
        trims = self._window is not None and train_x.size(0) > self._window
        x, y = train_x.detach().contiguous(), train_y.detach().contiguous()
        if trims:
            train_x, train_y = train_x[-self._window:], train_y[-self._window:]
        self._x_train, self._y_train = train_x, train_y
        if k and self._increment(x, y, r, k):
            return
        if trims:
            x, y = x[-self._window:], y[-self._window:]
        # conf.cem_gp_subset_size: the max-variance subset of a larger pool (sx_gp_select) is what gets fitted
        x, y = self._subset_of(x, y)
        # factorise on the device (sx_gp_fit), then lay the operands out for the matrix cores (sx_gp_pack)
        m, linv, alpha, logdet, status = self._fit(x, y)
        packed = self._pack(m, linv, alpha)
        if int(status.item()) & _lib.SX_STATUS_NOT_PD:
            raise RuntimeError('the kernel matrix K + noise I is not positive definite for the current hyper-parameters')
        self._install(x, m, packed, alpha, logdet.cpu(), y=y, logdet_dev=logdet)
        self._appended = 0

    def _check_data(self, train_x: Tensor, train_y: Tensor) -> None:
        """Raises where the merged data are more rows than the model holds (a window holds any number: it keeps the last m)
        or do not live on the GPU as float64."""
        if self._window is None or train_x.size(0) <= self._window:
            self._check_pool_size(train_x.size(0))
        _lib.require_gpu(train_x, 'train_x')
        _lib.require_gpu(train_y, 'train_y')

    def _update_model(self, x_train: Tensor, y_train: Tensor) -> None:
        """The warm path of one model: the data checked, one decision (`_increment_rows`), then `_apply`."""
        self._check_data(x_train, y_train)
        self._apply(x_train, y_train, *self._increment_rows(x_train, y_train))

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

    def _install(self, x: Tensor, m: _lib.SxGpModel, packed: Tuple[Tensor, Tensor], alpha: Tensor, logdet: Tensor,
                 y: Optional[Tensor] = None, logdet_dev: Optional[Tensor] = None) -> None:
        """Makes the packed fit of x the model's (logdet: host [n_s]); the fit workspace holds its W.  y, logdet_dev: the
        fitted targets and the device copy of logdet, which a later update needs to append to this fit
        (conf.cem_gp_incremental)."""
        self._model = m
        self._buffers = (x,) + tuple(packed)
        self._alpha = alpha
        self._linv_current = True
        self._append_ok = self._incremental and y is not None and logdet_dev is not None
        self._fit_state = (y, logdet_dev, tuple(t.clone() if isinstance(t, Tensor) else t for t in self._hyper_state())) \
            if self._append_ok else None
        # 1/2 log det(I + K_d / noise_d) = sum log diag L_d - N/2 log noise_d
        self._info_gain = (logdet - 0.5 * x.size(0) * torch.log(self.noise)).numpy()

    def mll_and_grad(self, x_train: Tensor, y_train: Tensor):
        """Exact marginal log likelihood per output [n_s] and its gradient [n_s x (D + 2)] w.r.t.
        (lengthscale, outputscale, noise), at the current hyper-parameters (host tensors)."""
        x, y = x_train.detach().contiguous(), y_train.detach().contiguous()
        self._append_ok = False
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
        self._workspace = _grown(self._workspace, nbytes, self._buffers[0].device)
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
        if self._window is not None:
            # (the caller's merged data; the update before this call has trimmed the stored rows to the same window)
            x_train, y_train = x_train[-self._window:], y_train[-self._window:]
        pool_x, pool_y = x_train, y_train
        if self._subset_idx is not None:
            # a bounded model trains on the subset its last fit selected; the closing _update_model selects once more,
            # with the trained hyper-parameters (the reference's single re-optimisation, gaussian_process.py:279-344)
            x_train = x_train.detach()[self._subset_idx].contiguous()
            y_train = y_train.detach()[self._subset_idx].contiguous()
        n = x_train.size(0)
        raw = [self._raw_lengthscale.clone().requires_grad_(True), self._raw_outputscale.clone().requires_grad_(True),
               self._raw_noise.clone().requires_grad_(True)]
        opt = torch.optim.Adam(raw, lr=0.01)
        losses = []
        for _ in range(self._training_iterations):
            self._raw_lengthscale, self._raw_outputscale, self._raw_noise = (t.detach() for t in raw)
            mll, grad = self.mll_and_grad(x_train, y_train)
            losses.append(float(-(mll / n).sum()))
            _adam_grads(raw, grad, n)
            opt.step()
        self._raw_lengthscale, self._raw_outputscale, self._raw_noise = (t.detach().clone() for t in raw)
        self._last_training_losses = losses
        self._update_model(pool_x, pool_y)

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
            x, y = self._x_train.detach().contiguous(), self._y_train.detach().contiguous()
            if self._subset_idx is not None:
                x, y = x[self._subset_idx].contiguous(), y[self._subset_idx].contiguous()
            self._fit(x, y)
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


# ---- max-variance subsets of E pools in one call (sx_gp_select) ---------------------------------------------------------------
def select_subsets_multi(ssms: Sequence['GpCemSSM'], xs: Sequence[Tensor], m: int, seed_idx=None,
                         raws: Optional[Sequence[Optional[Tuple[Tensor, Tensor, Tensor]]]] = None) -> Tuple[Tensor, Tensor]:
    """``ssms[e].select_subset(xs[e], m)`` for every e in ONE sx_gp_select call (an init launch per 8 problems and one launch
    per greedy step for all of them): (idx LongTensor [E x m], sel_var [E x m]) on the pools' device, problem e's rows
    bit-identical to the single call.  The models are exact RBF GPs of one (n_s, n_u), each with its own
    hyper-parameters (raws[e]: raw parameters to use in place of the model's own); the pools xs[e] [n_e x D] live on one
    device and may differ in size, m <= min n_e.  seed_idx: E sequences of one length n_seed <= m, rows that come first.
    RuntimeError naming the problem where a selection fails (a variance that is not positive, a bad seed)."""
    lib = _lib.lib()
    ssms, xs = list(ssms), list(xs)
    E = len(ssms)
    if E == 0 or len(xs) != E:
        raise ValueError(f'{E} models, {len(xs)} pools')
    first = ssms[0]
    if not all(isinstance(s, GpCemSSM) and s.kernel_family == 'rbf'
               and (s.num_states, s.num_actions) == (first.num_states, first.num_actions) for s in ssms):
        raise ValueError('select_subsets_multi takes exact RBF GPs (GpCemSSM) of one (n_s, n_u)')
    dev, d_in, m = xs[0].device, first.num_states + first.num_actions, int(m)
    pools = []
    for x in xs:
        _lib.require_gpu(x, 'x')
        assert_shape(x, (x.size(0), d_in))
        if x.device != dev:
            raise ValueError('the pools must live on one device')
        pools.append(x.detach().contiguous())
    n_min, n_max = min(x.size(0) for x in pools), max(x.size(0) for x in pools)
    if not 1 <= m <= n_min:
        raise ValueError(f'm={m}: a subset holds 1 .. {n_min} points (the smallest pool)')
    if m > MAX_TRAINING_POINTS or n_max > MAX_POOL_POINTS:
        raise ValueError(f'm={m}, {n_max} pool points: sx_gp_select takes m <= {MAX_TRAINING_POINTS} of up to {MAX_POOL_POINTS}')
    seeds, n_seed = None, 0
    if seed_idx is not None:
        seeds = torch.stack([torch.as_tensor(s, dtype=torch.int32).reshape(-1).cpu() for s in seed_idx]).to(dev).contiguous()
        if seeds.size(0) != E or seeds.size(1) > m:
            raise ValueError(f'seed_idx: {E} sequences of one length <= m, got {tuple(seeds.shape)}')
        n_seed = seeds.size(1)
        if n_seed == 0:
            seeds = None
    raws = list(raws) if raws is not None else [None] * E
    models = (_lib.SxGpModel * E)(*[s._fit_struct(x, raw) for s, x, raw in zip(ssms, pools, raws)])
    nbytes = _workspace_bytes(lib.sx_gp_select_workspace_bytes, first.num_states, E, n_max, m)
    workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    idx = torch.empty((E, m), dtype=torch.int32, device=dev)
    sel_var = torch.empty((E, m), dtype=torch.float64, device=dev)
    status = torch.zeros(E, dtype=torch.int32, device=dev)
    _lib.check(lib.sx_gp_select(models, E, m, _lib.ptr(seeds), n_seed, _lib.ptr(idx), _lib.ptr(sel_var), _lib.ptr(status),
                                _lib.ptr(workspace), nbytes, _lib.stream_ptr(dev)), 'sx_gp_select')
    host = status.cpu()
    for e in range(E):
        if int(host[e]) & _lib.SX_STATUS_NOT_PD:
            raise RuntimeError(f'problem {e}: the subset selection met a predictive variance that is not positive (K + noise I '
                               f'is not positive definite for the current hyper-parameters) or a seed that is out of range '
                               f'or repeated')
    return idx.long(), sel_var


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
        arr = _ptr_array
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


class _LockstepBuffers:
    """What a lockstep increment keeps between calls, with the model that leads the group: the one workspace allocation the
    problems' workspaces are cut from, and the problem table in pinned host memory and on the device.  Each grows on
    demand.  (A call ends in a host read of its results, so the previous call's copy of the table has completed.)"""

    def __init__(self):
        self.ws: Optional[Tensor] = None
        self.host_table: Optional[Tensor] = None
        self.table: Optional[Tensor] = None
        self._drop: Optional['_LockstepBuffers'] = None

    @property
    def drop(self) -> '_LockstepBuffers':
        """The same three for the lockstep drop of a slide (`_increment_group`): its table is still being copied when the
        append's is written, so the two calls do not share one."""
        if self._drop is None:
            self._drop = _LockstepBuffers()
        return self._drop

    def operands(self, sizes: List[int], table_bytes: int, dev):
        """What one table call over E = len(sizes) problems takes from here: (the problems' workspaces (void* [E]) cut from
        the one allocation, their sizes (int64 [E], each a multiple of 8 bytes), the host table, the device table)."""
        # (a quarter more than asked for: the training sets grow by a few rows from call to call)
        self.ws = _grown(self.ws, sum(sizes), dev, slack=sum(sizes) // 4)
        ptrs, at = [], self.ws.data_ptr()
        for nbytes in sizes:
            ptrs.append(at)
            at += nbytes
        if self.table is None or self.table.numel() < table_bytes or self.table.device != dev:
            self.host_table = torch.empty(table_bytes, dtype=torch.uint8, pin_memory=True)
            self.table = torch.empty(table_bytes, dtype=torch.uint8, device=dev)
        E = len(sizes)
        return ((ctypes.c_void_p * E)(*ptrs), (ctypes.c_int64 * E)(*sizes), self.host_table[:table_bytes],
                self.table[:table_bytes])


class _Increment(NamedTuple):
    """A model's verdict where its plain update extends the installed fit: the r oldest fitted rows dropped (0: an append,
    > 0: a slide), the last k rows of the merged data (train_x, train_y) appended."""
    r: int
    k: int
    train_x: Tensor
    train_y: Tensor


_ALONE, _FIT = 'alone', 'fit'     # the other two verdicts: the model's own update_model; fitted together with the other `fit` models


def _increment_group(ssms: List['GpCemSSM'], merged: List[Tuple[Tensor, Tensor]], r: int, k: int) -> None:
    """`GpCemSSM._apply` of E >= 2 models with one verdict (r, k), through the table entries.  r > 0: ONE sx_gp_drop_table +
    sx_gp_drop_multi (seven launches for all of them) of the r oldest fitted rows into fresh per-model buffers.  Then ONE
    sx_gp_append_table + sx_gp_append_multi (six launches) of the last k rows onto those outputs (onto the installed fits where
    r = 0), sharing the E status words, and one host read of the words and the E x n_s log-determinants, which decides for
    both calls as the single-model increment's one word does.  (The words are not read after the drop: where it is not
    positive definite the append runs on unspecified inputs, writes only its own outputs, and the shared word says so.)
    Then, per model, `GpCemSSM._commit` on the rows x[r:].  Model e's state afterwards equals, bit for bit, what its own
    update_model leaves.  A model that either call finds not positive definite is fitted in full on its stored rows, alone,
    after the others have been installed (and raises there as it always did); nothing is packed from its outputs.
    merged[e]: the untrimmed training set (stored rows, then the new ones)."""
    lib = _lib.lib()
    E, lead = len(ssms), ssms[0]
    n_s = lead.num_states
    if lead._lockstep_bufs is None:
        lead._lockstep_bufs = _LockstepBuffers()
    data = []
    for m, (train_x, train_y) in zip(ssms, merged):
        m._check_data(train_x, train_y)
        x, y = train_x.detach().contiguous(), train_y.detach().contiguous()
        data.append((x[r:].contiguous(), y[r:].contiguous()) if r else (x, y))
    dev = data[0][0].device
    start, status = [(m._fit_ws[1], m._alpha, m._fit_state[1]) for m in ssms], None
    if r:
        n_old = [m._fit_ws[1].size(1) for m in ssms]
        kept_y = [y[:n - r].contiguous() for (_, y), n in zip(data, n_old)]
        sizes = [_workspace_bytes(lib.sx_gp_drop_workspace_bytes, n_s, n, r) for n in n_old]
        linv, alpha, logdet, status = _outputs(n_s, [n - r for n in n_old], dev)
        logdet = logdet.view(E, n_s)
        ws, ws_bytes, host_table, table = lead._lockstep_bufs.drop.operands(sizes, int(lib.sx_gp_drop_table_bytes(E)), dev)
        n_arr = (ctypes.c_int * E)(*n_old)
        _lib.check(lib.sx_gp_drop_table(n_s, E, r, n_arr, _ptr_array(kept_y), _ptr_array([st[0] for st in start]),
                                        _ptr_array(linv), _ptr_array(alpha), _ptr_array(list(logdet)), _lib.ptr(status), ws,
                                        ws_bytes, ctypes.c_void_p(host_table.data_ptr())), 'sx_gp_drop_table')
        table.copy_(host_table, non_blocking=True)
        _lib.check(lib.sx_gp_drop_multi(n_s, E, r, n_arr, _lib.ptr(table), _lib.stream_ptr(dev)), 'sx_gp_drop_multi')
        start = list(zip(linv, alpha, logdet))
    models = (_lib.SxGpModel * E)(*[m._fit_struct(x) for m, (x, _) in zip(ssms, data)])
    sizes = [_workspace_bytes(lib.sx_gp_append_workspace_bytes, n_s, x.size(0), k) for x, _ in data]
    linv, alpha, logdet, status = _outputs(n_s, [x.size(0) for x, _ in data], dev, status)
    logdet = logdet.view(E, n_s)
    ws, ws_bytes, host_table, table = lead._lockstep_bufs.operands(sizes, int(lib.sx_gp_append_table_bytes(E)), dev)
    _lib.check(lib.sx_gp_append_table(models, E, k, _ptr_array([y for _, y in data]), _ptr_array([st[0] for st in start]),
                                      _ptr_array([st[1] for st in start]), _ptr_array([st[2] for st in start]),
                                      _ptr_array(linv), _ptr_array(alpha), _ptr_array(list(logdet)), _lib.ptr(status), ws,
                                      ws_bytes, ctypes.c_void_p(host_table.data_ptr())), 'sx_gp_append_table')
    table.copy_(host_table, non_blocking=True)
    _lib.check(lib.sx_gp_append_multi(models, E, k, _lib.ptr(table), _lib.stream_ptr(dev)), 'sx_gp_append_multi')
    host = torch.cat((status.double(), logdet.reshape(-1))).cpu()      # the call's one read of its results
    logdets = host[E:].reshape(E, n_s)
    bad = [bool(int(host[e]) & _lib.SX_STATUS_NOT_PD) for e in range(E)]
    for e, (m, (train_x, train_y)) in enumerate(zip(ssms, merged)):
        if bad[e]:
            continue    # (its outputs are unspecified and nothing is packed from them)
        # (r > 0 only where the merged rows overflow the window: the stored data are its last m rows)
        m._x_train, m._y_train = (train_x[-m._window:], train_y[-m._window:]) if r else (train_x, train_y)
        m._commit(*data[e], _lib.SxGpModel.from_buffer_copy(models[e]), linv[e], alpha[e], logdet[e], k,
                  logdet=logdets[e].clone())
    for e, m in enumerate(ssms):
        if bad[e]:
            m._apply(*merged[e])


def _verdicts(ssms: List[CemSSM], xs: List[Tensor], ys: List[Tensor], plain: bool):
    """The one verdict of every model of an update_models_multi call -- `_ALONE`, `_FIT` or an `_Increment` -- and the
    models that go alone in the order in which they do.
    Alone: a windowed model (conf.cem_gp_window) unless it has conf.cem_gp_incremental_lockstep and the update is a `plain`
    one (no opt_hyp, no replace_old); these go last.  And, once they are taken out, every model of a list that does not train
    together (`_multi_fit_applies`).  The others are fitted together -- but for those whose plain update extends their
    installed fit.  A model without conf.cem_gp_incremental_lockstep (it has no window here) decides by itself, reading its
    row comparison from the device, in index order (`_append_rows`); the models with the setting are decided together: the
    host checks per model, then the comparisons of all their kept fitted rows as one flag each, stacked and read once."""
    last = [i for i, m in enumerate(ssms)
            if getattr(m, '_window', None) is not None and not (plain and getattr(m, '_lockstep', False))]
    rest = [i for i in range(len(ssms)) if i not in last]
    if rest and not _multi_fit_applies([ssms[i] for i in rest], [xs[i] for i in rest]):
        return [_ALONE] * len(ssms), rest + last
    verdicts: List[Any] = [_ALONE if i in last else _FIT for i in range(len(ssms))]
    cands, flags = [], []
    for i in rest if plain else ():
        m = ssms[i]
        merged = m._append_merged(xs[i], ys[i])
        if merged is None:
            continue
        x, y = merged
        if not m._lockstep:
            k = m._append_rows(x, y)
            if k:
                verdicts[i] = _Increment(0, k, *merged)
            continue
        r, k = m._increment_rows_host(x)
        if k:
            cands.append((i, _Increment(r, k, *merged)))
            new_x, fit_x, new_y, fit_y = m._compared(x, y, r, k)
            flags.append((new_x == fit_x).all() & (new_y == fit_y).all())
    if cands:
        same = torch.stack(flags).cpu()                                # the decision's one read
        for (i, verdict), ok in zip(cands, same):
            if bool(ok):
                verdicts[i] = verdict
    return verdicts, last


def _fit_together(ssms: List['GpCemSSM'], xs: List[Tensor], ys: List[Tensor], opt_hyp: bool, replace_old: bool) -> None:
    """The update of the models whose verdict is `_FIT` (they train together, `_multi_fit_applies`): hyper-parameter
    training in lockstep where the update asks for it, then one batched fit and a commit per model.  Nothing is committed
    before the final fit has succeeded everywhere."""
    # the merged training sets, checked before anything changes
    merged = []
    for m, x, y in zip(ssms, xs, ys):
        n = x.size(0)
        assert_shape(x, (n, m.num_states + m.num_actions))
        assert_shape(y, (n, m.num_states))
        if not replace_old and m._x_train is not None and m._y_train is not None:
            x, y = torch.cat((m._x_train, x), dim=0), torch.cat((m._y_train, y), dim=0)
        if m._window is not None:
            x, y = x[-m._window:], y[-m._window:]     # (a windowed lockstep model that neither appends nor slides)
        m._check_pool_size(x.size(0))
        _lib.require_gpu(x, 'train_x')
        _lib.require_gpu(y, 'train_y')
        merged.append((x, y))
    # conf.cem_gp_subset_size: where every model cuts its pool down to one size, all selections go in one sx_gp_select call
    # and the lockstep fit below runs on the subsets; a mixed list is updated one model at a time
    selecting = [m._selects(x.size(0)) for m, (x, _) in zip(ssms, merged)]
    if any(selecting) and not (all(selecting) and len({m._subset_size for m in ssms}) == 1):
        for m, x, y in zip(ssms, xs, ys):
            m.update_model(x, y, opt_hyp, replace_old)
        return
    selecting = all(selecting)
    pools = [(x.detach().contiguous(), y.detach().contiguous()) for x, y in merged]
    raws = [(m._raw_lengthscale, m._raw_outputscale, m._raw_noise) for m in ssms]

    def subsets(raws):
        """the rows each model is fitted on at the raw hyper-parameters `raws` (all of them without the setting)"""
        if not selecting:
            return [None] * len(ssms), pools
        idx, _ = select_subsets_multi(ssms, [x for x, _ in pools], ssms[0]._subset_size, raws=raws)
        return list(idx), [(x[i].contiguous(), y[i].contiguous()) for (x, y), i in zip(pools, idx)]

    subset_idx, data = subsets(raws)
    fit = _MultiFit(ssms, [x for x, _ in data], [y for _, y in data])
    E, n_s, d_in = len(ssms), ssms[0].num_states, ssms[0].num_states + ssms[0].num_actions
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
                mll = host[e * n_s:(e + 1) * n_s].clone()
                losses[e].append(float(-(mll / n).sum()))
                _adam_grads(p, grads[e], n)
            opt.step()
        raws = [tuple(t.detach().clone() for t in p) for p in params]
        if selecting:
            # select once more, with the trained hyper-parameters, as the single-model update does
            subset_idx, data = subsets(raws)
            fit = _MultiFit(ssms, [x for x, _ in data], [y for _, y in data])
    # the final fit at the trained hyper-parameters; nothing is committed before it has succeeded everywhere
    fit.new_alpha()
    models = fit.launch(raws, mll=False)
    host = torch.cat((fit.status.double(), fit.logdet.reshape(-1))).cpu()
    fit.check_status(host[:E])
    logdets = host[E:].reshape(E, n_s)
    for e, m in enumerate(ssms):
        m._x_train, m._y_train = merged[e]
        m._subset_idx = subset_idx[e]
        m._raw_lengthscale, m._raw_outputscale, m._raw_noise = raws[e]
        if losses is not None:
            m._last_training_losses = losses[e]
        model = _lib.SxGpModel.from_buffer_copy(models[e])
        packed = m._pack(model, fit.ws[e][1], fit.alpha[e])
        m._install(fit.xs[e], model, packed, fit.alpha[e], logdets[e].clone(), y=fit.ys[e], logdet_dev=fit.logdet[e])
        m._appended = 0
        if opt_hyp or m.parametric:
            m._append_ok = False    # as update_model: the update after hyper-parameter training is a full fit


def update_models_multi(ssms: Sequence[CemSSM], xs: Sequence[Tensor], ys: Sequence[Tensor], opt_hyp=False,
                        replace_old=False) -> None:
    """``m.update_model(x, y, opt_hyp, replace_old)`` for every (m, x, y) at once: the reference's n_scenarios models, each
    retrained on its own data after every episode (episode_runner.py:55,123).  Every model ends in the state its own
    update_model leaves, bit for bit: data (trimmed to conf.cem_gp_window), hyper-parameters, loss curves
    (``_last_training_losses``) and predictions.

    One pass (`_verdicts`) gives every model one of four verdicts, and the work is done in this order:

    * **fit**: exact RBF GPs of one (n_s, n_u) and one iteration count train in lockstep (`_fit_together`), first: per Adam
      step ONE sx_gp_fit_multi and ONE sx_gp_mll_grad_multi launch sequence for all of them and one host read, then one
      batched fit and an sx_gp_pack per model.  Adam is the recipe of GpCemSSM._train_model, one optimizer over every
      model's raw parameters; its update is elementwise, and each model keeps its own parameter tensors, so each follows
      the trajectory it would follow alone.  A kernel matrix that is not positive definite in problem e (counted among the
      fitted models) raises RuntimeError naming e, and then none of these models' data, hyper-parameters or predictions
      have changed.  (Each model's fit workspace serves the batch from the start, so after such a call its cached
      W = L^-1 is marked stale, and its next predict_variance_jacobian factorises once more -- as after a failed
      single-model update.)  Where some of them select a max-variance subset (conf.cem_gp_subset_size) and others do not,
      or not one size, they are updated one model at a time instead.
    * **append (k)** and **slide (r, k)** (conf.cem_gp_incremental, a plain update -- no opt_hyp, no replace_old -- whose
      data extend the installed fit by k rows, after dropping its r oldest where it overflows conf.cem_gp_window): the
      models with conf.cem_gp_incremental_lockstep that share (r, k) and the device form a group, the groups of two or
      more go next, in the order in which their first members stand in the list, each in ONE sx_gp_append_multi call, after
      ONE sx_gp_drop_multi call where r > 0 (`_increment_group`); two host reads for all lockstep models whatever their
      number, one for the decision and one for the results.  Then the remaining ones, alone and in the order of the list
      (sx_gp_append, after sx_gp_drop where r > 0: `GpCemSSM._apply`).  A model that is not positive definite there is fitted
      in full, alone, after the others of its group have been installed.
    * **alone**, last: its own update_model.  A windowed model goes alone unless it has conf.cem_gp_incremental_lockstep
      and the update is a plain one; so does every model of any other list (other families, JunkDimensionsSSM, differing
      shapes or iteration counts, data on several devices)."""
    ssms, xs, ys = list(ssms), list(xs), list(ys)
    if not len(ssms) == len(xs) == len(ys):
        raise ValueError(f'{len(ssms)} models, {len(xs)} input sets, {len(ys)} target sets')
    verdicts, alone = _verdicts(ssms, xs, ys, plain=not opt_hyp and not replace_old)
    fitted = [i for i, v in enumerate(verdicts) if v is _FIT]
    if fitted:
        _fit_together([ssms[i] for i in fitted], [xs[i] for i in fitted], [ys[i] for i in fitted], opt_hyp, replace_old)
    groups: Dict[Tuple[int, int, Any], List[int]] = {}
    for i, v in enumerate(verdicts):
        if isinstance(v, _Increment) and ssms[i]._lockstep:
            groups.setdefault((v.r, v.k, v.train_x.device), []).append(i)
    grouped = set()
    for (r, k, _), members in groups.items():
        if len(members) >= 2:
            _increment_group([ssms[i] for i in members], [verdicts[i][2:] for i in members], r, k)
            grouped.update(members)
    for i, v in enumerate(verdicts):
        if isinstance(v, _Increment) and i not in grouped:
            ssms[i]._check_data(v.train_x, v.train_y)
            ssms[i]._apply(v.train_x, v.train_y, v.r, v.k)
    for i in alone:
        ssms[i].update_model(xs[i], ys[i], opt_hyp, replace_old)
