"""The real-output models JunkDimensionsSSM hands to the fused rollout over a feature-space GP or an MC-dropout ensemble.

The wrapper's junk columns reach both kinds of model only through the first linear layer (the 'nn' feature network, the
dropout network; the 'linear' kernel's features are the input itself), and a column that is zero in every training row and
every query adds exactly 0 to ``W_1 z``.  The padded model's real outputs are therefore those of the same model over the
D = n_s + n_u + s columns that are ever non-zero (``JunkDimensionsSSM._kept_columns``): training rows ``[x, u, 0_s]``,
queries ``[x, 0_s, u]``, s = ``query_shift``.  ``feature_view`` and ``mlp_view`` build that model from the inner model's
current parameters as an ``sx_feat_model`` / ``sx_mlp_model`` for ``sx_cem_rollout_feat_junk`` / ``sx_cem_rollout_mlp_junk``.
"""
import ctypes
from typing import Sequence, Tuple

import torch
from torch import Tensor, nn

from .. import _lib
from ..utils import assert_shape
from .ssm_cem import CemSSM


class KeptColumnView(CemSSM):
    """A device model over the kept columns: n_s real outputs, D = n_s + n_u + s inputs, i.e. n_u + s "actions" (the junk
    columns a query fills, then the real actions).  ``kernel_family`` is the inner model's ('feature' or 'mlp');
    ``feat_model`` / ``mlp_model`` is what the rollout entry takes.  ``predict_*`` run sx_feat_predict / sx_mlp_predict, which
    are instantiated for the plain models' shapes only (of the views: (n_s, n_u + s) = (2, 2)); the others serve the fused
    rollout alone."""

    def __init__(self, family: str, model, buffers: Tuple[Tensor, ...], n_s: int, n_in: int):
        super().__init__(n_s, n_in - n_s)
        self.kernel_family = family
        self._model = model
        self._buffers = buffers      # keeps the device operands alive while the struct points at them

    @property
    def feat_model(self) -> _lib.SxFeatModel:
        assert self.kernel_family == 'feature'
        return self._model

    @property
    def mlp_model(self) -> _lib.SxMlpModel:
        assert self.kernel_family == 'mlp'
        return self._model

    def _predict_z(self, z: Tensor, jacobians: bool):
        n, d_in = z.size(0), self.num_states + self.num_actions
        assert_shape(z, (n, d_in))
        _lib.require_gpu(z, 'states/actions')
        if self.num_actions > _lib.SX_MAX_NU:
            raise NotImplementedError(f'the kept-column model over {d_in} inputs is rolled out only (sx_cem_rollout_*_junk): '
                                      f'prediction is instantiated for up to {_lib.SX_MAX_NU} actions')
        z = z.detach().contiguous()
        mean = torch.empty((n, self.num_states), dtype=torch.float64, device=z.device)
        var = torch.empty_like(mean)
        jac = torch.empty((n, self.num_states, d_in), dtype=torch.float64, device=z.device) if jacobians else None
        if n:
            entry = 'sx_feat_predict' if self.kernel_family == 'feature' else 'sx_mlp_predict'
            _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(self._model), _lib.ptr(z), n, _lib.ptr(mean), _lib.ptr(var),
                                                  _lib.ptr(jac), _lib.stream_ptr(z.device)), entry)
        return mean, var, jac

    def predict_with_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        return self._predict_z(self._join_states_actions(states, actions), True)

    def predict_without_jacobians(self, states: Tensor, actions: Tensor) -> Tuple[Tensor, Tensor]:
        mean, var, _ = self._predict_z(self._join_states_actions(states, actions), False)
        return mean, var

    def predict_raw(self, z: Tensor) -> Tuple[Tensor, Tensor]:
        mean, var, _ = self._predict_z(z, False)
        return mean, var

    def _update_model(self, x_train: Tensor, y_train: Tensor) -> None:
        raise NotImplementedError('a kept-column view is rebuilt from its inner model, not trained')

    def _train_model(self, x_train: Tensor, y_train: Tensor) -> None:
        raise NotImplementedError('a kept-column view is rebuilt from its inner model, not trained')

    def collect_metrics(self):
        return {}

    @property
    def parametric(self) -> bool:
        return True


def _first_layer_columns(linears: Sequence[nn.Linear], cols: Sequence[int], dev) -> list:
    """Flattened (W, b) of every layer in the device layout, W_1 cut to the kept input columns."""
    idx = torch.tensor(list(cols), dtype=torch.long, device=linears[0].weight.device)
    parts = []
    for i, lin in enumerate(linears):
        w = lin.weight.detach()
        parts += [(w.index_select(1, idx) if i == 0 else w).reshape(-1), lin.bias.detach().reshape(-1)]
    return [p.to(dev, torch.float64) for p in parts]


def feature_view(inner, cols: Sequence[int], n_s: int, x_kept: Tensor, y: Tensor) -> KeptColumnView:
    """The feature-space GP over the kept columns with the first n_s outputs of `inner` (a FeatureGpCemSSM over the padded
    columns): the network's first-layer weight columns at `cols`, the same PReLU slope, kernel scales and noises, refit by
    sx_feat_fit on the kept-column training rows `x_kept` [N x D] and the real targets `y` [N x n_s].  For the 'nn' kernel
    the features of every point are the padded model's; for the 'linear' kernel (phi = z) the padded A_d is, after a
    permutation, block diagonal in the kept and the junk features, so the kept block's posterior is this fit."""
    lib = _lib.lib()
    dev = x_kept.device
    d_in, n = len(cols), x_kept.size(0)
    assert_shape(x_kept, (n, d_in))
    assert_shape(y, (n, n_s))
    x_kept, y = x_kept.detach().contiguous(), y.detach().to(torch.float64).contiguous()
    net = inner._net
    widths = [d_in] + list(inner._widths[1:])
    net_buf = None
    if net is not None:
        net_buf = torch.cat(_first_layer_columns([m for m in net if isinstance(m, nn.Linear)], cols, dev)).contiguous()
    m = _lib.SxFeatModel()
    m.n_s, m.n_u = n_s, d_in - n_s
    m.n_feat = widths[-1]
    m.n_layers = len(widths) - 1
    m.normalise = 1 if net is not None else 0
    for i, w in enumerate(widths):
        m.width[i] = w
    m.prelu = float(net[-1].weight.detach().reshape(-1)[0]) if net is not None else 0.0
    _lib.fill(m.noise, inner.noise[:n_s].numpy())
    m.net = net_buf.data_ptr() if net_buf is not None else None
    F = m.n_feat
    phi = torch.empty((n, F), dtype=torch.float64, device=dev)
    _lib.check(lib.sx_feat_features(ctypes.byref(m), _lib.ptr(x_kept), n, _lib.ptr(phi), _lib.stream_ptr(dev)),
               'sx_feat_features')
    wbar = torch.empty((n_s, F), dtype=torch.float64, device=dev)
    minv = torch.empty((n_s, F, F), dtype=torch.float64, device=dev)
    stats = torch.empty((n_s, 3), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lam = (ctypes.c_double * n_s)(*[float(v) for v in (inner.noise / inner.kernel_scale)[:n_s]])
    _lib.check(lib.sx_feat_fit(ctypes.byref(m), _lib.ptr(phi), _lib.ptr(y), n, lam, _lib.ptr(wbar), _lib.ptr(minv),
                               _lib.ptr(stats), _lib.ptr(status), _lib.stream_ptr(dev)), 'sx_feat_fit')
    if int(status.item()) & _lib.SX_STATUS_NOT_PD:
        raise RuntimeError('Phi^T Phi + noise / c I over the kept columns is not positive definite')
    m.wbar, m.minv = wbar.data_ptr(), minv.data_ptr()
    return KeptColumnView('feature', m, (x_kept, net_buf, wbar, minv), n_s, d_in)


def mlp_view(inner, cols: Sequence[int], n_s: int) -> KeptColumnView:
    """The MC-dropout ensemble over the kept columns with the first n_s outputs of `inner` (a McDropoutSSM or
    GalConcreteDropoutSSM over the padded columns), from its frozen members: the first-layer weight columns and the input
    masks' columns at `cols`, the hidden layers as they are, and the output layer's mean rows [0, n_s) -- with predict_std
    also its log-std rows [n_s_pad, n_s_pad + n_s), n_s_pad = inner.num_states."""
    net = inner._model
    masks = inner._buffers[1]                               # [S x (width_0 + width_1 + ...)], width_0 = padded D
    dev = masks.device
    d_in, d_pad = len(cols), net.sizes[0]
    n_s_pad = inner.num_states
    rows = list(range(n_s)) + (list(range(n_s_pad, n_s_pad + n_s)) if inner._predict_std else [])
    linears = list(net.linears) + [net.out]
    parts = _first_layer_columns(linears, cols, dev)
    row_idx = torch.tensor(rows, dtype=torch.long, device=dev)
    w_out = parts[-2].view(linears[-1].weight.size(0), -1)   # (W_1 = W_out without hidden layers: columns already cut)
    parts[-2] = w_out.index_select(0, row_idx).reshape(-1)
    parts[-1] = parts[-1].index_select(0, row_idx)
    net_buf = torch.cat(parts).contiguous()
    col_idx = torch.tensor(list(cols), dtype=torch.long, device=dev)
    mask_buf = torch.cat((masks.index_select(1, col_idx), masks[:, d_pad:]), dim=1).contiguous()
    m = _lib.SxMlpModel()
    m.n_s, m.n_u, m.n_hidden = n_s, d_in - n_s, len(net.sizes) - 1
    m.n_out, m.n_samples, m.predict_std = len(rows), inner._mlp.n_samples, int(bool(inner._predict_std))
    for i, w in enumerate([d_in] + list(net.sizes[1:])):
        m.width[i] = w
    m.net, m.masks = net_buf.data_ptr(), mask_buf.data_ptr()
    return KeptColumnView('mlp', m, (net_buf, mask_buf), n_s, d_in)
