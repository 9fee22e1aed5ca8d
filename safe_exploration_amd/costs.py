"""Kernel-form objectives of the Taylor rollouts beyond sx_env's two modes.

`SaturatingCost` is the PILCO saturating loss of the trigonometrically augmented state Gaussian, the cost the reference's
cart-pole configs hand to `init_solver` (experiments/journal_experiment_configs/defaultconfig_episode.py:113-159 over
utils_casadi.py: trig_prop / trig_aug with a = 1, keep_radian = False, loss_sat, generic_cost).  As `sx_sat_cost` it is
the objective of sx_cem_perf_rollout_taylor_sat[_multi] and sx_cem_cautious_rollout_sat."""
import ctypes
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib

RANK_TOL = 1e-12      # eigenvalues of the weight below RANK_TOL * the largest are dropped (and none may lie below minus that)


class SaturatingCost:
    """loss(mu, Sigma) = 1 - exp(-1/2 d^T W (I + S~ W)^-1 d) / sqrt(det(I + S~ W)), d = m~ - target, over the augmented
    Gaussian (m~, S~): the state without entry `trig_idx`, then sin and cos of it (n_a = n_s + 1); without `trig_idx`
    the state itself (n_a = n_s).  A trajectory costs the sum of the loss over its states mu_1 .. mu_T.

    target [n_a], weight [n_a x n_a] symmetric positive semi-definite and not zero.  `struct` is the `_lib.SxSatCost` the
    library takes: W = V V^T with V [n_a x k] from the symmetric eigendecomposition of the weight, k its rank."""

    def __init__(self, target, weight, trig_idx: Optional[int] = None):
        z = np.asarray(target, dtype=np.float64)
        w = np.asarray(weight, dtype=np.float64)
        if z.ndim != 1 or z.size < 1:
            raise ValueError(f'target must be a vector, got shape {z.shape}')
        n_a = z.size
        n_s = n_a if trig_idx is None else n_a - 1
        if trig_idx is not None and (int(trig_idx) != trig_idx or not 0 <= int(trig_idx) < n_s):
            raise ValueError(f'trig_idx={trig_idx!r} must be None or a state index in 0 .. {n_s - 1} (target has n_s + 1 = '
                             f'{n_a} entries: the state without the angle, then its sin and cos)')
        if not 1 <= n_s <= _lib.SX_MAX_NS:
            raise ValueError(f'target of length {n_a} means n_s = {n_s}: the library is built for 1 <= n_s <= {_lib.SX_MAX_NS}')
        if w.shape != (n_a, n_a):
            raise ValueError(f'weight must be [{n_a} x {n_a}] like target, got shape {w.shape}')
        if not (np.isfinite(z).all() and np.isfinite(w).all()):
            raise ValueError('target and weight must be finite')
        if not np.allclose(w, w.T, rtol=0.0, atol=1e-12 * max(np.abs(w).max(), 1e-300)):
            raise ValueError('weight must be symmetric')
        lam, vec = np.linalg.eigh(0.5 * (w + w.T))
        if lam[-1] <= 0.0:
            raise ValueError('weight must be positive semi-definite and not zero')
        if lam[0] < -RANK_TOL * lam[-1]:
            raise ValueError(f'weight must be positive semi-definite: smallest eigenvalue {lam[0]:.3e}')
        keep = lam >= RANK_TOL * lam[-1]
        self.target, self.weight = z.copy(), 0.5 * (w + w.T)
        self.trig_idx = None if trig_idx is None else int(trig_idx)
        self.n_s, self.n_a = n_s, n_a
        self.v = np.ascontiguousarray(vec[:, keep] * np.sqrt(lam[keep]))      # [n_a x k]
        self.rank = int(self.v.shape[1])
        self.struct = _lib.SxSatCost()
        self.struct.trig_idx = -1 if self.trig_idx is None else self.trig_idx
        self.struct.rank = self.rank
        _lib.fill(self.struct.target, self.target)
        _lib.fill(self.struct.v, self.v)

    def _key(self):
        return (self.trig_idx, self.target.tobytes(), self.weight.tobytes())

    def __eq__(self, other):
        return isinstance(other, SaturatingCost) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f'SaturatingCost(n_s={self.n_s}, trig_idx={self.trig_idx}, rank={self.rank})'

    def augment(self, mu: Tensor, cov: Tensor):
        """(m~ [... x n_a], S~ [... x n_a x n_a]) of mu [... x n_s], cov [... x n_s x n_s] (trig_prop of the reference)."""
        i = self.trig_idx
        if i is None:
            return mu, cov
        keep = [j for j in range(self.n_s) if j != i]
        m, v = mu[..., i], cov[..., i, i]
        e0, e1 = torch.exp(-0.5 * v), torch.exp(-2.0 * v)
        s, c = e0 * torch.sin(m), e0 * torch.cos(m)
        vss = 0.5 * (1.0 - e1 * torch.cos(2.0 * m)) - s * s
        vcc = 0.5 * (1.0 + e1 * torch.cos(2.0 * m)) - c * c
        vsc = 0.5 * e1 * torch.sin(2.0 * m) - s * c
        col = cov[..., keep, i]                                              # Cov(x, angle) of the kept states
        ma = torch.cat([mu[..., keep], s[..., None], c[..., None]], dim=-1)
        sa = mu.new_zeros(mu.shape[:-1] + (self.n_a, self.n_a))
        k = len(keep)
        sa[..., :k, :k] = cov[..., keep, :][..., :, keep]
        sa[..., :k, k] = col * c[..., None]
        sa[..., k, :k] = sa[..., :k, k]
        sa[..., :k, k + 1] = -col * s[..., None]
        sa[..., k + 1, :k] = sa[..., :k, k + 1]
        sa[..., k, k], sa[..., k + 1, k + 1] = vss, vcc
        sa[..., k, k + 1] = vsc
        sa[..., k + 1, k] = vsc
        return ma, sa

    def __call__(self, mu: Tensor, cov: Tensor) -> Tensor:
        """The loss of mu [... x n_s], cov [... x n_s x n_s] in the reference's own inverse / determinant form (loss_sat),
        in float64 on the tensors' device.  Returns [...]."""
        mu, cov = mu.to(torch.float64), cov.to(torch.float64)
        if mu.size(-1) != self.n_s or cov.shape != mu.shape + (self.n_s,):
            raise ValueError(f'mu must be [... x {self.n_s}] and cov [... x {self.n_s} x {self.n_s}], got '
                             f'{tuple(mu.shape)}, {tuple(cov.shape)}')
        ma, sa = self.augment(mu, cov)
        w = torch.as_tensor(self.weight, dtype=torch.float64, device=mu.device)
        d = ma - torch.as_tensor(self.target, dtype=torch.float64, device=mu.device)
        isw = torch.eye(self.n_a, dtype=torch.float64, device=mu.device) + sa @ w
        sol = torch.linalg.solve(isw, d[..., None])[..., 0]                  # (I + S~ W)^-1 d
        q = ((d @ w) * sol).sum(-1)
        return 1.0 - torch.exp(-0.5 * q) / torch.sqrt(torch.linalg.det(isw))

    def evaluate_device(self, mu: Tensor, cov: Tensor, status: Optional[Tensor] = None) -> Tensor:
        """The loss of mu [P x n_s], cov [P x n_s x n_s] (float64, on the GPU) through sx_sat_cost_eval: the device function
        the rollouts price their steps with.  A non-finite loss comes back NaN and sets SX_STATUS_NAN in `status` (int32
        [1], or-ed into).  Returns [P]."""
        _lib.require_gpu(mu, 'mu')
        _lib.require_gpu(cov, 'cov')
        if mu.dim() != 2 or mu.size(1) != self.n_s or tuple(cov.shape) != (mu.size(0), self.n_s, self.n_s):
            raise ValueError(f'mu must be [P x {self.n_s}] and cov [P x {self.n_s} x {self.n_s}], got {tuple(mu.shape)}, '
                             f'{tuple(cov.shape)}')
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=mu.device)
        loss = torch.empty(mu.size(0), dtype=torch.float64, device=mu.device)
        _lib.check(_lib.lib().sx_sat_cost_eval(ctypes.byref(self.struct), self.n_s, mu.size(0), _lib.ptr(mu.contiguous()),
                                               _lib.ptr(cov.contiguous()), _lib.ptr(loss), _lib.ptr(status),
                                               _lib.stream_ptr(mu.device)), 'sx_sat_cost_eval')
        return loss
