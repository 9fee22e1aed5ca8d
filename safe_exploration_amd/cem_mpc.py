"""The constrained cross-entropy optimiser, fused onto the GPU.

Stands where the reference uses the third-party ``constrained_cem_mpc.ConstrainedCemMpc`` (call sites:
``safe_exploration/safempc_cem.py:7-8,139,193-196,235,270,278``).  That library drives the rollout through Python
callbacks -- H sequential ``DynamicsFunc`` calls and one ``Constraint`` call per trajectory per iteration.  Here one
CEM iteration is two launches: ``sx_cem_rollout`` (all particles x all H steps: sampling, GP predict, reachability,
objective and constraint costs) and ``sx_cem_rank_refit`` (ranking, elite refit, best feasible sequence).

The loop semantics are this repository's specification (DESIGN.md "CEM specification"; the library's source is not
available, "parity unpinned"); what the reference's tests pin -- ``get_actions`` returns ``(actions [H x n_u] | None,
rollouts)``, an action-constraint cost of 3 per violating step, 10 per state outside the polytope -- is kept.
"""
import ctypes
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib, distributed
from .costs import SaturatingCost
from .gp_reachability_pytorch import raise_for_status, save_failure_state
from .ssm_cem.gp_ssm_cem import GpCemSSM


@dataclass
class Rollouts:
    """One CEM iteration's particles (what ``CemSafeMPC._plot_optimisation_process`` reads, safempc_cem.py:268-286)."""
    trajectories: Optional[Tensor]   # [P x H x (n_s + n_s^2)] flat states, or None when not recorded
    actions: Tensor                  # [P x H x n_u]
    objective_costs: Tensor          # [P]
    constraint_costs: Tensor         # [P]
    # with FusedCemMpc(perf_variance=True): the performance trajectory's means and posterior variances [P x n_perf x n_s]
    perf_trajectories: Optional[Tensor] = None
    perf_sigma: Optional[Tensor] = None
    # with FusedCemMpc(perf_type='taylor'): the propagated state covariances Sigma_1 .. Sigma_n_perf [P x n_perf x n_s x n_s]
    # (perf_sigma is then diag G_t, the variance including the uncertainty of the state)
    perf_cov: Optional[Tensor] = None


def _rollout(suffix: str, head: tuple, x0: Tensor, horizon: int, n_s: int, n_u: int, words: int, unsupported, *,
             actions, mean, std, noise, q0, want_traj, want_sigma, status, elite_rows, want_dist, workspace=()):
    """What `cem_rollout` and `cem_rollout_multi` share: the outputs, the `elite_rows` check and the launch of
    sx_cem_rollout[_elites]<suffix>(*head, E, P, H, x0, q0, mean, std | elite_rows, k, noise, <outputs>, status,
    *workspace | mean_out, std_out, stream).  `workspace`: (pointer, bytes) of the plain single-model entries; `words`: the
    size of a fresh status; `unsupported`: what SX_ERR_UNSUPPORTED raises."""
    dev = x0.device
    E = x0.size(0)
    if noise is not None:
        P = noise.size(1)
        actions = torch.empty((E, P, horizon, n_u), dtype=torch.float64, device=dev)
    else:
        P = actions.size(1)
        actions = actions.contiguous()
    S = n_s + n_s * n_s
    traj = torch.empty((E, P, horizon, S), dtype=torch.float64, device=dev) if want_traj else None
    sigma = torch.empty((E, P, horizon, n_s), dtype=torch.float64, device=dev) if want_sigma else None
    obj = torch.empty((E, P), dtype=torch.float64, device=dev)
    con = torch.empty((E, P), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(words, dtype=torch.int32, device=dev)
    out = dict(actions=actions, obj_cost=obj, con_cost=con, traj=traj, sigma=sigma, status=status)
    if elite_rows is not None:
        k = elite_rows.size(1)
        if noise is None or tuple(elite_rows.shape) != (E, k, 2 + horizon * n_u) or not elite_rows.is_contiguous():
            raise ValueError(f'elite_rows must be a contiguous [{E} x k x {2 + horizon * n_u}] tensor and come with noise')
        m_out = torch.empty((E, horizon, n_u), dtype=torch.float64, device=dev) if want_dist else None
        s_out = torch.empty((E, horizon, n_u), dtype=torch.float64, device=dev) if want_dist else None
        out.update(mean=m_out, std=s_out)
        if workspace:
            raise ValueError('the elite-row entries take no workspace')
        entry, dist, tail = 'sx_cem_rollout_elites' + suffix, (_lib.ptr(elite_rows), k), (_lib.ptr(m_out), _lib.ptr(s_out))
    else:
        entry, dist, tail = 'sx_cem_rollout' + suffix, (_lib.ptr(mean), _lib.ptr(std)), workspace
    code = getattr(_lib.lib(), entry)(*head, E, P, horizon, _lib.ptr(x0.contiguous()), _lib.ptr(q0), *dist, _lib.ptr(noise),
                                      _lib.ptr(actions), _lib.ptr(traj), _lib.ptr(sigma), _lib.ptr(obj), _lib.ptr(con),
                                      _lib.ptr(status), *tail, _lib.stream_ptr(dev))
    if unsupported is not None and code == _lib.SX_ERR_UNSUPPORTED:
        raise unsupported(f'{entry}: no single-launch form for the model')
    _lib.check(code, entry)
    return out


def cem_rollout(ssm: GpCemSSM, env: _lib.SxEnv, x0: Tensor, horizon: int, *, actions: Optional[Tensor] = None,
                mean: Optional[Tensor] = None, std: Optional[Tensor] = None, noise: Optional[Tensor] = None,
                q0: Optional[Tensor] = None, want_traj: bool = False, want_sigma: bool = False,
                status: Optional[Tensor] = None, elite_rows: Optional[Tensor] = None, want_dist: bool = False, cost=None,
                con_set=None):
    """Thin wrapper over sx_cem_rollout / sx_cem_rollout_elites (and their _junk, _feat and _mlp counterparts).

    x0 [E x n_s]; either `actions` [E x P x H x n_u] (given), or (`mean`, `std` [E x H x n_u], `noise` [E x P x H x n_u]),
    or (`elite_rows` [E x k x (2 + H n_u)], `noise`): the distribution is then refit from the previous iteration's elite
    rows in the rollout kernel's prologue (`fused_refit_applies`), and `mean` / `std` are not read; `want_dist` returns
    that refit as `mean` / `std`.
    `cost` (a `costs.SaturatingCost`; exact RBF GPs only) selects sx_cem_rollout_sat / sx_cem_rollout_elites_sat: obj_cost
    is the sum of the cost over the safety ellipsoids (p_t, Q_t), t = 1 .. H, read as means and covariances, env.obj_mode
    is not read and everything else is unchanged.  The streaming kernel only: a training set on
    the workspace path has no such launch.
    `con_set` (an `_lib.SxConSet`, `make_con_set`; exact RBF GPs only) selects sx_cem_rollout_cons /
    sx_cem_rollout_elites_cons, together with `cost` where given: con_cost then carries the feedback bounds on the control
    ellipsoids and the obstacle polytope on the intermediate safety ellipsoids, everything else is
    the launch's with the empty set.  The streaming kernel only, as with `cost`.
    Returns dict(actions, obj_cost [E x P], con_cost [E x P], traj | None, sigma | None, status int32[1]).
    """
    _lib.require_gpu(x0, 'x0')
    family = getattr(ssm, 'kernel_family', 'rbf')
    workspace, unsupported = (), None
    if con_set is not None:
        _require_exact_rbf([ssm], _CON_SET_IS)
        head = (ctypes.byref(ssm.device_model), ctypes.byref(env), _con_set_arg(con_set)) + (_cost_args(cost, ssm) or (None,))
        suffix = '_cons'
    elif cost is not None:
        _require_exact_rbf([ssm], _COST_IS)
        head, suffix = (ctypes.byref(ssm.device_model), ctypes.byref(env)) + _cost_args(cost, ssm), '_sat'
    elif family in ('feature', 'mlp', 'feature_junk', 'mlp_junk'):
        # 'feature': degenerate kernels ('linear', 'nn'), the weight-space rollout, one particle per lane (csrc/sx_feat.hpp);
        # 'mlp': MC-dropout ensembles over the frozen members, matrix cores for 1-2 hidden layers of <= 64 units
        # (csrc/sx_mlp_mfma.hpp), one particle per lane otherwise (csrc/sx_mlp.hpp).  Neither has an elite-row form.
        # JunkDimensionsSSM over one ('feature_junk', 'mlp_junk'): the _junk entries over the kept-column model
        # (`real_output_view`) with the query shift.
        junk = family.endswith('_junk')
        owner = ssm.real_output_view() if junk else ssm
        suffix, model = ('_feat', owner.feat_model) if family.startswith('feature') else ('_mlp', owner.mlp_model)
        head, elite_rows = (ctypes.byref(model), ctypes.byref(env)) + ((ssm.query_shift,) if junk else ()), None
        suffix += '_junk' if junk else ''
    else:
        # exact RBF GP ('rbf'); JunkDimensionsSSM over one ('rbf_junk') through the _junk entries: the real-output GP over
        # the kept columns (`real_output_view`) with the query shift.  That GP also owns the workspace.
        junk = family == 'rbf_junk'
        owner = ssm.real_output_view() if junk else ssm
        model, shift = owner.device_model, ssm.query_shift if junk else 0
        head = (ctypes.byref(model), ctypes.byref(env)) + ((shift,) if junk else ())
        suffix, unsupported = ('_junk', FusedJunkUnsupported) if junk else ('', None)
        if elite_rows is None:
            # (a query shift > 0 never takes a workspace)
            P = (actions if noise is None else noise).size(1)
            ws_bytes = (int(_lib.lib().sx_cem_rollout_workspace_bytes(ctypes.byref(model), x0.size(0), P, horizon))
                        if shift == 0 else 0)
            if ws_bytes < 0:
                raise _lib.SxError('sx_cem_rollout_workspace_bytes: bad arguments')
            workspace = (_lib.ptr(owner.workspace(ws_bytes)), ws_bytes)   # None on the fused path; cached on the model else
    return _rollout(suffix, head, x0, horizon, ssm.num_states, ssm.num_actions, 1, unsupported, actions=actions, mean=mean,
                    std=std, noise=noise, q0=q0, want_traj=want_traj, want_sigma=want_sigma, status=status,
                    elite_rows=elite_rows, want_dist=want_dist, workspace=workspace)


def _require_exact_rbf(ssms, what: str, numbered: bool = False) -> None:
    """NotImplementedError unless every model is an exact RBF GP.  `what`: the feature that needs one, with its verb ('the
    performance trajectory is'); `numbered`: the models are the solvers' of a multi-model solve, named by their index."""
    for i, ssm in enumerate(ssms):
        family = getattr(ssm, 'kernel_family', 'rbf')
        if family != 'rbf':
            raise NotImplementedError(f'{what} built for exact RBF GPs' + (f': solver {i} has' if numbered else ', not')
                                      + f' kernel_family {family!r} (feature-GP, MC-dropout, junk-dimension and step-by-step '
                                      f'models)')


# the features of the rollout wrappers that need one, as `_require_exact_rbf` names them
_COST_IS = 'the saturating cost on the safety trajectory is'
_CON_SET_IS = 'the constraint set (con_set: feedback bounds, obstacle polytope) is'
_STARTS_ARE = 'per-particle start states (static exploration) are'
_GAINS_ARE = 'per-particle, per-step feedback gains (multi-step reachability) are'


def _con_set_arg(con_set):
    """The sx_con_set pointer of a rollout entry's arguments."""
    if not isinstance(con_set, _lib.SxConSet):
        raise TypeError(f'con_set must be an _lib.SxConSet (make_con_set) or None, got {type(con_set).__name__}')
    return ctypes.byref(con_set)


def _checked_con_set(con_set, ssm):
    """`con_set` as the constructors of `FusedCemMpc` and `StaticCemMpc` keep it: None, or a set over an exact RBF GP."""
    if con_set is not None:
        _con_set_arg(con_set)
        _require_exact_rbf([ssm], _CON_SET_IS)
    return con_set


def _con_set_kw(con_set) -> dict:
    """The constraint set as the rollouts' keyword; empty without one, so that they are called as before."""
    return {} if con_set is None else dict(con_set=con_set)


def hook_objective(hook, means: Tensor, steps: int, n_s: int, like: Tensor) -> Tensor:
    """An objective hook (an ``Environment.objective_cost_function`` without a kernel form) summed over the recorded means
    [E x P x steps x n_s], step by step in that order: a contiguous tensor shaped `like`."""
    obj = torch.zeros_like(like)
    for t in range(steps):
        obj += hook(means[:, :, t].reshape(-1, n_s)).reshape(obj.shape)
    return obj.contiguous()


def split_flat_states(states: Tensor, n_s: int, device, episodes=None) -> Tuple[Tensor, Tensor]:
    """Flat start states [E x (n_s + n_s^2)] as (x0 [E x n_s] contiguous, the Q block [E x n_s^2]) in float64 on `device`.
    `episodes`: the E the caller wants (None: any); ValueError for another shape."""
    S = n_s + n_s * n_s
    if states.dim() != 2 or states.size(1) != S or episodes not in (None, states.size(0)):
        raise ValueError(f'Wanted shape ({"E" if episodes is None else episodes}, {S}), got {tuple(states.shape)}')
    states = states.to(device, torch.float64)
    return states[:, :n_s].contiguous(), states[:, n_s:]


def conset_eval(env: _lib.SxEnv, con_set, u: Tensor, q_start: Optional[Tensor], p_next: Optional[Tensor],
                q_next: Optional[Tensor], check_obstacle: bool = True) -> Tensor:
    """Thin wrapper over sx_conset_eval: [P], the constraint set's cost of one step of P particles -- the action cost (3)
    where u [P x n_u] leaves the box or, from an ellipsoid (., q_start [P x n_s x n_s]; None: a point) with the feedback
    bounds on, the control ellipsoid (u, K q_start K^T) is not certified inside it, plus (`check_obstacle`) the state cost
    (10) where (p_next [P x n_s], q_next [P x n_s x n_s]) is not certified inside the obstacle rows."""
    _lib.require_gpu(u, 'u')
    P, dev = u.size(0), u.device
    out = torch.empty(P, dtype=torch.float64, device=dev)
    c = lambda t: None if t is None else t.contiguous()
    _lib.check(_lib.lib().sx_conset_eval(ctypes.byref(env), _con_set_arg(con_set), P, _lib.ptr(c(u)), _lib.ptr(c(q_start)),
                                         _lib.ptr(c(p_next)), _lib.ptr(c(q_next)), int(bool(check_obstacle)), _lib.ptr(out),
                                         _lib.stream_ptr(dev)), 'sx_conset_eval')
    return out


def _starts_rollout(suffix: str, head, ssms: Sequence, horizon: int, words: int, unsupported, *, mean, std, noise, rows,
                    want_traj, want_sigma, status, con_set, gains=None, with_gains: bool = False):
    """What `cem_rollout_starts`, `cem_rollout_starts_multi` and `cem_rollout_gains` share: the checks of the rows, the
    outputs and the launch of
    sx_cem_rollout_starts[_cons]<suffix>(*head(E, dev)[, con_set], E, P, H, mean, std, noise, rows, <outputs>, status, stream)
    or, `with_gains`, of sx_cem_rollout_gains (the same arguments with `gains` behind `rows`).
    `head(E, dev)`: the entry's arguments in front of the set, made once the problem count and the device are known;
    `words`: the size of a fresh status (None: one word per problem); `unsupported`: what SX_ERR_UNSUPPORTED raises."""
    _require_exact_rbf(ssms, _GAINS_ARE if with_gains else _STARTS_ARE)
    cons = ()
    if con_set is not None:
        _require_exact_rbf(ssms, _CON_SET_IS)
        cons = (_con_set_arg(con_set),)
    entry = 'sx_cem_rollout_gains' if with_gains else 'sx_cem_rollout_starts' + ('_cons' if cons else '') + suffix
    n_s, n_u = ssms[0].num_states, ssms[0].num_actions
    L = n_s + horizon * n_u
    given = rows if noise is None else noise
    if (noise is None) == (rows is None) or given.dim() != 3 or given.size(2) != L or not given.is_contiguous():
        raise ValueError(f'either noise (the rows are drawn) or rows (given), a contiguous [E x P x {L}] tensor')
    _lib.require_gpu(given, 'rows' if noise is None else 'noise')
    E, P, dev = given.size(0), given.size(1), given.device
    head = head(E, dev)
    extra = ()
    if with_gains:
        shape = (E, P, horizon - 1, n_u, n_s)
        if horizon > 1 and (gains is None or tuple(gains.shape) != shape or not gains.is_contiguous()
                            or gains.dtype != torch.float64 or gains.device != dev):
            raise ValueError(f'gains must be a contiguous float64 [E x P x (H - 1) x n_u x n_s] = {shape} tensor on {dev}')
        extra = (_lib.ptr(gains if horizon > 1 else None),)
    if noise is not None:
        if mean is None or std is None or tuple(mean.shape) != (E, L) or tuple(std.shape) != (E, L):
            raise ValueError(f'noise needs the sampling distribution: mean and std [{E} x {L}]')
        mean, std = mean.contiguous(), std.contiguous()
        rows = torch.empty((E, P, L), dtype=torch.float64, device=dev)
    S = n_s + n_s * n_s
    traj = torch.empty((E, P, horizon, S), dtype=torch.float64, device=dev) if want_traj else None
    sigma = torch.empty((E, P, horizon, n_s), dtype=torch.float64, device=dev) if want_sigma else None
    obj = torch.empty((E, P), dtype=torch.float64, device=dev)
    con = torch.empty((E, P), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(E if words is None else words, dtype=torch.int32, device=dev)
    code = getattr(_lib.lib(), entry)(*head, *cons, E, P, horizon, _lib.ptr(mean if noise is not None else None),
                                      _lib.ptr(std if noise is not None else None), _lib.ptr(noise), _lib.ptr(rows),
                                      *extra, _lib.ptr(traj), _lib.ptr(sigma), _lib.ptr(obj), _lib.ptr(con), _lib.ptr(status),
                                      _lib.stream_ptr(dev))
    if unsupported is not None and code == _lib.SX_ERR_UNSUPPORTED:
        raise unsupported(f'{entry}: no single-launch form for the models')
    _lib.check(code, entry)
    return dict(rows=rows, obj_cost=obj, con_cost=con, traj=traj, sigma=sigma, status=status)


def cem_rollout_starts(ssm: GpCemSSM, env: _lib.SxEnv, horizon: int, *, mean: Optional[Tensor] = None,
                       std: Optional[Tensor] = None, noise: Optional[Tensor] = None, rows: Optional[Tensor] = None,
                       want_traj: bool = False, want_sigma: bool = False, status: Optional[Tensor] = None, con_set=None):
    """Thin wrapper over sx_cem_rollout_starts: the rollout whose particles each start from the first n_s entries of their
    own CEM row [x0 | actions], L = n_s + H n_u (static exploration).

    Either (`mean`, `std` [E x L], `noise` [E x P x L]): the rows are drawn, or `rows` [E x P x L] (given).
    Returns dict(rows, obj_cost [E x P], con_cost [E x P], traj | None, sigma | None, status int32[1]); a start outside the
    safe polytope has added SX_STATE_VIOLATION_COST to its particle's con_cost.
    `con_set` (an `_lib.SxConSet`, `make_con_set`) selects sx_cem_rollout_starts_cons: the feedback bounds from step 1 on,
    the obstacle rows on every intermediate ellipsoid, and SX_STATE_VIOLATION_COST once more for a start that violates the
    obstacle rows; everything but con_cost is the launch's without the set.
    """
    return _starts_rollout('', lambda E, dev: (ctypes.byref(ssm.device_model), ctypes.byref(env)), [ssm], horizon, 1, None,
                           mean=mean, std=std, noise=noise, rows=rows, want_traj=want_traj, want_sigma=want_sigma,
                           status=status, con_set=con_set)


class FusedGainsUnsupported(_lib.SxError):
    """sx_cem_rollout_gains answered SX_ERR_UNSUPPORTED (before any launch): propagate step by step."""


def cem_rollout_gains(ssm: GpCemSSM, env: _lib.SxEnv, horizon: int, *, gains: Optional[Tensor], mean: Optional[Tensor] = None,
                      std: Optional[Tensor] = None, noise: Optional[Tensor] = None, rows: Optional[Tensor] = None,
                      want_traj: bool = False, want_sigma: bool = False, status: Optional[Tensor] = None):
    """Thin wrapper over sx_cem_rollout_gains: `cem_rollout_starts` under a feedback gain per particle and step (multi-step
    reachability).  `gains` [E x P x (H - 1) x n_u x n_s]: K_t of step t = 1 .. H - 1 at index
    t - 1 (None allowed for H = 1); step 0 starts from the point of the row.  env.k_fb is not read.  Rows, outputs and costs
    as in `cem_rollout_starts`; SX_ERR_UNSUPPORTED raises `FusedGainsUnsupported`."""
    return _starts_rollout('', lambda E, dev: (ctypes.byref(ssm.device_model), ctypes.byref(env)), [ssm], horizon, 1,
                           FusedGainsUnsupported, mean=mean, std=std, noise=noise, rows=rows, want_traj=want_traj,
                           want_sigma=want_sigma, status=status, con_set=None, gains=gains, with_gains=True)


class FusedMultiUnsupported(_lib.SxError):
    """sx_cem_rollout_multi answered SX_ERR_UNSUPPORTED (before any launch): solve the problems one model at a time."""


# the families with a multi-model rollout: kernel_family -> (the model's struct attribute, its ctypes type, the C prefix of
# the table entries, the suffix of the rollout entry)
MULTI_FAMILIES = {'rbf': ('device_model', _lib.SxGpModel, 'sx_gp_model', '_multi'),
                  'feature': ('feat_model', _lib.SxFeatModel, 'sx_feat_model', '_feat_multi'),
                  'mlp': ('mlp_model', _lib.SxMlpModel, 'sx_mlp_model', '_mlp_multi')}


def multi_family(ssms: Sequence) -> Optional[str]:
    """The kernel_family all `ssms` share if it has a multi-model rollout ('rbf', 'feature', 'mlp'); None for mixed
    families, JunkDimensionsSSM ('*_junk') and 'stepwise' models."""
    families = {getattr(ssm, 'kernel_family', 'rbf') for ssm in ssms}
    family = families.pop() if len(families) == 1 else None
    return family if family in MULTI_FAMILIES else None


def model_array(ssms: Sequence, family: str):
    """The host array of the models' structs (sx_gp_model / sx_feat_model / sx_mlp_model) for the multi-model entries."""
    attr, ctype = MULTI_FAMILIES[family][:2]
    return (ctype * len(ssms))(*[getattr(ssm, attr) for ssm in ssms])


def model_table_bytes(array, family: str) -> int:
    """Bytes of the device table of these models; < 0 where one launch does not serve them (host only).  The exact GP's
    size depends on the shape alone; the feature-GP and MC-dropout tables also require one architecture."""
    lib, E = _lib.lib(), len(array)
    if family == 'rbf':
        n_s, n_u = array[0].n_s, array[0].n_u
        return int(lib.sx_gp_model_table_bytes(n_s, n_u, E))
    return int(getattr(lib, MULTI_FAMILIES[family][2] + '_table_bytes')(array, E))


class GpModelTable:
    """The device table of E models of one family (`family`: 'rbf' -- sx_gp_model_table, the default --, 'feature' --
    sx_feat_model_table -- or 'mlp' -- sx_mlp_model_table), rebuilt only when one of the models changes (the models build
    a new device_model / feat_model / mlp_model struct on every update).  `get` returns (the host array of the models,
    the device table)."""

    def __init__(self, family: str = 'rbf'):
        if family not in MULTI_FAMILIES:
            raise ValueError(f'no multi-model table for kernel_family {family!r}')
        self.family = family
        self._models = None
        self._array = None
        self._table = None

    def get(self, ssms: Sequence[GpCemSSM], dev):
        attr = MULTI_FAMILIES[self.family][0]
        models = [getattr(ssm, attr) for ssm in ssms]
        if (self._models is not None and len(models) == len(self._models) and self._table.device == dev
                and all(a is b for a, b in zip(models, self._models))):
            return self._array, self._table
        lib, E = _lib.lib(), len(models)
        n_s, n_u = models[0].n_s, models[0].n_u
        if any((m.n_s, m.n_u) != (n_s, n_u) for m in models):
            raise ValueError(f'the models of a multi-model rollout must share (n_s, n_u); got '
                             f'{[(m.n_s, m.n_u) for m in models]}')
        array = model_array(ssms, self.family)
        nbytes = model_table_bytes(array, self.family)
        if nbytes < 0:
            raise FusedMultiUnsupported(f'{MULTI_FAMILIES[self.family][2]}_table_bytes: no single launch for these models '
                                        f'((n_s, n_u) = ({n_s}, {n_u}) without a rollout kernel, or differing '
                                        f'architectures)')
        table = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        entry = MULTI_FAMILIES[self.family][2] + '_table'
        _lib.check(getattr(lib, entry)(array, E, _lib.ptr(table), _lib.stream_ptr(dev)), entry)
        self._models, self._array, self._table = models, array, table
        return array, table


def cem_rollout_multi(ssms: Sequence[GpCemSSM], env: _lib.SxEnv, x0: Tensor, horizon: int, *,
                      actions: Optional[Tensor] = None, mean: Optional[Tensor] = None, std: Optional[Tensor] = None,
                      noise: Optional[Tensor] = None, q0: Optional[Tensor] = None, want_traj: bool = False,
                      want_sigma: bool = False, status: Optional[Tensor] = None, elite_rows: Optional[Tensor] = None,
                      want_dist: bool = False, table: Optional[GpModelTable] = None, cost=None, con_set=None):
    """`cem_rollout` for E problems with a model each (ssms[e] for problem e), one launch.  The models share one
    kernel_family: exact RBF GPs ('rbf': sx_cem_rollout_multi / sx_cem_rollout_elites_multi), feature-space GPs
    ('feature': sx_cem_rollout_feat_multi) or MC-dropout ensembles ('mlp': sx_cem_rollout_mlp_multi; neither of the last
    two has an elite-row form).  Buffers as in `cem_rollout`; `status` is int32 [E], one word per problem.  `table` keeps
    the device table of the models between calls (a fresh one is built otherwise, as where it belongs to another family).
    `cost` as in `cem_rollout` (sx_cem_rollout_sat_multi / sx_cem_rollout_elites_sat_multi; exact RBF GPs only).
    `con_set` as in `cem_rollout`: ONE set for all problems, as they share `env` (sx_cem_rollout_cons_multi /
    sx_cem_rollout_elites_cons_multi, together with `cost` where given; exact RBF GPs only).
    Raises FusedMultiUnsupported where the library has no single launch for the models (before any launch): mixed
    families, JunkDimensionsSSM and step-by-step models, differing architectures, a shape without a kernel."""
    if con_set is not None:
        _require_exact_rbf(ssms, _CON_SET_IS)
    if cost is not None:
        _require_exact_rbf(ssms, _COST_IS)
    family = multi_family(ssms)
    if family is None:
        raise FusedMultiUnsupported('the multi-model rollout takes models of one kernel_family: "rbf", "feature" or "mlp"; '
                                    f'got {[getattr(ssm, "kernel_family", "rbf") for ssm in ssms]}')
    if family != 'rbf' and elite_rows is not None:
        raise ValueError(f'the {family!r} family has no elite-row form of the multi-model rollout')
    _lib.require_gpu(x0, 'x0')
    E = x0.size(0)
    if len(ssms) != E:
        raise ValueError(f'{len(ssms)} models for {E} problems')
    if status is not None and status.numel() != E:
        raise ValueError(f'status must hold one word per problem ({E}), got {status.numel()}')
    if table is None or table.family != family:
        table = GpModelTable(family)
    models, tab = table.get(ssms, x0.device)
    head = (models, _lib.ptr(tab), ctypes.byref(env))
    if con_set is not None:
        head += (_con_set_arg(con_set),) + (_cost_args(cost, ssms[0]) or (None,))
        suffix = '_cons'
    else:
        if cost is not None:
            head += _cost_args(cost, ssms[0])
        suffix = '_sat' if cost is not None else ''
    return _rollout(suffix + MULTI_FAMILIES[family][3], head, x0, horizon,
                    ssms[0].num_states, ssms[0].num_actions, E, FusedMultiUnsupported, actions=actions, mean=mean, std=std,
                    noise=noise, q0=q0, want_traj=want_traj, want_sigma=want_sigma, status=status, elite_rows=elite_rows,
                    want_dist=want_dist)


def cem_rollout_starts_multi(ssms: Sequence[GpCemSSM], env: _lib.SxEnv, horizon: int, *, mean: Optional[Tensor] = None,
                             std: Optional[Tensor] = None, noise: Optional[Tensor] = None, rows: Optional[Tensor] = None,
                             want_traj: bool = False, want_sigma: bool = False, status: Optional[Tensor] = None,
                             table: Optional[GpModelTable] = None, con_set=None):
    """`cem_rollout_starts` for E problems with an exact RBF GP each (ssms[e] for problem e; a scenario with R restarts
    stands R times in the list), one launch: sx_cem_rollout_starts_multi, with `con_set` (ONE set for all problems)
    sx_cem_rollout_starts_cons_multi.  Buffers as in `cem_rollout_starts` (`mean`, `std` [E x L]: a start distribution per
    problem); `status` is int32 [E], one word per problem.  `table` keeps the device table of the models between calls.
    Raises FusedMultiUnsupported where the library has no single launch for the models (before any launch)."""
    if table is None or table.family != 'rbf':
        table = GpModelTable()      # (it owns the device table: held here until the launch is enqueued)

    def head(E, dev):
        if len(ssms) != E:
            raise ValueError(f'{len(ssms)} models for {E} problems')
        if status is not None and status.numel() != E:
            raise ValueError(f'status must hold one word per problem ({E}), got {status.numel()}')
        models, tab = table.get(ssms, dev)
        return models, _lib.ptr(tab), ctypes.byref(env)
    return _starts_rollout('_multi', head, ssms, horizon, None, FusedMultiUnsupported, mean=mean, std=std, noise=noise,
                           rows=rows, want_traj=want_traj, want_sigma=want_sigma, status=status, con_set=con_set)


class FusedJunkUnsupported(_lib.SxError):
    """sx_cem_rollout_junk answered SX_ERR_UNSUPPORTED (before any launch): the solve goes step by step."""


def _require_rbf(ssms: Sequence, x0: Tensor) -> None:
    _lib.require_gpu(x0, 'x0')
    _require_exact_rbf(ssms, 'the performance trajectory is')


def _perf_rollout(entry: str, head: tuple, ssms: Sequence, x0: Tensor, horizon: int, n_perf: int, r: int, *, safe_actions,
                  obj_cost, con_cost, status, tail_mean, tail_std, tail_noise, rows, want_traj, want_sigma=None,
                  unsupported=None, want_cov=None, terminal_safety=False):
    """What `cem_perf_rollout`, `cem_perf_rollout_var`, `cem_perf_rollout_taylor` and their multi-model forms share
    (after `_require_rbf`): the buffers and the launch of `entry`(*head, E, P, H, n_perf, r, x0, safe_actions, tail_mean,
    tail_std, tail_noise, rows, obj_cost, con_cost, perf_traj[, perf_sigma[, perf_cov, terminal_safety]], status, stream).
    `want_sigma` is None for the mean-only entries (no perf_sigma argument), `want_cov` is None for all but the Taylor entries
    (no perf_cov / terminal_safety arguments); `unsupported(n_s, n_u)`: what SX_ERR_UNSUPPORTED raises, where the entry has
    a message of its own."""
    dev, n_s, n_u = x0.device, ssms[0].num_states, ssms[0].num_actions
    E, P = safe_actions.size(0), safe_actions.size(1)
    T = n_perf - r
    if tail_noise is not None:
        if rows is not None:
            raise ValueError('either tail_noise (the tail is drawn) or rows (the tail is given), not both')
        rows = torch.empty((E, P, horizon + T, n_u), dtype=torch.float64, device=dev)
    elif rows is None or tuple(rows.shape) != (E, P, horizon + T, n_u) or not rows.is_contiguous():
        raise ValueError(f'without tail_noise, rows must be a contiguous [{E} x {P} x {horizon + T} x {n_u}] tensor')
    traj = torch.empty((E, P, n_perf, n_s), dtype=torch.float64, device=dev) if want_traj else None
    sigma = torch.empty((E, P, n_perf, n_s), dtype=torch.float64, device=dev) if want_sigma else None
    outs = (_lib.ptr(traj),) + (() if want_sigma is None else (_lib.ptr(sigma),))
    cov = torch.empty((E, P, n_perf, n_s, n_s), dtype=torch.float64, device=dev) if want_cov else None
    if want_cov is not None:
        outs += (_lib.ptr(cov), int(bool(terminal_safety)))
    code = getattr(_lib.lib(), entry)(*head, E, P, horizon, n_perf, r, _lib.ptr(x0.contiguous()), _lib.ptr(safe_actions),
                                      _lib.ptr(tail_mean), _lib.ptr(tail_std), _lib.ptr(tail_noise), _lib.ptr(rows),
                                      _lib.ptr(obj_cost), _lib.ptr(con_cost), *outs, _lib.ptr(status), _lib.stream_ptr(dev))
    if unsupported is not None and code == _lib.SX_ERR_UNSUPPORTED:
        raise unsupported(n_s, n_u)
    _lib.check(code, entry)
    out = dict(rows=rows, obj_cost=obj_cost, con_cost=con_cost, perf_traj=traj, status=status)
    if want_sigma is not None:
        out['perf_sigma'] = sigma
    if want_cov is not None:
        out['perf_cov'] = cov
    return out


def cem_perf_rollout(ssm: GpCemSSM, env: _lib.SxEnv, x0: Tensor, horizon: int, n_perf: int, r: int, *,
                     safe_actions: Tensor, obj_cost: Tensor, con_cost: Tensor, status: Tensor,
                     tail_mean: Optional[Tensor] = None, tail_std: Optional[Tensor] = None,
                     tail_noise: Optional[Tensor] = None, rows: Optional[Tensor] = None, want_traj: bool = False):
    """Thin wrapper over sx_cem_perf_rollout: the performance trajectory of the particles of a safety rollout (exact RBF
    GPs only).  x0 [E x n_s]; `safe_actions` [E x P x H x n_u], `obj_cost` (overwritten) and `con_cost` (added to) [E x P]
    as `cem_rollout` returned them; the tail either drawn (`tail_mean`, `tail_std` [E x T x n_u], `tail_noise`
    [E x P x T x n_u], T = n_perf - r) or given as the tail of `rows` [E x P x (H + T) x n_u].
    Returns dict(rows, obj_cost, con_cost, perf_traj [E x P x n_perf x n_s] | None, status)."""
    _require_rbf([ssm], x0)
    head = (ctypes.byref(ssm.device_model), _lib.ptr(ssm._alpha), ctypes.byref(env))
    return _perf_rollout('sx_cem_perf_rollout', head, [ssm], x0, horizon, n_perf, r, safe_actions=safe_actions,
                         obj_cost=obj_cost, con_cost=con_cost, status=status, tail_mean=tail_mean, tail_std=tail_std,
                         tail_noise=tail_noise, rows=rows, want_traj=want_traj)


def _no_form(entry: str, what: str, ssm, n_perf: int):
    """What SX_ERR_UNSUPPORTED raises from the single-model entry of a GP-product form, as `_perf_rollout` calls it."""
    return lambda n_s, n_u: _lib.SxError(
        f'{entry}: no form of the {what} performance rollout for this model ((n_s, n_u) = ({n_s}, {n_u}), N = '
        f'{ssm.device_model.n_train}, n_perf = {n_perf}): it runs with Kstar in LDS, all outputs at once or output by output '
        f'(n_pad <= 1024), and has no workspace path')


def cem_perf_rollout_var(ssm: GpCemSSM, env: _lib.SxEnv, x0: Tensor, horizon: int, n_perf: int, r: int, *,
                         safe_actions: Tensor, obj_cost: Tensor, con_cost: Tensor, status: Tensor,
                         tail_mean: Optional[Tensor] = None, tail_std: Optional[Tensor] = None,
                         tail_noise: Optional[Tensor] = None, rows: Optional[Tensor] = None, want_traj: bool = False,
                         want_sigma: bool = False):
    """Thin wrapper over sx_cem_perf_rollout_var: `cem_perf_rollout` with the GP's posterior variance at every step (the
    N x N product of the safety kernels), for both objective modes -- SX_OBJ_NEG_VARIANCE sums -var_t over the performance
    trajectory.  Arguments as `cem_perf_rollout`; `want_sigma` also returns the variances.
    Returns dict(rows, obj_cost, con_cost, perf_traj [E x P x n_perf x n_s] | None, perf_sigma (same shape) | None,
    status)."""
    _require_rbf([ssm], x0)
    head = (ctypes.byref(ssm.device_model), ctypes.byref(env))
    return _perf_rollout('sx_cem_perf_rollout_var', head, [ssm], x0, horizon, n_perf, r, safe_actions=safe_actions,
                         obj_cost=obj_cost, con_cost=con_cost, status=status, tail_mean=tail_mean, tail_std=tail_std,
                         tail_noise=tail_noise, rows=rows, want_traj=want_traj, want_sigma=bool(want_sigma),
                         unsupported=_no_form('sx_cem_perf_rollout_var', 'variance', ssm, n_perf))


PERF_TYPES = ('mean_equivalent', 'taylor')


class PerfNames(NamedTuple):
    """How a message of `PerfSpec.checked` spells the five settings and the horizon: what the caller's user typed."""
    n_perf: str
    r: str
    variance: str
    type: str
    terminal_safety: str
    horizon: str
    range_last: bool = False    # the rule on (n_perf, r) is tested behind the others, not in front of them


KEYWORD_NAMES = PerfNames('n_perf', 'perf_r', 'perf_variance', 'perf_type', 'perf_terminal_safety', 'time_horizon')
CONF_NAMES = PerfNames('cem_n_perf', 'cem_perf_r', 'cem_perf_variance', 'cem_perf_type', 'cem_perf_terminal_safety',
                       'mpc_time_horizon', range_last=True)


class PerfSpec(NamedTuple):
    """Does a solve have a performance trajectory, and which one: `n_perf` steps (0: none) that share
    their first `r` actions with the safety trajectory; `variance`: they carry the GP's posterior variance; `type`: one of
    PERF_TYPES; `terminal_safety`: the 'taylor' ellipsoid at step H + 2 must lie in the safe polytope."""
    n_perf: int = 0
    r: int = 1
    variance: bool = False
    type: str = 'mean_equivalent'
    terminal_safety: bool = False

    @property
    def on(self) -> bool:
        return self.n_perf > 0

    @property
    def kind(self) -> Optional[str]:
        """The performance rollout: 'mean' (sx_cem_perf_rollout[_multi]), 'variance' (sx_cem_perf_rollout_var[_multi]) or
        'taylor' (sx_cem_perf_rollout_taylor[_multi]; it carries the variance by itself); None without a trajectory."""
        if not self.on:
            return None
        return 'taylor' if self.type == 'taylor' else 'variance' if self.variance else 'mean'

    @property
    def tail(self) -> int:
        """T: the steps of a CEM row behind the H safety steps."""
        return self.n_perf - self.r if self.on else 0

    def row_steps(self, horizon: int) -> int:
        return horizon + self.tail

    def keywords(self) -> dict:
        """The spec as `FusedCemMpc`'s keywords: n_perf, perf_r, and of the other three those that are not the default."""
        return {k: v for k, v, d in zip(KEYWORD_NAMES, self, PERF_OFF) if v != d or k in ('n_perf', 'perf_r')}

    def checked(self, horizon: int, *, names: PerfNames = KEYWORD_NAMES) -> 'PerfSpec':
        """THE validation of the five settings against the safety horizon: the spec with its fields as int / bool, or
        ValueError naming the setting as `names` spells it."""
        s = PerfSpec(int(self.n_perf), int(self.r), bool(self.variance), self.type, bool(self.terminal_safety))
        n, taylor = names, self.type == 'taylor'
        rules = [
            (s.n_perf < 0 or (s.on and not (1 <= s.r <= horizon and s.n_perf > s.r)),
             f'a performance trajectory needs 1 <= {n.r} <= {n.horizon} and {n.n_perf} > {n.r}, got {n.n_perf}={s.n_perf}, '
             f'{n.r}={s.r}, {n.horizon}={horizon}'),
            (s.variance and not s.on, f'{n.variance}=True needs a performance trajectory ({n.n_perf} > 0)'),
            (s.type not in PERF_TYPES, f'{n.type} must be one of {PERF_TYPES}, got {s.type!r}'),
            (taylor and not s.on, f"{n.type}='taylor' needs a performance trajectory ({n.n_perf} > 0)"),
            (s.terminal_safety and not taylor, f"{n.terminal_safety} needs the propagated covariance ({n.type}='taylor')"),
            (s.terminal_safety and s.n_perf < horizon + 2,
             f'{n.terminal_safety} checks the performance state {n.horizon} + 2 = {horizon + 2}: {n.n_perf}={s.n_perf} is too '
             f'short ({n.n_perf} >= {n.horizon} + 2)')]
        if n.range_last:
            rules.append(rules.pop(0))
        for failed, message in rules:
            if failed:
                raise ValueError(message)
        return s


PERF_OFF = PerfSpec()


def perf_spec_of(solver) -> PerfSpec:
    """A solver's spec; the off spec for an object that carries none (an injected optimiser, a stand-in built without the
    constructor).  The one place where the five settings have a default."""
    spec = getattr(solver, '_perf', None)
    return spec if isinstance(spec, PerfSpec) else PERF_OFF


def _cost_args(cost, ssm) -> tuple:
    """What a `cost` adds to the arguments of a rollout entry behind `env`: nothing, or its sx_sat_cost (for `ssm`'s states)."""
    if cost is None:
        return ()
    if not isinstance(cost, SaturatingCost):
        raise TypeError(f'cost must be a costs.SaturatingCost or None, got {type(cost).__name__}')
    n_s = ssm.num_states
    if cost.n_s != n_s:
        raise ValueError(f'the cost is built for n_s = {cost.n_s}, the model has n_s = {n_s}')
    return (ctypes.byref(cost.struct),)


def cem_perf_rollout_taylor(ssm: GpCemSSM, env: _lib.SxEnv, x0: Tensor, horizon: int, n_perf: int, r: int, *,
                            safe_actions: Tensor, obj_cost: Tensor, con_cost: Tensor, status: Tensor,
                            tail_mean: Optional[Tensor] = None, tail_std: Optional[Tensor] = None,
                            tail_noise: Optional[Tensor] = None, rows: Optional[Tensor] = None, want_traj: bool = False,
                            want_sigma: bool = False, want_cov: bool = False, terminal_safety: bool = False, cost=None):
    """Thin wrapper over sx_cem_perf_rollout_taylor: `cem_perf_rollout_var` with the state covariance propagated to first
    order under the fixed feedback `env.k_fb` -- Sigma_{t+1} = H Sigma_t H^T + diag(var_t), and the objective sees
    diag(G_t) = var_t + diag(M Sigma_t M^T).  Arguments as `cem_perf_rollout_var`; `want_sigma` returns diag(G_t), `want_cov`
    Sigma_1 .. Sigma_{n_perf} [E x P x n_perf x n_s x n_s]; `terminal_safety` adds the state-violation cost where the
    ellipsoid (mu_s, Sigma_s), s = horizon + 2, leaves the safe polytope (needs n_perf >= horizon + 2).  `cost` (a
    `costs.SaturatingCost`) selects sx_cem_perf_rollout_taylor_sat: obj_cost is the sum of the cost over (mu_{t+1},
    Sigma_{t+1}) and env.obj_mode is not read; everything else is unchanged.
    Returns dict(rows, obj_cost, con_cost, perf_traj | None, perf_sigma | None, perf_cov | None, status)."""
    _require_rbf([ssm], x0)
    _check_terminal_safety(terminal_safety, n_perf, horizon)
    head = (ctypes.byref(ssm.device_model), ctypes.byref(env)) + _cost_args(cost, ssm)
    entry = 'sx_cem_perf_rollout_taylor' + ('_sat' if cost is not None else '')
    return _perf_rollout(entry, head, [ssm], x0, horizon, n_perf, r, safe_actions=safe_actions,
                         obj_cost=obj_cost, con_cost=con_cost, status=status, tail_mean=tail_mean, tail_std=tail_std,
                         tail_noise=tail_noise, rows=rows, want_traj=want_traj, want_sigma=bool(want_sigma),
                         unsupported=_no_form('sx_cem_perf_rollout_taylor', 'Taylor', ssm, n_perf), want_cov=bool(want_cov),
                         terminal_safety=terminal_safety)


class PerfModelTable:
    """The device table of sx_cem_perf_table for E exact GPs -- their kernel constants, training inputs and alpha, what the
    mean-only performance rollout reads --, kept like `GpModelTable` and rebuilt only when one of the models changes (a
    model builds a new device_model struct, and a new alpha, on every update).  `get` returns (the host array of the
    models, the device table)."""

    def __init__(self):
        self._models = None
        self._alphas = None
        self._array = None
        self._table = None

    def get(self, ssms: Sequence[GpCemSSM], dev):
        models, alphas = [ssm.device_model for ssm in ssms], [ssm._alpha for ssm in ssms]
        if (self._models is not None and len(models) == len(self._models) and self._table.device == dev
                and all(a is b for a, b in zip(models, self._models))
                and all(a is b for a, b in zip(alphas, self._alphas))):
            return self._array, self._table
        lib, E = _lib.lib(), len(models)
        n_s, n_u = models[0].n_s, models[0].n_u
        if any((m.n_s, m.n_u) != (n_s, n_u) for m in models):
            raise ValueError(f'the models of a multi-model rollout must share (n_s, n_u); got '
                             f'{[(m.n_s, m.n_u) for m in models]}')
        array = model_array(ssms, 'rbf')
        nbytes = int(lib.sx_cem_perf_table_bytes(n_s, n_u, E))
        if nbytes < 0:
            raise FusedMultiUnsupported(f'sx_cem_perf_table_bytes: (n_s, n_u) = ({n_s}, {n_u}) has no performance rollout')
        table = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        ptrs = (ctypes.c_void_p * E)(*[_lib.ptr(a) for a in alphas])
        _lib.check(lib.sx_cem_perf_table(array, ptrs, E, _lib.ptr(table), _lib.stream_ptr(dev)), 'sx_cem_perf_table')
        self._models, self._alphas, self._array, self._table = models, alphas, array, table
        return array, table


def _check_terminal_safety(terminal_safety: bool, n_perf: int, horizon: int) -> None:
    if terminal_safety and n_perf < horizon + 2:
        raise ValueError(f'terminal_safety checks the performance state {horizon + 2}: n_perf = {n_perf} is too short '
                         f'(n_perf >= horizon + 2)')


def _perf_multi_preamble(entry: str, what: str, ssms: Sequence, x0: Tensor, n_perf: int, status, table, want, *,
                         terminal_safety: bool = False, horizon: int = 0):
    """What the multi-model performance wrappers do before `_perf_rollout`: the checks (the Taylor form's on
    `terminal_safety` among them), the device table (`table` if it is a `want` for exact GPs, else a fresh one) and what
    SX_ERR_UNSUPPORTED raises.  Returns (the models, the device table, unsupported); the caller holds the table's tensor
    until its launch is enqueued (a fresh table has no other owner)."""
    _require_rbf(ssms, x0)
    E = x0.size(0)
    if len(ssms) != E:
        raise ValueError(f'{len(ssms)} models for {E} problems')
    if status is not None and status.numel() != E:
        raise ValueError(f'status must hold one word per problem ({E}), got {status.numel()}')
    _check_terminal_safety(terminal_safety, n_perf, horizon)
    if not isinstance(table, want) or getattr(table, 'family', 'rbf') != 'rbf':
        table = want()
    models, dev_table = table.get(ssms, x0.device)

    def unsupported(n_s, n_u):
        return FusedMultiUnsupported(f'{entry}: no single launch of the {what} for these models ((n_s, n_u) = '
                                     f'({n_s}, {n_u}), N = {[ssm.device_model.n_train for ssm in ssms]}, n_perf = {n_perf})')
    return models, dev_table, unsupported


def cem_perf_rollout_multi(ssms: Sequence[GpCemSSM], env: _lib.SxEnv, x0: Tensor, horizon: int, n_perf: int, r: int, *,
                           variance: bool = False, safe_actions: Tensor, obj_cost: Tensor, con_cost: Tensor, status: Tensor,
                           tail_mean: Optional[Tensor] = None, tail_std: Optional[Tensor] = None,
                           tail_noise: Optional[Tensor] = None, rows: Optional[Tensor] = None, want_traj: bool = False,
                           want_sigma: bool = False, table=None):
    """`cem_perf_rollout` (`variance=False`: sx_cem_perf_rollout_multi) or `cem_perf_rollout_var` (`variance=True`:
    sx_cem_perf_rollout_var_multi) for E problems with an exact GP each (ssms[e] for problem e) in one launch.  Buffers as
    in the single-model wrappers, per problem; `status` is int32 [E], one word per problem.  `table` keeps the device table
    between calls: a `PerfModelTable` for the mean-only form, the `GpModelTable` of `cem_rollout_multi` for the variance
    form (a fresh one is built otherwise).  Raises FusedMultiUnsupported where the library has no single launch for the
    models (before any launch)."""
    entry = 'sx_cem_perf_rollout_var_multi' if variance else 'sx_cem_perf_rollout_multi'
    models, dev_table, unsupported = _perf_multi_preamble(entry, 'performance rollout', ssms, x0, n_perf, status, table,
                                                          GpModelTable if variance else PerfModelTable)
    return _perf_rollout(entry, (models, _lib.ptr(dev_table), ctypes.byref(env)), ssms, x0, horizon, n_perf, r, safe_actions=safe_actions,
                         obj_cost=obj_cost, con_cost=con_cost, status=status, tail_mean=tail_mean, tail_std=tail_std,
                         tail_noise=tail_noise, rows=rows, want_traj=want_traj,
                         want_sigma=bool(want_sigma) if variance else None, unsupported=unsupported)


def cem_perf_rollout_taylor_multi(ssms: Sequence[GpCemSSM], env: _lib.SxEnv, x0: Tensor, horizon: int, n_perf: int, r: int,
                                  *, safe_actions: Tensor, obj_cost: Tensor, con_cost: Tensor, status: Tensor,
                                  tail_mean: Optional[Tensor] = None, tail_std: Optional[Tensor] = None,
                                  tail_noise: Optional[Tensor] = None, rows: Optional[Tensor] = None,
                                  want_traj: bool = False, want_sigma: bool = False, want_cov: bool = False,
                                  terminal_safety: bool = False, table=None, cost=None):
    """`cem_perf_rollout_taylor` for E problems with an exact GP each (ssms[e] for problem e) in one launch
    (sx_cem_perf_rollout_taylor_multi).  There is one `env`: the feedback gain, the safe polytope and the terminal-safety
    step are the same for all problems.  Buffers as in the single-model wrapper, per problem; `status` is int32 [E], one
    word per problem.  `table` keeps the device table between calls: the `GpModelTable` of `cem_rollout_multi` (a fresh
    one is built otherwise).  `cost` selects sx_cem_perf_rollout_taylor_sat_multi, as in the single-model wrapper.  Raises
    FusedMultiUnsupported where the library has no single launch for the models (before any launch)."""
    entry = 'sx_cem_perf_rollout_taylor_sat_multi' if cost is not None else 'sx_cem_perf_rollout_taylor_multi'
    models, dev_table, unsupported = _perf_multi_preamble(entry, "'taylor' performance rollout", ssms, x0, n_perf, status,
                                                          table, GpModelTable, terminal_safety=terminal_safety,
                                                          horizon=horizon)
    head = (models, _lib.ptr(dev_table), ctypes.byref(env)) + _cost_args(cost, ssms[0])
    return _perf_rollout(entry, head, ssms, x0, horizon, n_perf, r, safe_actions=safe_actions,
                         obj_cost=obj_cost, con_cost=con_cost, status=status, tail_mean=tail_mean, tail_std=tail_std,
                         tail_noise=tail_noise, rows=rows, want_traj=want_traj, want_sigma=bool(want_sigma),
                         unsupported=unsupported, want_cov=bool(want_cov), terminal_safety=terminal_safety)


def _launch_perf(perf: PerfSpec, ssms: Sequence, env: _lib.SxEnv, x0: Tensor, horizon: int, safety: dict, mean: Tensor,
                 std: Tensor, tail_noise: Tensor, status: Tensor, *, multi: bool = False, want_traj: bool = False,
                 record: bool = False, table=None, cost=None):
    """The one performance launch of a CEM iteration, for `FusedCemMpc.solve` (ssms = [the model]) and
    `MultiModelPerfCemMpc.solve` (`multi`: a model per problem, and the solver's `table` for the kind): the rollout of
    `perf.kind` behind the safety rollout's result `safety`, its tail drawn from the columns past `horizon` of the
    full-row `mean` / `std` with `tail_noise`.  `want_traj` asks for the means; `record` for all the variance and Taylor
    forms carry (means, variances, covariances).  A multi-model solve asks for neither.  `cost` (Taylor only): the
    saturating cost as the kernel's objective.  The wrappers are looked up on the module when called.  Returns the
    wrapper's dict."""
    kind = perf.kind
    kw = dict(safe_actions=safety['actions'], obj_cost=safety['obj_cost'].contiguous(),
              con_cost=safety['con_cost'].contiguous(), status=status, tail_mean=mean[:, horizon:].contiguous(),
              tail_std=std[:, horizon:].contiguous(), tail_noise=tail_noise)
    if multi:
        kw.update(table=table, **({} if kind == 'taylor' else dict(variance=kind == 'variance')))
    elif kind == 'mean':
        kw.update(want_traj=want_traj)
    else:
        kw.update(want_traj=want_traj or record, want_sigma=record, **(dict(want_cov=record) if kind == 'taylor' else {}))
    if kind == 'taylor':
        kw.update(terminal_safety=perf.terminal_safety, **({} if cost is None else dict(cost=cost)))
    name = 'cem_perf_rollout' + {'mean': '', 'variance': '_var', 'taylor': '_taylor'}[kind]
    if multi:
        name = 'cem_perf_rollout_taylor_multi' if kind == 'taylor' else 'cem_perf_rollout_multi'
    return globals()[name](ssms if multi else ssms[0], env, x0, horizon, perf.n_perf, perf.r, **kw)


def fused_refit_applies(ssm, episodes: int, particles: int, horizon: int, candidates: Optional[int] = None) -> bool:
    """May the elite refit move from the ranking kernel's tail into the next rollout's prologue (sx_cem_rollout_elites)?
    Exact-GP models on the single-launch path whose H n_u means and standard deviations fit the prologue's scratch, where
    the ranking that produces the rows (over `candidates` rows per problem; default: the particles) is the counting one.
    (JunkDimensionsSSM over an exact GP, 'rbf_junk': the same for its real-output GP, sx_cem_rollout_elites_junk.)
    The feature-GP and MC-dropout families, 'feature_junk' and 'mlp_junk' included, have no elite-row form: False."""
    family = getattr(ssm, 'kernel_family', 'rbf')
    if family not in ('rbf', 'rbf_junk'):
        return False
    if 2 * horizon * ssm.num_actions > 256 * (1 + ssm.num_states):   # the bound of plan_rollout (csrc/sx_gp_rollout.hip)
        return False
    lib = _lib.lib()
    model = ssm.real_output_view().device_model if family == 'rbf_junk' else ssm.device_model
    if int(lib.sx_cem_rollout_workspace_bytes(ctypes.byref(model), episodes, particles, horizon)) != 0:
        return False
    # worth it where the ranking spreads over the chip and its refit would be a serial tail; many problems at once
    # (config 5: 8 episodes per GPU) rank and refit side by side, one workgroup each
    return int(lib.sx_cem_rank_counts(episodes, particles if candidates is None else candidates)) == 1


def cem_rollout_stepwise(ssm: GpCemSSM, env: _lib.SxEnv, x0: Tensor, actions: Tensor, *, status: Tensor, group=None,
                         objective_hook=None, cost=None, con_set=None):
    """The rollout of ONE problem step by step, the way the reference's optimiser drives it: H dynamics-callback calls on
    the whole particle batch (safempc_cem.py:288-302), each = sx_gp_predict + sx_onestep_reach, then the costs.

    This is the path that keeps the reference's WHOLE-BATCH zero fix-up (gp_reachability_pytorch.py:234-243: an exact
    zero variance anywhere in the batch also lifts the negative ones), which the fused kernel cannot see across its
    workgroups.  `FusedCemMpc` falls back to it when a fused solve reports both SX_STATUS_NAN and SX_STATUS_ZERO_FIX --
    the only case in which the two rules can differ.  ~3 H launches per iteration instead of one; nothing synchronises.

    x0 [n_s], or [P x n_s]: a start per particle (`StaticCemMpc`; the cost of a start outside the polytope is
    `start_constraint_cost`, not part of this rollout); actions [P x H x n_u] (this rank's particles); with a process group the batch spans the ranks: the
    "zero present" flag is all-reduced (MAX) per step.  Returns dict(obj_cost [P], con_cost [P]); `status` is OR-ed.
    `cost` (a `costs.SaturatingCost`): the objective of a step is the cost of its ellipsoid (p_{t+1}, Q_{t+1}) through
    sx_sat_cost_eval -- one more launch per step, in place of the hook and env.obj_mode -- as sx_cem_rollout_sat prices it.
    `con_set` (an `_lib.SxConSet`): the action cost of a step and the obstacle cost of the ellipsoid it reaches come from
    sx_conset_eval -- one launch per step in place of the box test -- as sx_cem_rollout_cons charges them.
    """
    _cost_args(cost, ssm)
    if con_set is not None:
        _con_set_arg(con_set)
    n_s, n_u = ssm.num_states, ssm.num_actions
    dev = actions.device
    P, H, _ = actions.shape
    lib = _lib.lib()
    arr = lambda field, r, c: torch.tensor(list(field)[:r * c], dtype=torch.float64, device=dev).view(r, c)
    u_min, u_max = arr(env.u_min, 1, n_u), arr(env.u_max, 1, n_u)
    w_abs, target, w_lin = arr(env.obj_w_abs, 1, n_s), arr(env.obj_target, 1, n_s), arr(env.obj_w_lin, 1, n_s)
    p = x0.reshape(-1, n_s).expand(P, n_s).contiguous()
    q = None
    obj = torch.zeros(P, dtype=torch.float64, device=dev)
    con = torch.zeros(P, dtype=torch.float64, device=dev)
    d = torch.empty((P, env.m), dtype=torch.float64, device=dev)
    inside = torch.empty((P,), dtype=torch.uint8, device=dev)
    for t in range(H):
        u = actions[:, t].contiguous()
        if q is None:
            mean, var = ssm.predict_without_jacobians(p, u)
            jac = None
        else:
            mean, var, jac = ssm.predict_with_jacobians(p, u)
            jac = jac.contiguous()
        mean, var = mean.contiguous(), var.contiguous()     # (a wrapping CemSSM may hand back slices: JunkDimensionsSSM)
        if group is not None:
            # the batch spans the ranks: if ANY rank holds an exact zero, every rank lifts its non-positive variances
            zero_any = (var == 0).any().to(torch.int32).reshape(1)
            torch.distributed.all_reduce(zero_any, op=torch.distributed.ReduceOp.MAX, group=group)
            lifted = zero_any.bool() & (var <= 0)
            status |= torch.where(lifted.any(), _lib.SX_STATUS_ZERO_FIX, 0).to(torch.int32)
            var = torch.where(lifted, torch.full_like(var, 1e-5), var)
        p1, q1, sigma = torch.empty_like(p), torch.empty((P, n_s, n_s), dtype=torch.float64, device=dev), torch.empty_like(p)
        _lib.check(lib.sx_onestep_reach(ctypes.byref(env), P, _lib.ptr(p), _lib.ptr(q), _lib.ptr(u), _lib.ptr(mean),
                                        _lib.ptr(var.contiguous()), _lib.ptr(jac), _lib.ptr(p1), _lib.ptr(q1),
                                        _lib.ptr(sigma), _lib.ptr(status), _lib.stream_ptr(dev)), 'sx_onestep_reach')
        # costs: objective safempc_cem.py:304-312, action box test_safempc_cem.py:59-71, polytope safempc_cem.py:102-132
        if cost is not None:
            obj = obj + cost.evaluate_device(p1, q1, status)
        elif objective_hook is not None:
            obj = obj + objective_hook(p1)
        elif env.obj_mode == _lib.SX_OBJ_NEG_VARIANCE:
            obj = obj - sigma.sum(dim=1)
        else:
            obj = obj + (w_abs * (target - p1).abs() + w_lin * p1).sum(dim=1)
        if con_set is None:
            con = con + _lib.SX_ACTION_VIOLATION_COST * ((u < u_min) | (u > u_max)).any(dim=1)
        else:
            # (q: the ellipsoid the step starts from, None at a point; the terminal ellipsoid meets no obstacle row)
            con = con + conset_eval(env, con_set, u, q, p1, q1, check_obstacle=t + 1 < H)
        if env.con_mode == _lib.SX_CON_ALL_STATES or t == H - 1:
            _lib.check(lib.sx_polytope_distance(ctypes.byref(env), P, _lib.ptr(p1), _lib.ptr(q1), 1.0, _lib.ptr(d),
                                                _lib.ptr(inside), _lib.stream_ptr(dev)), 'sx_polytope_distance')
            con = con + _lib.SX_STATE_VIOLATION_COST * (inside == 0)
        p, q = p1, q1
    return dict(obj_cost=obj, con_cost=con)


def start_constraint_cost(env: _lib.SxEnv, x0: Tensor) -> Tensor:
    """[P]: SX_STATE_VIOLATION_COST for every start x0 [P x n_s] outside the safe polytope (h_mat x0 - h_vec >= 0 in any
    row), what sx_cem_rollout_starts adds in its kernel: sx_polytope_distance on the points (an all-zero Q)."""
    P, n_s = x0.shape
    dev = x0.device
    d = torch.empty((P, env.m), dtype=torch.float64, device=dev)
    inside = torch.empty((P,), dtype=torch.uint8, device=dev)
    q = torch.zeros((P, n_s, n_s), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().sx_polytope_distance(ctypes.byref(env), P, _lib.ptr(x0.contiguous()), _lib.ptr(q), 1.0, _lib.ptr(d),
                                               _lib.ptr(inside), _lib.stream_ptr(dev)), 'sx_polytope_distance')
    return _lib.SX_STATE_VIOLATION_COST * (inside == 0)


def start_obstacle_cost(env: _lib.SxEnv, con_set, x0: Tensor) -> Tensor:
    """[P]: SX_STATE_VIOLATION_COST for every start x0 [P x n_s] that violates the obstacle rows of `con_set` (some
    h_obs-row distance of the point >= 0), what sx_cem_rollout_starts_cons adds in its kernel beside `start_constraint_cost`:
    sx_conset_eval's obstacle part on the points (an all-zero Q) with no feedback bounds and an action inside the box."""
    P, n_s = x0.shape
    n_u, dev = env.n_u, x0.device
    # (the box's lower bound is inside the strict box test, so the action part of the cost is zero)
    u = torch.tensor(list(env.u_min)[:n_u], dtype=torch.float64, device=dev).expand(P, n_u).contiguous()
    q = torch.zeros((P, n_s, n_s), dtype=torch.float64, device=dev)
    return conset_eval(env, con_set, u, None, x0, q, check_obstacle=True)


def cem_rank_refit(con: Tensor, obj: Tensor, actions: Tensor, k: int, *, cost_stride: int = 1,
                   act_stride: Optional[int] = None, row_len: Optional[int] = None, num_candidates: Optional[int] = None,
                   num_problems: Optional[int] = None, want_rows: bool = False, want_refit: bool = True,
                   rows_out: Optional[Tensor] = None):
    """Thin wrapper over sx_cem_rank_refit for E problems.

    Plain layout: con/obj [E x P], actions [E x P x ...].  Candidate-row layout (after the multi-GPU exchange): pass
    views into a [E x C x (2 + L)] buffer with cost_stride = act_stride = 2 + L, row_len = L, num_candidates = C,
    num_problems = E.  `rows_out` (contiguous [E x k x (2 + L)]) receives the elite rows in place of a fresh tensor: the
    multi-GPU solve hands in this rank's slot of the exchange buffer.
    """
    dev = con.device
    E = num_problems if num_problems is not None else con.size(0)
    P = num_candidates if num_candidates is not None else con.size(1)
    L = row_len if row_len is not None else actions[0, 0].numel()
    act_stride = act_stride if act_stride is not None else L
    idx = torch.empty((E, k), dtype=torch.int32, device=dev)
    rows = None
    if rows_out is not None:
        if tuple(rows_out.shape) != (E, k, 2 + L) or not rows_out.is_contiguous() or rows_out.dtype != torch.float64:
            raise ValueError(f'rows_out must be a contiguous float64 [{E} x {k} x {2 + L}] tensor')
        rows = rows_out
    elif want_rows:
        rows = torch.empty((E, k, 2 + L), dtype=torch.float64, device=dev)
    mean = torch.empty((E, L), dtype=torch.float64, device=dev) if want_refit else None
    std = torch.empty((E, L), dtype=torch.float64, device=dev) if want_refit else None
    best = torch.empty((E, L), dtype=torch.float64, device=dev)
    best_ok = torch.empty((E,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().sx_cem_rank_refit(E, P, k, L, ctypes.c_void_p(con.data_ptr()), ctypes.c_void_p(obj.data_ptr()),
                                            cost_stride, ctypes.c_void_p(actions.data_ptr()), act_stride, _lib.ptr(idx),
                                            _lib.ptr(rows), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(best),
                                            _lib.ptr(best_ok), _lib.stream_ptr(dev)), 'sx_cem_rank_refit')
    return dict(elite_idx=idx, elite_rows=rows, mean=mean, std=std, best=best, best_ok=best_ok)


# limits of cem_rank_kernel (csrc/sx_rank.hpp: kRankThreads * kRankSlots candidates per problem, kRankMaxK elites)
RANK_MAX_CANDIDATES = 16384
RANK_MAX_ELITES = 2048


def rank_chunks(num_candidates: int) -> int:
    """Chunks a ranking of `num_candidates` is split into (1 = the kernel takes them at once): the smallest count that
    divides the candidates evenly into chunks of at most RANK_MAX_CANDIDATES."""
    c = -(-num_candidates // RANK_MAX_CANDIDATES)
    while num_candidates % c:
        c += 1
    return c


def check_rank_limits(num_rollouts: int, num_elites: int, share: int, world: int = 1) -> None:
    """ValueError where the ranking kernel cannot pick `num_elites` of `num_rollouts` particles, `share` of them on this GPU
    of `world`: every rank hands in its top-k rows, and a share beyond RANK_MAX_CANDIDATES ranks in two levels
    (`cem_rank_refit_any`)."""
    if num_elites > num_rollouts:
        raise ValueError(f'num_elites={num_elites} exceeds num_rollouts={num_rollouts}')
    if num_elites > num_rollouts // world:
        # every rank hands in its local top-k rows; a rank that owns fewer than k particles could not, and the
        # global top-k would silently miss candidates
        raise ValueError(f'num_elites={num_elites} exceeds the smallest per-GPU share '
                         f'({num_rollouts // world} of {num_rollouts} particles over {world} GPUs)')
    if num_elites > RANK_MAX_ELITES:
        raise ValueError(f'num_elites={num_elites} exceeds the ranking kernel\'s limit of {RANK_MAX_ELITES}')
    if world > 1 and world * (num_elites + 1) > RANK_MAX_CANDIDATES:
        raise ValueError(f'{world * (num_elites + 1)} candidate rows after the exchange exceed the ranking kernel\'s '
                         f'limit of {RANK_MAX_CANDIDATES}')
    chunks = rank_chunks(share)     # > 1: two-level ranking on this GPU (cem_rank_refit_any)
    if chunks > 1 and (num_elites > share // chunks or chunks * num_elites > RANK_MAX_CANDIDATES):
        raise ValueError(f'{share} particles per GPU rank in {chunks} chunks: num_elites={num_elites} is '
                         f'too large for it (limit {min(share // chunks, RANK_MAX_CANDIDATES // chunks)})')


def expand_init_std(init_std, horizon: int, n_u: int) -> Tensor:
    """`init_std` -- a scalar, one value per step [H] or [H x n_u] -- as a float64 [H x n_u] tensor on the host."""
    std = torch.as_tensor(init_std, dtype=torch.float64).cpu()
    return (std.reshape(horizon, -1) if std.dim() > 0 else std).expand(horizon, n_u).clone()


def cem_rank_refit_any(con: Tensor, obj: Tensor, actions: Tensor, k: int, **kw):
    """`cem_rank_refit` for any candidate count.  Beyond the kernel's 16 384 candidates per problem (BASELINE config 3's
    65 536 particles on ONE GPU) the ranking runs in two levels, exactly like the multi-GPU exchange without the collective:
    the C chunks of a problem hand in their top-k rows (one launch, E x C workgroups side by side), a second launch ranks
    the C k candidates.  `elite_idx` then numbers candidate rows, not particles (as after the exchange); equal
    (constraint, objective) pairs across chunks are ordered by chunk, not by particle index."""
    E, P = con.shape
    C = rank_chunks(P)
    if C == 1:
        return cem_rank_refit(con, obj, actions, k, **kw)
    Pc, L = P // C, actions[0, 0].numel()
    if k > Pc or C * k > RANK_MAX_CANDIDATES:
        raise ValueError(f'{P} candidates rank in {C} chunks of {Pc}: k={k} must not exceed the chunk size, nor '
                         f'{C} k the kernel\'s {RANK_MAX_CANDIDATES}')
    local = cem_rank_refit(con.reshape(E * C, Pc), obj.reshape(E * C, Pc), actions.reshape(E * C, Pc, L), k,
                           want_rows=True, want_refit=False)
    flat = local['elite_rows'].reshape(-1)                       # [E x C k x (2 + L)] candidate rows
    return cem_rank_refit(flat, flat[1:], flat[2:], k, cost_stride=2 + L, act_stride=2 + L, row_len=L,
                          num_candidates=C * k, num_problems=E, **kw)


def _hand_off(owner, best: Tensor, best_ok: Tensor, status: Tensor, q_block: Optional[Tensor]):
    """The ONE device->host hand-off of a solve: one launch packs [status words | flags | point-state check | actions], one
    copy into pinned memory (kept on `owner`) brings them over (sx_cem_pack_result).  Returns (status words int64 [G],
    found bool [E], "q_block has a non-zero entry", best on the host)."""
    G, E, L = status.numel(), best_ok.numel(), best[0].numel()
    n = G + E + 1 + E * L
    packed = torch.empty(n, dtype=torch.float64, device=best.device)
    _lib.check(_lib.lib().sx_cem_pack_result(G, E, L, _lib.ptr(status), _lib.ptr(best_ok), _lib.ptr(q_block),
                                             q_block.numel() if q_block is not None else 0,
                                             _lib.ptr(best.contiguous()), _lib.ptr(packed),
                                             _lib.stream_ptr(best.device)), 'sx_cem_pack_result')
    host = getattr(owner, '_pinned', None)
    if host is None or host.numel() < n:
        owner._pinned = host = torch.empty(max(n, 256), dtype=torch.float64).pin_memory()
    host[:n].copy_(packed, non_blocking=True)
    torch.cuda.current_stream(best.device).synchronize()
    out = host[:n].clone()
    return (out[:G].to(torch.int64), out[G:G + E] != 0, bool(out[G + E] != 0),
            out[G + E + 1:].view(best.shape))


def fold_status(words) -> int:
    """Bitwise OR of the per-rank status words `solve` returns (host side: a handful of ints)."""
    out = 0
    for w in words.reshape(-1).tolist():
        out |= int(w)
    return out


def _cem_iterations(iterations: int, rollout, rank, mean: Tensor, std: Tensor):
    """The CEM loop of a solve: per iteration `rollout(it, mean, std, rows)`, then `rank(it, rollout)`, whose elite rows
    (where it skipped the refit: the next rollout refits in its prologue) or refit (mean, std) go to the next iteration.
    Returns the last ranking (`best`, `best_ok`)."""
    rows = out = None
    for it in range(iterations):
        out = rank(it, rollout(it, mean, std, rows))
        if out['mean'] is None:
            rows = out['elite_rows']
        else:
            mean, std = out['mean'].view(mean.shape), out['std'].view(std.shape)
    return out


def _check_solve(owner, x0: Tensor, q_block: Optional[Tensor], best: Tensor, best_ok: Tensor, status: Tensor, where: str,
                 problems):
    """What follows a FusedCemMpc or MultiModelCemMpc solve: the ONE device->host hand-off, the point-state check, the
    step-by-step repeat (same draws) of a problem whose status has both SX_STATUS_NAN and SX_STATUS_ZERO_FIX set, and
    raise_for_status with the failure dump.  `problems`: how the status words group -- (solver, rows) per problem, rows
    indexing both the status words and the episodes: one problem over all G rank words and E episodes for a single-model
    solve, (solvers[e], e:e+1) for a multi-model one.  Returns (best, found bool [E] on the host, "a problem repeated")."""
    words, found, is_nonpoint, best_host = _hand_off(owner, best, best_ok, status, q_block)
    if is_nonpoint:
        raise NotImplementedError(f'{where} starts from point states (all-zero Q), as CemSafeMPC.get_action does')
    statuses = [fold_status(words[r]) for _, r in problems]
    both = _lib.SX_STATUS_NAN | _lib.SX_STATUS_ZERO_FIX
    repeated = False
    for i, (s, r) in enumerate(problems):
        if (statuses[i] & both) == both and owner._last_noise is not None:
            # The fused kernel lifts exact-zero variances per particle; the reference decides on the whole batch: with a
            # zero present it lifts the NEGATIVE variances too and carries on, where the kernel went to sqrt -> NaN
            # (gp_reachability_pytorch.py:234-243).  Both bits set is the only case in which that can matter: repeat
            # the solve with the same draws through the step-by-step path, which follows the reference's rule.
            owner.stepwise_fallbacks += 1
            repeated = True
            b, ok, _, st = s.solve(x0[r], noise=owner._last_noise[:, r].contiguous(), stepwise=True)
            w, found[r], _, best_host[r] = _hand_off(owner, b, ok, st, None)
            statuses[i] = fold_status(w)
    for (s, _), st in zip(problems, statuses):
        s.last_status = st
    for i, ((s, r), st) in enumerate(zip(problems, statuses)):
        # (a solver that did not run the checked solve itself holds none of its actions)
        raise_for_status(st, where if len(problems) == 1 else f'{where} (problem {i})',
                         dump=lambda s=s, r=r: save_failure_state(s._ssm, x0[r], s._last_actions if s is owner else None))
    return best_host, found, repeated


def _checked_cost(cost, n_s: int, kind: Optional[str], on_safety: bool = False):
    """`cost` as `set_cost` of the solvers keeps it: None, or a SaturatingCost for this state dimension on a solver whose
    performance rollout is the Taylor form (`kind`; the cautious solver's always is), or which prices the safety
    ellipsoids (`on_safety`: FusedCemMpc(cost_on_safety=True), which has no performance trajectory)."""
    if cost is None:
        return None
    if not isinstance(cost, SaturatingCost):
        raise TypeError(f'cost must be a costs.SaturatingCost or None, got {type(cost).__name__}')
    if kind != 'taylor' and not on_safety:
        raise ValueError("a SaturatingCost prices (mean, covariance) pairs: it needs a performance trajectory with "
                         "cem_perf_type='taylor' (perf_type='taylor', n_perf > 0), not "
                         + ('no performance trajectory' if kind is None else f'the {kind!r} form')
                         + ('; without one, cost_on_safety=True (cem_cost_on_safety) prices the safety ellipsoids'
                            if kind is None else ''))
    if cost.n_s != n_s:
        raise ValueError(f'the cost is built for n_s = {cost.n_s}, the model has n_s = {n_s}')
    return cost


class FusedCemMpc:
    """Drop-in for ``ConstrainedCemMpc``: ``get_actions(flat_state [1 x S]) -> (actions [H x n_u] | None, rollouts)``.

    With a process group of G > 1 ranks the particles are sharded (``num_rollouts`` is the GLOBAL count): every rank
    rolls out its share, keeps its local top-k rows, ONE all-gather per iteration assembles the G*(k+1) candidate rows, and
    every rank redundantly ranks them and refits -- bit-identical on all ranks.

    ``n_perf > 0`` adds the performance trajectory of a SafeMPC (exact RBF GPs, one GPU): n_perf
    mean-equivalent steps that share their first ``perf_r`` actions with the safety trajectory and carry the objective,
    while the safety trajectory keeps the constraints.  The CEM distribution then covers the row [safety actions | tail] of
    H + n_perf - perf_r steps; an iteration is the safety rollout, ``sx_cem_perf_rollout`` and the ranking over those rows.
    ``get_actions*`` still return the H safety actions of the best row; its tail is ``last_perf_actions``.

    ``perf_variance=True`` (with ``n_perf > 0``) runs ``sx_cem_perf_rollout_var`` in place of ``sx_cem_perf_rollout``: the
    performance trajectory then carries the GP's posterior variance at every step, and with it the variance objective
    (SX_OBJ_NEG_VARIANCE: an exploration run looks n_perf steps ahead for where the model is uncertain).  Recorded rollouts
    keep the performance means and variances.

    ``perf_type='taylor'`` (with ``n_perf > 0``; default ``'mean_equivalent'``) runs ``sx_cem_perf_rollout_taylor``: the
    state covariance is propagated to first order along the performance trajectory under the fixed feedback ``env.k_fb``,
    and the objective sees the variance including it.  It carries the variance objective by itself, as ``perf_variance``
    does.  ``perf_terminal_safety=True`` adds the state-violation cost where the performance ellipsoid at step
    ``time_horizon + 2`` leaves the safe polytope (``n_perf >= time_horizon + 2``).  Recorded rollouts gain ``perf_cov``.

    ``cost_on_safety=True`` (with ``n_perf == 0``) lets ``set_cost`` take a ``SaturatingCost`` as the
    objective of the safety trajectory itself: every ellipsoid (p_t, Q_t), t = 1 .. H, is priced as a mean and a covariance
    in the rollout kernel (``sx_cem_rollout_sat`` / ``sx_cem_rollout_elites_sat``, the streaming form), what the reference's
    ``n_perf = 0`` configs hand their solver.  The cost belongs to one trajectory, chosen by ``n_perf``.

    ``con_set`` (an ``_lib.SxConSet``, ``make_con_set``) adds the reference's SafeMPC constraints to
    the safety trajectory: the control ellipsoid (k_ff_t, K Q_t K^T) inside the action box wherever a step starts from an
    ellipsoid, and the obstacle polytope on every intermediate safety ellipsoid, as penalties of 3 and 10 in the rollout
    kernel (``sx_cem_rollout_cons`` / ``sx_cem_rollout_elites_cons``, the streaming form; the step-by-step path charges
    them with ``sx_conset_eval``).  Exact RBF GPs on one GPU without a performance trajectory; ``set_env`` keeps the set.
    """

    def __init__(self, ssm: GpCemSSM, env: _lib.SxEnv, time_horizon: int, num_rollouts: int, num_elites: int,
                 num_iterations: int, *, device=None, seed: int = 0, init_std=1.0, warm_start: str = 'zero',
                 record_rollouts: bool = False, process_group=None, force_exchange: bool = False, n_perf: int = 0,
                 perf_r: int = 1, perf_variance: bool = False, perf_type: str = 'mean_equivalent',
                 perf_terminal_safety: bool = False, cost_on_safety: bool = False, con_set=None):
        self._ssm = ssm
        self._con_set = _checked_con_set(con_set, ssm)
        if con_set is not None:
            if int(n_perf) > 0:
                raise NotImplementedError(f'con_set constrains the safety trajectory of a solve without a performance '
                                          f'trajectory: got n_perf={n_perf} (cem_n_perf > 0 is not built)')
            if process_group is not None:
                raise NotImplementedError('con_set is not built for sharded particles (a process group)')
        self._cost_on_safety = bool(cost_on_safety)
        if self._cost_on_safety and int(n_perf) > 0:
            raise ValueError(f'cost_on_safety=True prices the safety trajectory, which carries the objective only without a '
                             f'performance trajectory: got n_perf={n_perf}.  The cost belongs to one trajectory, chosen by '
                             f"n_perf (n_perf > 0 with perf_type='taylor' prices the performance trajectory)")
        self._env = env
        self._horizon = time_horizon
        # the performance trajectory (off with n_perf = 0): T tail steps behind the H safety steps of a row
        self._perf = PerfSpec(n_perf, perf_r, perf_variance, perf_type, perf_terminal_safety).checked(time_horizon)
        if self._perf.on:
            _require_exact_rbf([ssm], 'the performance trajectory is')
            if process_group is not None:
                raise NotImplementedError('the performance trajectory is not built for sharded particles (a process group)')
            self._check_perf_objective(env)
        self.last_perf_actions = None     # [E x T x n_u] on the host: the tail of the last checked solve's best rows
        self._num_iterations = num_iterations
        self._record = record_rollouts
        # the first iteration's sampling distribution: std is a scalar or one value per step [H] / [H x n_u];
        # warm_start 'zero' = mean 0 (the reference's cold start), 'safe_policy' = the safe controller u = k_fb x rolled
        # through the model's mean dynamics from x0 (safe_policy_plan)
        self._init_std = expand_init_std(init_std, time_horizon, ssm.num_actions)
        if self._perf.on:   # the tail steps start from the last safety step's value
            self._init_std = torch.cat([self._init_std, self._init_std[-1:].expand(self._perf.tail, -1)])
        if warm_start not in ('zero', 'safe_policy'):
            raise ValueError(f"warm_start must be 'zero' or 'safe_policy', got {warm_start!r}")
        self._warm_start = warm_start
        self._group = process_group
        self._world, self._rank = distributed.world_and_rank(process_group)
        # force_exchange: take the sharded code path (local ranking -> collective -> global ranking) even with ONE rank -- how
        # tests/test_gpu_distributed.py runs that path over RCCL (backend 'nccl') on a single-GPU box
        self._sharded = self._world > 1 or (force_exchange and process_group is not None)
        self._num_rollouts = num_rollouts
        self._local_rollouts, _ = distributed.shard_particles(num_rollouts, self._world, self._rank)
        check_rank_limits(num_rollouts, num_elites, self._local_rollouts, self._world)
        self._num_elites = num_elites
        self._local_elites = num_elites     # the same k on every rank
        self._device = torch.device(device if device is not None else 'cuda:0')
        self._init_std = self._init_std.to(self._device)
        # the iteration's collective on the compute stream (our own RCCL communicator) where the group is an nccl one
        self._comm = distributed.make_comm(process_group, self._device) if self._sharded else None
        self._gen = torch.Generator(device=self._device)
        self._gen.manual_seed(distributed.rank_seed(seed, self._rank))
        self.last_status = 0
        # a CemSSM that only offers the predict_* surface (JunkDimensionsSSM over a HIP-backed model) is always rolled out
        # step by step: sx_gp_predict through the wrapper + sx_onestep_reach per step, the reference's own call pattern
        self._always_stepwise = getattr(ssm, 'kernel_family', None) == 'stepwise'
        self.stepwise_fallbacks = 0     # solves repeated through the step-by-step path (see _check_solve)
        self._last_noise = self._last_actions = None
        self._objective_hook = None
        self._cost = None
        # bench.py sets this to a list: (start, end) torch.cuda.Event pairs are then recorded around every
        # sx_cem_rollout launch, on the stream the kernel runs on
        self.rollout_events = None
        # likewise around the multi-GPU part of an iteration (collective + global ranking launch): bench.py's exchange_us.
        # Every `exchange_event_stride`-th exchange only: an event pair around EVERY exchange cost 7 us per iteration
        # (measured with one RCCL rank), 4 % of a sharded config-2 iteration
        self.exchange_events = None
        self.exchange_event_stride = 16
        self._exchanges_seen = 0

    @property
    def num_iterations(self) -> int:
        return self._num_iterations

    def set_env(self, env: _lib.SxEnv, objective_hook=None) -> None:
        """New problem constants (the pendulum's objective target moves between calls).  `objective_hook`, if given, is
        an ``Environment.objective_cost_function`` this module has no kernel form for: it is then evaluated with torch
        on the recorded trajectory centres, H small launches per iteration instead of none."""
        if self._perf.on and objective_hook is None:
            self._check_perf_objective(env)
        self._env = env
        self._objective_hook = objective_hook
        self._prior_tensors = None

    def set_cost(self, cost) -> None:
        """The saturating cost (`costs.SaturatingCost`) as the objective of the performance trajectory, priced in the kernel
        on (mu_{t+1}, Sigma_{t+1}) of every step (sx_cem_perf_rollout_taylor_sat): env's objective is then not read and no
        objective hook is evaluated.  None takes it off again.  Needs the propagated covariance.
        On a solver built with ``cost_on_safety=True`` (no performance trajectory) the cost prices the safety ellipsoids
        instead (sx_cem_rollout_sat; the step-by-step path prices them with sx_sat_cost_eval): again env's objective is not
        read, no hook is evaluated and no trajectory is recorded for one."""
        on_safety = getattr(self, '_cost_on_safety', False)
        if cost is not None and on_safety:
            _require_exact_rbf([self._ssm], _COST_IS)
        self._cost = _checked_cost(cost, self._ssm.num_states, perf_spec_of(self).kind, on_safety)

    @property
    def _safety_cost(self):
        """The cost where it prices the safety trajectory (cost_on_safety), else None."""
        return self._cost if getattr(self, '_cost_on_safety', False) else None

    def _check_perf_objective(self, env: _lib.SxEnv) -> None:
        if env.obj_mode == _lib.SX_OBJ_NEG_VARIANCE and self._perf.kind == 'mean':
            raise ValueError('the performance trajectory propagates means only: it cannot carry the variance objective '
                             '(SX_OBJ_NEG_VARIANCE); give the environment an objective_cost_function, or pass '
                             "perf_variance=True or perf_type='taylor'")

    def _prior(self):
        """(a [n_s x n_s], b [n_s x n_u], k_fb [n_u x n_s]) of the current sx_env as device tensors."""
        if getattr(self, '_prior_tensors', None) is None:
            n_s, n_u = self._ssm.num_states, self._ssm.num_actions
            t = lambda arr, r, c: torch.tensor(list(arr)[:r * c], dtype=torch.float64, device=self._device).view(r, c)
            self._prior_tensors = (t(self._env.a, n_s, n_s), t(self._env.b, n_s, n_u), t(self._env.k_fb, n_u, n_s))
        return self._prior_tensors

    def safe_policy_plan(self, x0: Tensor, steps: Optional[int] = None) -> Tensor:
        """[E x H x n_u] ([E x steps x n_u] where given): the safe controller u_t = k_fb x_t (reference safempc_cem.py:259-262, the last rung of the
        fallback ladder) rolled through the model's MEAN dynamics x_{t+1} = a x_t + b u_t + mu(x_t, u_t) from x0
        [E x n_s] -- H one-point-per-episode sx_gp_predict launches, nothing synchronises.  It is the warm start of
        workloads whose open-loop instability (cart-pole: 1.77 per step, 9e4 over H = 20) leaves a zero-mean start no
        feasible particle to learn from."""
        a, b, k_fb = self._prior()
        x = x0.to(self._device, torch.float64)
        plan = []
        for _ in range(self._horizon if steps is None else steps):
            u = x @ k_fb.t()
            mean, _ = self._ssm.predict_without_jacobians(x.contiguous(), u.contiguous())
            plan.append(u)
            x = x @ a.t() + u @ b.t() + mean
        return torch.stack(plan, dim=1)

    def _constant(self, name: str, episodes: int, dev, make) -> Tensor:
        """A read-only device tensor that depends on (name, episodes, device) only, built once."""
        cache = self.__dict__.setdefault('_constants', {})
        key = (name, episodes, str(dev))
        if key not in cache:
            cache[key] = make()
        return cache[key]

    def _fresh_status(self, dev) -> Tensor:
        """A zeroed int32[1] status word: slices of a pool that is zeroed once per 256 solves (one fill launch instead of
        256).  A slice is handed out once per pool generation; callers read it right after the solve."""
        pool = getattr(self, '_status_pool', None)
        if pool is None or self._status_next >= pool.numel() or pool.device != dev:
            self._status_pool = pool = torch.zeros(256, dtype=torch.int32, device=dev)
            self._status_next = 0
        i = self._status_next
        self._status_next += 1
        return pool[i:i + 1]

    def _exchange(self, episodes: int, k: int, row_len: int, dev):
        """The exchange buffers of a solve.  One problem (all-gather mode): every cell is overwritten by each solve and the
        padding rows never change, so the object is built once and kept -- four small launches per solve otherwise.  Several
        problems (all-reduce over zero padding): fresh, zeroed buffers per solve."""
        if episodes != 1:
            return distributed.EliteExchange(self._num_iterations, episodes, k, row_len, self._group, dev, comm=self._comm)
        key = (k, row_len, str(dev))
        cache = self.__dict__.setdefault('_xch_cache', {})
        if key not in cache:
            cache[key] = distributed.EliteExchange(self._num_iterations, 1, k, row_len, self._group, dev, comm=self._comm)
        return cache[key]

    def _next_noise(self, episodes: int) -> Tensor:
        """[iters x E x P_local x H x n_u] standard normals for one solve (H + T steps with a performance trajectory), from
        this solver's generator.  They are drawn for
        up to 8 solves per generator launch (at most 256 MB): one launch per solve is 8 us + a 6 us gap in front of the first
        rollout, 1.2 % of a config-2 solve."""
        shape = (self._num_iterations, episodes, self._local_rollouts, self._perf.row_steps(self._horizon),
                 self._ssm.num_actions)
        pool = getattr(self, '_noise_pool', None)
        if pool is None or tuple(pool.shape[1:]) != shape or self._noise_next >= pool.size(0):
            per_solve = 8
            for n in shape:
                per_solve *= n
            batch = max(1, min(8, (256 << 20) // max(per_solve, 1)))
            self._noise_pool = pool = torch.randn((batch,) + shape, dtype=torch.float64, device=self._device,
                                                  generator=self._gen)
            self._noise_next = 0
        out = pool[self._noise_next]
        self._noise_next += 1
        return out

    def sample_noise(self, episodes: int = 1) -> Tensor:
        return torch.randn((episodes, self._local_rollouts, self._perf.row_steps(self._horizon), self._ssm.num_actions),
                           dtype=torch.float64, device=self._device, generator=self._gen)

    def start_distribution(self, x0: Tensor, init_mean: Optional[Tensor] = None,
                           init_std: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """The first iteration's sampling distribution (mean, std) [E x H x n_u] from start states x0 [E x n_s]:
        `init_mean` / `init_std` where given, else the warm start's mean and the constructor's init_std; with a performance
        trajectory H + T steps, the tail behind the safety steps (zero mean, or the safe policy's plan continued).  (The constant
        ones are kept between solves: three small launches per solve otherwise, 2 % of a config-2 solve.)"""
        perf = self._perf
        E, dev, H, n_u = x0.size(0), x0.device, perf.row_steps(self._horizon), self._ssm.num_actions
        if init_mean is not None:
            mean = init_mean.to(dev).reshape(E, H, n_u).clone()
        elif self._warm_start == 'safe_policy' and perf.on:
            # the plan continued for n_perf steps: its first H steps, then the steps perf_r .. n_perf - 1 as the tail
            plan = self.safe_policy_plan(x0, max(self._horizon, perf.n_perf))
            mean = torch.cat([plan[:, :self._horizon], plan[:, perf.r:perf.n_perf]], dim=1).contiguous()
        elif self._warm_start == 'safe_policy':
            mean = self.safe_policy_plan(x0).contiguous()
        else:
            mean = self._constant('zero_mean', E, dev, lambda: torch.zeros((E, H, n_u), dtype=torch.float64, device=dev))
        std = (init_std.to(dev).reshape(E, H, n_u).clone() if init_std is not None else
               self._constant('init_std', E, dev, lambda: self._init_std.to(dev).expand(E, H, n_u).contiguous()))
        return mean, std

    def _refit_in_prologue(self, episodes: int) -> bool:
        """`fused_refit_applies` for a solve of this solver's model, over the candidates of an iteration's last ranking
        launch: the exchanged rows of a sharded solve, the chunks' elite rows of a two-level ranking, else the particles."""
        chunks = rank_chunks(self._local_rollouts)
        candidates = (self._world * (self._local_elites + (1 if episodes == 1 else 0)) if self._sharded
                      else chunks * self._num_elites if chunks > 1 else self._local_rollouts)
        return fused_refit_applies(self._ssm, episodes, self._local_rollouts, self._horizon, candidates)

    def _rollout_stepwise(self, x0: Tensor, mean: Tensor, std: Tensor, eps: Tensor, status: Tensor):
        """One iteration's rollout through `cem_rollout_stepwise`, problem by problem."""
        acts = (mean.unsqueeze(1) + std.unsqueeze(1) * eps).contiguous()       # [E x P x H x n_u]
        cost = self._safety_cost
        per_e = [cem_rollout_stepwise(self._ssm, self._env, x0[e], acts[e], status=status,
                                      group=self._group if self._world > 1 else None,
                                      objective_hook=self._objective_hook if cost is None else None,
                                      **({} if cost is None else dict(cost=cost)),
                                      **_con_set_kw(getattr(self, '_con_set', None))) for e in range(x0.size(0))]
        return dict(actions=acts, traj=None, obj_cost=torch.stack([q['obj_cost'] for q in per_e]),
                    con_cost=torch.stack([q['con_cost'] for q in per_e]))

    def solve(self, x0: Tensor, noise: Optional[Tensor] = None, init_mean: Optional[Tensor] = None,
              init_std: Optional[Tensor] = None, stepwise: bool = False) -> Tuple[Tensor, Tensor, List[Rollouts], Tensor]:
        """E independent solves from x0 [E x n_s] (points).  Nothing here synchronises with the host.

        stepwise: roll out through `cem_rollout_stepwise` (H x (sx_gp_predict + sx_onestep_reach) per iteration, the
        reference's whole-batch zero fix-up) instead of the fused kernel; `get_actions` uses it to settle the one case
        in which the fused kernel's per-particle fix-up can differ from the reference's.

        noise: optional [iters x E x P_local x H x n_u] pre-drawn standard normals (parity tests inject them).
        Returns (best [E x H x n_u], best_ok int32 [E], rollouts per iteration (if recorded), status int32 [G]: the
        status word of every rank, identical on all ranks; G = 1 without a process group -- OR them, `fold_status`).

        With a performance trajectory (n_perf > 0) the rows are H + T steps long, T = n_perf - perf_r: `noise`,
        `init_mean`, `init_std` and the returned best rows have H + T where the above says H, the tail behind the safety
        actions.
        """
        n_u, H, E, dev = self._ssm.num_actions, self._horizon, x0.size(0), x0.device
        spec = self._perf
        perf, rows_steps = spec.on, spec.row_steps(H)
        L = rows_steps * n_u
        mean, std = self.start_distribution(x0, init_mean, init_std)
        status = self._fresh_status(dev)
        history: List[Rollouts] = []
        xch = None
        stepwise = stepwise or self._always_stepwise
        if noise is None and 'sample_noise' not in vars(self):
            # one generator launch for the whole solve instead of one per iteration (a test that patches sample_noise
            # on the instance still gets its per-iteration calls)
            noise = self._next_noise(E)
        self._last_noise, self._last_actions = noise, None
        # From the second iteration on the refit happens in the rollout kernel's prologue, straight from the elite rows of
        # the ranking before it (sx_cem_rollout_elites): the ranking launches then skip their refit tail.
        # (not with a performance trajectory: the prologue reads rows of 2 + H n_u, the ranking launch refits the long rows)
        in_prologue = (not stepwise) and (not perf) and self._refit_in_prologue(E)
        # (a cost on the safety trajectory rides in the rollout call: no hook is evaluated, no trajectory recorded for one)
        safety_cost = self._safety_cost
        cost_kw = dict({} if safety_cost is None else dict(cost=safety_cost), **_con_set_kw(getattr(self, '_con_set', None)))
        want_traj = self._record or (self._objective_hook is not None and not perf and safety_cost is None)
        if perf and noise is not None:
            # the draws of the safety steps and of the tail, each contiguous: two copies per solve
            noise_safe, noise_tail = noise[:, :, :, :H].contiguous(), noise[:, :, :, H:].contiguous()

        def rollout(it, mean, std, rows):
            nonlocal stepwise, in_prologue
            eps = noise[it] if noise is not None else self.sample_noise(E)
            if noise is None:
                self._last_noise = None      # per-iteration draws (a patched sample_noise): nothing to replay
            if self.rollout_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(torch.cuda.current_stream(dev))
            if perf:
                # the safety rollout runs over the first H steps of the row's distribution and draws
                full_mean, full_std = mean, std
                mean, std = mean[:, :H].contiguous(), std[:, :H].contiguous()
                eps, eps_tail = ((noise_safe[it], noise_tail[it]) if noise is not None
                                 else (eps[:, :, :H].contiguous(), eps[:, :, H:].contiguous()))
            if stepwise:
                r = self._rollout_stepwise(x0, mean, std, eps, status)
            else:
                try:
                    r = cem_rollout(self._ssm, self._env, x0, H, mean=mean, std=std, elite_rows=rows,
                                    noise=eps.contiguous(), want_traj=want_traj, status=status, **cost_kw)
                except FusedJunkUnsupported:
                    # (answered before any launch) the junk-dimension model has no single-launch form for this training
                    # set: the whole solve goes step by step through the wrapper
                    if it != 0:
                        raise
                    stepwise, in_prologue = True, False
                    r = self._rollout_stepwise(x0, mean, std, eps, status)
            if perf:
                # the performance trajectory: its objective replaces the safety trajectory's, the tail's action box adds to
                # the constraint cost, and the rows [safety actions | tail] are what the ranking sees
                # (with a kernel-form cost no hook is evaluated)
                hook, n_s = (self._objective_hook if self._cost is None else None), self._ssm.num_states
                pr = _launch_perf(spec, [self._ssm], self._env, x0, H, r, full_mean, full_std, eps_tail, status,
                                  want_traj=hook is not None, record=self._record, cost=self._cost)
                r.update({key: pr[key] for key in ('perf_traj', 'perf_sigma', 'perf_cov') if key in pr})
                r.update(safe_actions=r['actions'], actions=pr['rows'], obj_cost=pr['obj_cost'], con_cost=pr['con_cost'])
                if hook is not None:
                    r['obj_cost'] = hook_objective(hook, pr['perf_traj'], spec.n_perf, n_s, pr['obj_cost'])
            elif self._objective_hook is not None and not stepwise and safety_cost is None:
                n_s = self._ssm.num_states      # (the hook sees the trajectory centres [E x P x H x n_s])
                r['obj_cost'] = hook_objective(self._objective_hook, r['traj'][..., :n_s], H, n_s, r['obj_cost'])
            if self.rollout_events is not None:
                ev[1].record(torch.cuda.current_stream(dev))
                self.rollout_events.append(ev)
            self._last_actions = r['actions']
            if self._record and r['traj'] is not None:
                for e in range(E):
                    history.append(Rollouts(r['traj'][e], r.get('safe_actions', r['actions'])[e], r['obj_cost'][e],
                                            r['con_cost'][e]))
                    if r.get('perf_sigma') is not None:
                        history[-1].perf_trajectories, history[-1].perf_sigma = r['perf_traj'][e], r['perf_sigma'][e]
                    if r.get('perf_cov') is not None:
                        history[-1].perf_cov = r['perf_cov'][e]
            return r

        def rank(it, r):
            nonlocal xch, status
            if not self._sharded:
                return cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['actions'], self._num_elites,
                                          want_rows=in_prologue, want_refit=not in_prologue)
            k = self._local_elites
            if xch is None:
                xch = self._exchange(E, k, L, dev)
            timed = self.exchange_events is not None and self._exchanges_seen % self.exchange_event_stride == 0
            self._exchanges_seen += 1
            if timed:   # four marks: before the local ranking | before the collective | after it | after the global ranking
                xev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                xev[0].record(torch.cuda.current_stream(dev))
            if E == 1:
                # the local elite rows go straight into this rank's slot: no copy between the kernel and the collective
                cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['actions'], k, want_refit=False,
                                   rows_out=xch.local_slot(it))
            else:
                local = cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['actions'], k, want_rows=True, want_refit=False)
                xch.local_slot(it).copy_(local['elite_rows'])
            last = it == self._num_iterations - 1
            if timed:
                xev[1].record(torch.cuda.current_stream(dev))
            # the ONE collective of the iteration; on the last one the status words of all ranks ride along
            # (every rollout of this solve has been enqueued by then)
            cand, words = xch.exchange(it, status if last else None)
            if timed:
                xev[2].record(torch.cuda.current_stream(dev))
            if last:
                status = words
            flat = cand.reshape(-1)
            out = cem_rank_refit(flat, flat[1:], flat[2:], self._num_elites, cost_stride=2 + L,
                                 act_stride=2 + L, row_len=L, num_candidates=xch.candidates, num_problems=E,
                                 want_rows=in_prologue, want_refit=not in_prologue)
            if timed:
                xev[3].record(torch.cuda.current_stream(dev))
                self.exchange_events.append(xev)
            return out

        out = _cem_iterations(self._num_iterations, rollout, rank, mean, std)
        return out['best'].view(E, rows_steps, n_u), out['best_ok'], history, status

    def _solve_checked(self, x0: Tensor, where: str, q_block: Optional[Tensor] = None):
        """`solve` + `_check_solve`, whose one hand-off also carries "is any entry of `q_block` non-zero" (the callers'
        point-state check, made on the device).  Returns (best [E x H x n_u] ON THE HOST, found bool [E] on the host,
        rollouts)."""
        if q_block is not None and not q_block.is_contiguous():
            q_block = q_block.contiguous()
        best, best_ok, history, status = self.solve(x0)
        best_host, found, repeated = _check_solve(self, x0, q_block, best, best_ok, status, where, [(self, slice(None))])
        if self._perf.on:
            # the callers' plan is the safety actions of the best row; its tail stays readable
            self.last_perf_actions = best_host[:, self._horizon:]
            best_host = best_host[:, :self._horizon]
        return best_host, found, [] if repeated else history     # (a step-by-step solve records no rollouts)

    def get_actions_batch(self, states: Tensor) -> Tuple[Tensor, Tensor, List[Rollouts]]:
        """E independent episodes at once (BASELINE config 5): flat start states [E x (n_s + n_s^2)], all
        points.  One fused solve: the kernels carry the episode dimension, episodes never exchange anything.

        Returns (actions [E x H x n_u] on the host, found bool [E] on the host, rollouts); ``found[e] == False`` is the
        ``get_actions`` ``None`` of episode e.  Raises like ``get_actions`` if any episode hit a numerical failure.
        """
        x0, q_block = split_flat_states(states, self._ssm.num_states, self._device)
        return self._solve_checked(x0, 'get_actions_batch', q_block=q_block)

    def get_actions(self, state: Tensor) -> Tuple[Optional[Tensor], List[Rollouts]]:
        """state: the flat start state [1 x (n_s + n_s^2)] with an all-zero Q block (a point, safempc_cem.py:234-235).
        The selected actions come back on the host (they travel with the solve's one device->host hand-off)."""
        x0, q_block = split_flat_states(state.reshape(1, -1), self._ssm.num_states, self._device, episodes=1)
        best, found, history = self._solve_checked(x0, 'get_actions', q_block=q_block)
        if not bool(found[0]):
            return None, history
        return best[0], history


class SharedPolicy(NamedTuple):
    """What a multi-model class asks of its solvers beside the table of the settings they share."""
    what: str                   # the solve, as the messages name it: 'a multi-model static solve'
    con_set: str = 'none'       # the constraint set: 'none' may carry one, 'all' carry one byte-equal set, or 'all_or_none'
    exact_rbf: bool = False     # every solver's model is an exact RBF GP
    label: str = ''             # what stands in front of a differing setting's name


def _setting(solver, attr):
    """(a solver's setting as it is compared, may a message print it): tensors by value and ctypes structs (sx_env) byte for
    byte, neither printed.  `attr`: the attribute's name -- read with a default: an injected optimiser need not be one of
    our classes -- or a function of the solver."""
    v = attr(solver) if callable(attr) else getattr(solver, attr, None)
    if isinstance(v, Tensor):
        return tuple(v.reshape(-1).tolist()), False
    return (bytes(v), False) if isinstance(v, ctypes.Structure) else (v, True)


def _model_shape(solver) -> tuple:
    return solver._ssm.num_states, solver._ssm.num_actions


def _compare_settings(solvers: Sequence, table, what: str, label: str = '') -> None:
    """ValueError, naming the setting and the solver, unless every solver has solver 0's value of every (reported name,
    attribute) of `table`."""
    for name, attr in table:
        first, printable = _setting(solvers[0], attr)
        for e, s in enumerate(solvers[1:], start=1):
            other = _setting(s, attr)[0]
            if other != first:
                raise ValueError(f'the solvers of {what} must share {label}{name}: '
                                 + (f'solver 0 has {first!r}, solver {e} has {other!r}' if printable
                                    else f'solver {e} differs from solver 0'))


def _shared_con_set(solvers: Sequence, policy: str, what: str):
    """The constraint set of a multi-model solve (None: no solver carries one), whose launch takes ONE: by `policy` no
    solver may carry a set ('none'), all carry one ('all') or all or none do ('all_or_none'), and the sets are equal byte
    for byte, as the environments are compared.  NotImplementedError, naming con_set, where the solve is not built for the
    solvers' sets; ValueError for differing ones."""
    sets = [getattr(m, '_con_set', None) for m in solvers]
    have = sum(c is not None for c in sets)
    if have and policy == 'none':
        raise NotImplementedError(f'{what} is not built for con_set: MultiModelConsCemMpc solves over solvers that all '
                                  f'carry one set')
    if have not in (0, len(sets)):
        raise NotImplementedError(f'the solvers of {what} all carry a constraint set (con_set) or none does: {have} of '
                                  f'{len(sets)} have one; the ones without act in a multi-model solve of their own')
    if not have and policy == 'all':
        raise NotImplementedError(f'{what} needs solvers with a constraint set (con_set); MultiModelCemMpc solves the others')
    for e, c in enumerate(sets[:have]):
        _con_set_arg(c)
        if bytes(c) != bytes(sets[0]):
            raise ValueError(f'the solvers of {what} must share one constraint set (con_set: the obstacle rows and the '
                             f'feedback bounds of the environment they share): solver {e} differs from solver 0')
    return sets[0]


def check_shared_settings(solvers: Sequence, table, policy: SharedPolicy) -> None:
    """THE comparison of the solvers of one multi-model solve: the models' family and the constraint sets by `policy`
    (NotImplementedError), then every setting of `table` (ValueError)."""
    if policy.exact_rbf:
        _require_exact_rbf([m._ssm for m in solvers], policy.what + ' is', numbered=True)
    _shared_con_set(solvers, policy.con_set, policy.what)
    _compare_settings(solvers, table, policy.what, policy.label)


class MultiModelCem:
    """What the multi-model solvers share.  Problem (or scenario) e keeps a single-model solver of its own, ``solvers[e]``:
    it supplies the problem's noise draws and start distribution, so a multi-model solve samples exactly what the solvers'
    own solves would, and it takes over where the single launch does not apply (``fused_applies``; ``per_model_solves``
    counts those solves) and for the step-by-step repeat of one problem (``stepwise_fallbacks``).  The solvers agree on
    the class's ``_SHARED`` settings and ``_POLICY`` (``check_solvers``).  The device table of the models is kept between
    solves.

    A subclass supplies the two, how problem e draws its noise and starts, the rollout call of ``solve`` and the form
    query ``fused_applies``."""

    _SHARED: tuple = ()         # (reported name, attribute) of every setting the solvers of one solve share
    _POLICY: SharedPolicy

    def __init__(self, solvers: Sequence, family: Optional[str] = 'rbf', table: Optional[tuple] = None):
        """`table`: the settings compared here, where they are fewer than `check_solvers` compares."""
        solvers = list(solvers)
        if not solvers:
            raise ValueError(f'{type(self).__name__} needs at least one solver')
        check_shared_settings(solvers, self._SHARED if table is None else table, self._POLICY)
        self._solvers = solvers
        self._table = GpModelTable(family) if family is not None else None
        self._last_noise = self._last_actions = None
        self.stepwise_fallbacks = 0     # problems repeated through the step-by-step path (what _check_solve counts)
        self.per_model_solves = 0       # solves that went one solver at a time (single launch not applicable)

    @classmethod
    def check_solvers(cls, solvers: Sequence) -> None:
        """ValueError, naming the setting and the solver, unless the solvers share every setting of the class's `_SHARED`;
        NotImplementedError where the class is not built for the solvers' constraint sets or models (`_POLICY`)."""
        check_shared_settings(solvers, cls._SHARED, cls._POLICY)

    @property
    def solvers(self) -> list:
        return self._solvers

    @property
    def last_status(self) -> List[int]:
        """The status word of every problem's last solve."""
        return [s.last_status for s in self._solvers]

    @property
    def _env(self) -> _lib.SxEnv:
        return self._solvers[0]._env      # (ONE sx_env: check_solvers compares the solvers')

    @property
    def _device(self):
        return self._solvers[0]._device

    def set_env(self, env: _lib.SxEnv) -> None:
        """`set_env` on every solver."""
        for s in self._solvers:
            s.set_env(env)

    def set_cost(self, cost) -> None:
        """`set_cost` on every solver."""
        for s in self._solvers:
            s.set_cost(cost)

    def _get_actions_multi(self, states: Tensor, where: str, **init) -> Tuple[Tensor, Tensor]:
        """`get_actions_multi` of the classes that solve from given states (problem e over `self._ssms[e]`): flat start
        states [E x (n_s + n_s^2)], all points.  One solve per solver, each with its own checks (and its own step-by-step
        repeat), where `fused_applies` is False; else ONE `solve` and `_check_solve` with a status word per problem.
        `init`: per-problem tensors [E x ...] for `solve`, handed row by row to the solvers' own solves.  Returns (best
        rows on the host, found bool [E] on the host)."""
        x0, q_block = split_flat_states(states, self._ssms[0].num_states, self._device, episodes=len(self._ssms))
        q_block = q_block.contiguous()
        if not self.fused_applies():
            self.per_model_solves += 1
            per = [s._solve_checked(x0[e:e + 1], where, q_block=q_block[e:e + 1],
                                    **{key: v[e:e + 1] for key, v in init.items()}) for e, s in enumerate(self._solvers)]
            return torch.cat([p[0] for p in per]), torch.cat([p[1] for p in per])
        best, best_ok, status = self.solve(x0, **init)
        best_host, found, _ = _check_solve(self, x0, q_block, best, best_ok, status, where,
                                           [(s, slice(e, e + 1)) for e, s in enumerate(self._solvers)])
        return best_host, found


def keep_multi(cached, cls, solvers: Sequence):
    """`cached` where it is a `cls` over exactly `solvers`, else a new one (`cls.from_solvers`): how a front end keeps the
    multi-model solver, and with it the device table, between calls."""
    if type(cached) is cls and len(cached.solvers) == len(solvers) and all(a is b for a, b in zip(cached.solvers, solvers)):
        return cached
    return cls.from_solvers(solvers)


class MultiModelCemMpc(MultiModelCem):
    """E independent problems with a model each -- the reference's exploration scenarios, each with its own training set,
    hyper-parameters or network -- solved together: one multi-model rollout launch and one ``sx_cem_rank_refit`` launch per
    CEM iteration for all of them, where ``FusedCemMpc`` needs one solve per model.  The models share one kernel_family:
    exact RBF GPs (``sx_cem_rollout_multi``), feature-space GPs, 'linear' / 'nn' (``sx_cem_rollout_feat_multi``), or
    MC-dropout ensembles (``sx_cem_rollout_mlp_multi``); the last two share their architecture too, and have no elite-row
    form (the ranking kernel refits).

    Problem e keeps a ``FusedCemMpc`` (built here from the same settings with seed ``seed + e`` unless given), which also
    supplies its warm start.  The single launch does not apply to mixed families, JunkDimensionsSSM and step-by-step
    models, differing architectures and an exact-GP training set that needs the workspace path.  The problems share `env`
    and the CEM settings; sharded (multi-GPU) multi-model solves are out of scope.

    Solvers built with ``cost_on_safety=True`` carry their ``SaturatingCost`` into the launch (``sx_cem_rollout_sat_multi`` /
    ``sx_cem_rollout_elites_sat_multi``): equal costs on all solvers, or none on any of them.  Solvers with a constraint set
    (``con_set``) are refused here: ``MultiModelConsCemMpc`` solves those.
    """

    # what one launch needs of its solvers: compared at construction.  (The start distributions are the solvers' own:
    # `solve` takes problem e's from solvers[e].)
    _LAUNCH = (('time_horizon', '_horizon'), ('num_rollouts', '_num_rollouts'), ('num_elites', '_num_elites'),
               ('num_iterations', '_num_iterations'),
               ('the performance trajectory (n_perf, perf_r, perf_variance, perf_type, perf_terminal_safety)', perf_spec_of))
    # what the solvers of a front end's get_actions_multi share (`check_solvers`)
    _SHARED = (('the solver type', '__class__'),) + _LAUNCH + (
        ('warm_start', '_warm_start'), ('device', '_device'), ('the world size', '_world'),
        ('cost_on_safety', '_cost_on_safety'), ('init_std', '_init_std'), ('the environment constants (sx_env)', '_env'))
    _POLICY = SharedPolicy('a multi-model solve', label='the CEM settings (horizon, rollouts, elites, iterations, initial '
                           'distribution, device, the performance trajectory\'s n_perf, perf_r, perf_variance, perf_type, '
                           'perf_terminal_safety, and cost_on_safety) and the environment constants; of these, ')
    _FORM = 'sx_cem_rollout_multi_form'     # the form query of exact RBF GPs: < 0 where they have no single launch
    # the kernel-form cost: equal on all solvers or on none, compared before every solve
    _COST = (('the cost (equal costs on all of the solvers, or none on any of them)', '_cost'),)

    def __init__(self, ssms: Sequence[GpCemSSM], env: _lib.SxEnv, time_horizon: int, num_rollouts: int, num_elites: int,
                 num_iterations: int, *, device=None, seed: int = 0, init_std=1.0, warm_start: str = 'zero',
                 process_group=None, solvers: Optional[Sequence[FusedCemMpc]] = None):
        if process_group is not None:
            raise ValueError('MultiModelCemMpc solves on one GPU: sharded multi-model solves are not supported')
        self._ssms = list(ssms)
        if not self._ssms:
            raise ValueError('MultiModelCemMpc needs at least one model')
        if len({(s.num_states, s.num_actions) for s in self._ssms}) != 1:
            raise ValueError('the models of a multi-model solve must share (n_s, n_u)')
        if solvers is None:
            solvers = [FusedCemMpc(ssm, env, time_horizon, num_rollouts, num_elites, num_iterations, device=device,
                                   seed=seed + e, init_std=init_std, warm_start=warm_start)
                       for e, ssm in enumerate(self._ssms)]
        super().__init__(solvers, multi_family(self._ssms), self._LAUNCH)
        first = self._solvers[0]
        if (len(self._solvers) != len(self._ssms) or any(s._sharded for s in self._solvers)
                or (first._horizon, first._num_rollouts, first._num_elites, first._num_iterations)
                != (time_horizon, num_rollouts, num_elites, num_iterations)):
            raise ValueError(f'{len(self._solvers)} solvers for {len(self._ssms)} models: one per model, unsharded, with this '
                             f'solve\'s horizon, particles, elites and iterations')
        self._check_trajectories()
        self._horizon = time_horizon
        self._num_elites = num_elites
        self._num_iterations = num_iterations
        self._solver_cost()

    def _check_trajectories(self) -> None:
        """The trajectories of the solvers this class solves over: the safety trajectory alone."""
        if any(perf_spec_of(s).on for s in self._solvers):
            raise NotImplementedError('MultiModelCemMpc solves have no performance trajectory (solvers with n_perf > 0): '
                                      'MultiModelPerfCemMpc solves those')

    def _solver_cost(self):
        """The kernel-form cost of the solve: the solvers' (`FusedCemMpc.set_cost`), equal on all of them or on none."""
        _compare_settings(self._solvers, self._COST, self._POLICY.what)
        return getattr(self._solvers[0], '_cost', None)

    def _shared_set(self):
        """The solvers' constraint set as the rollout call takes it: none here (MultiModelConsCemMpc: the set)."""
        return None

    @classmethod
    def from_solvers(cls, solvers: Sequence[FusedCemMpc]) -> 'MultiModelCemMpc':
        """The multi-model solve over existing single-model solvers, solvers[e] for problem e, with their settings (which
        `check_solvers` compares)."""
        first = solvers[0]
        return cls([s._ssm for s in solvers], first._env, first._horizon, first._num_rollouts, first._num_elites,
                   first._num_iterations, device=first._device, solvers=solvers)

    def fused_applies(self) -> bool:
        """Does one multi-model launch serve the models?  Exact RBF GPs without the workspace path
        (sx_cem_rollout_multi_form); feature-space GPs or MC-dropout ensembles of one shape and architecture (the sign of
        sx_feat_model_table_bytes / sx_mlp_model_table_bytes).  Host only."""
        family = multi_family(self._ssms)
        if family is None:
            return False
        models = model_array(self._ssms, family)
        if family == 'rbf':
            return int(getattr(_lib.lib(), self._FORM)(models, len(self._ssms), self._horizon)) >= 0
        return model_table_bytes(models, family) >= 0

    def _begin(self, x0: Tensor, noise: Optional[Tensor]):
        """What opens a solve: x0's shape, then per problem e what solvers[e] would draw and start from alone -- its noise
        (unless given) and its start distribution -- and a status word.  Returns (noise, mean, std, status)."""
        E, n_s = len(self._ssms), self._ssms[0].num_states
        if x0.shape != (E, n_s):
            raise ValueError(f'x0 must be [{E} x {n_s}], got {tuple(x0.shape)}')
        if noise is None:
            noise = torch.stack([s._next_noise(1)[:, 0] for s in self._solvers], dim=1)
        self._last_noise = noise
        starts = [s.start_distribution(x0[e:e + 1]) for e, s in enumerate(self._solvers)]
        mean, std = torch.cat([m for m, _ in starts]), torch.cat([sd for _, sd in starts])
        return noise, mean, std, torch.zeros(E, dtype=torch.int32, device=x0.device)

    def solve(self, x0: Tensor, noise: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """E = len(models) solves from x0 [E x n_s] (points) in one launch per step of the loop.  Nothing synchronises.
        noise: optional [iters x E x P x H x n_u] standard normals; by default problem e draws from solvers[e].
        Returns (best [E x H x n_u], best_ok int32 [E], status int32 [E]: one word per problem).
        Raises FusedMultiUnsupported (before any launch) where the single launch does not apply."""
        E, H, n_u = len(self._ssms), self._horizon, self._ssms[0].num_actions
        noise, mean, std, status = self._begin(x0, noise)
        # (solver 0 stands for all: the solvers share this solve's settings, and a model on the workspace path has no
        # multi-model launch at all)
        in_prologue = self._solvers[0]._refit_in_prologue(E)
        # the solvers' cost where it prices the safety trajectory (cost_on_safety): it rides in the rollout call
        cost = self._solver_cost() if getattr(self._solvers[0], '_cost_on_safety', False) else None
        cost_kw = dict({} if cost is None else dict(cost=cost), **_con_set_kw(self._shared_set()))

        def rollout(it, mean, std, rows):
            return cem_rollout_multi(self._ssms, self._env, x0, H, mean=mean, std=std, elite_rows=rows,
                                     noise=noise[it].contiguous(), status=status, table=self._table, **cost_kw)

        def rank(it, r):
            return cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['actions'], self._num_elites, want_rows=in_prologue,
                                      want_refit=not in_prologue)

        out = _cem_iterations(self._num_iterations, rollout, rank, mean, std)
        return out['best'].view(E, H, n_u), out['best_ok'], status

    def get_actions_multi(self, states: Tensor, where: str = 'get_actions_multi') -> Tuple[Tensor, Tensor]:
        """Flat start states [E x (n_s + n_s^2)], all points, problem e for model e.  Returns (actions [E x H x n_u] on the
        host, found bool [E] on the host); ``found[e] == False`` is the ``get_actions`` ``None`` of problem e.  Raises like
        ``FusedCemMpc.get_actions`` if any problem hit a numerical failure; the step-by-step repeat of a solve that reports
        both SX_STATUS_NAN and SX_STATUS_ZERO_FIX is made for that problem only."""
        self._solver_cost()      # mixed costs raise before anything is solved, one model at a time included
        return self._get_actions_multi(states, where)


class MultiModelConsCemMpc(MultiModelCemMpc):
    """``MultiModelCemMpc`` over solvers with a constraint set (``FusedCemMpc(con_set=...)``): E
    exact RBF GPs whose solvers carry ONE set -- the scenarios share the environment, and so its obstacle rows and feedback
    bounds.  An iteration is ``sx_cem_rollout_cons_multi`` / ``sx_cem_rollout_elites_cons_multi`` (with the solvers'
    ``cost_on_safety`` cost where they have one) and the ranking launch, as in the parent.  The per-problem step-by-step
    repeat of ``_check_solve`` and the one-solve-per-model fallback (a training set on the workspace path) are the
    solvers' own, which carry the set already.
    """
    _POLICY = MultiModelCemMpc._POLICY._replace(con_set='all')
    _FORM = 'sx_cem_rollout_cons_multi_form'

    def __init__(self, ssms: Sequence[GpCemSSM], env: _lib.SxEnv, time_horizon: int, num_rollouts: int, num_elites: int,
                 num_iterations: int, *, con_set=None, device=None, seed: int = 0, init_std=1.0, warm_start: str = 'zero',
                 process_group=None, solvers: Optional[Sequence[FusedCemMpc]] = None):
        if process_group is not None:
            raise NotImplementedError('con_set is not built for sharded particles (a process group)')
        if solvers is None:
            if con_set is None:
                raise ValueError('MultiModelConsCemMpc needs a constraint set (con_set); MultiModelCemMpc solves without one')
            solvers = [FusedCemMpc(ssm, env, time_horizon, num_rollouts, num_elites, num_iterations, device=device,
                                   seed=seed + e, init_std=init_std, warm_start=warm_start, con_set=con_set)
                       for e, ssm in enumerate(ssms)]
        super().__init__(ssms, env, time_horizon, num_rollouts, num_elites, num_iterations, device=device, seed=seed,
                         init_std=init_std, warm_start=warm_start, solvers=solvers)
        if con_set is not None and bytes(con_set) != bytes(self._solvers[0]._con_set):
            raise ValueError('the solvers carry another constraint set than the con_set given')
        _require_exact_rbf(self._ssms, _CON_SET_IS)

    def _shared_set(self):
        return _shared_con_set(self._solvers, 'all', self._POLICY.what)



class MultiModelPerfCemMpc(MultiModelCemMpc):
    """``MultiModelCemMpc`` over solvers with a performance trajectory (``FusedCemMpc(n_perf > 0)``, DESIGN.md section
    3.9): E exact RBF GPs whose solvers share ``n_perf``, ``perf_r``, ``perf_variance``, ``perf_type`` and
    ``perf_terminal_safety``.  An iteration is ``sx_cem_rollout_multi`` over the first H steps of the rows, ONE
    performance-rollout launch for all problems (``sx_cem_perf_rollout_multi``, ``sx_cem_perf_rollout_var_multi`` with
    ``perf_variance``, or ``sx_cem_perf_rollout_taylor_multi`` with ``perf_type='taylor'``) and the ranking over the rows
    of H + T steps, T = n_perf - perf_r; the ranking launch refits (no prologue refit, as in ``FusedCemMpc.solve`` with a
    performance trajectory).  Problem e draws solvers[e]'s noise and start distribution, which have row length.
    ``get_actions_multi`` returns the H safety actions and leaves the tail in every solver's ``last_perf_actions``.
    Where either launch has no form for the models (``fused_applies`` is False) the problems are solved one model at a
    time (``per_model_solves``).
    """
    def __init__(self, ssms: Sequence[GpCemSSM], env: _lib.SxEnv, time_horizon: int, num_rollouts: int, num_elites: int,
                 num_iterations: int, *, n_perf: Optional[int] = None, perf_r: int = 1, perf_variance: bool = False,
                 device=None, seed: int = 0, init_std=1.0, warm_start: str = 'zero', process_group=None,
                 solvers: Optional[Sequence[FusedCemMpc]] = None, perf_type: str = 'mean_equivalent',
                 perf_terminal_safety: bool = False):
        if process_group is not None:
            raise NotImplementedError('the performance trajectory is not built for sharded particles (a process group)')
        if solvers is None:
            if not n_perf or n_perf <= 0:
                raise ValueError('MultiModelPerfCemMpc needs a performance trajectory (n_perf > 0); MultiModelCemMpc solves '
                                 'without one')
            solvers = [FusedCemMpc(ssm, env, time_horizon, num_rollouts, num_elites, num_iterations, device=device,
                                   seed=seed + e, init_std=init_std, warm_start=warm_start, n_perf=n_perf, perf_r=perf_r,
                                   perf_variance=perf_variance, perf_type=perf_type,
                                   perf_terminal_safety=perf_terminal_safety) for e, ssm in enumerate(ssms)]
        super().__init__(ssms, env, time_horizon, num_rollouts, num_elites, num_iterations, device=device, seed=seed,
                         init_std=init_std, warm_start=warm_start, solvers=solvers)
        self._perf = perf_spec_of(self._solvers[0])     # (the base has compared the solvers' specs)
        if n_perf is not None and (int(n_perf), int(perf_r), bool(perf_variance)) != self._perf[:3]:
            raise ValueError(f'the solvers have (n_perf, perf_r, perf_variance) = {tuple(self._perf[:3])}'
                             f', not {(n_perf, perf_r, perf_variance)}')
        _require_exact_rbf(self._ssms, 'the performance trajectory is', numbered=True)
        # the device table the performance launch reads: alpha per model for the mean-only form, else the safety launch's
        self._perf_table = PerfModelTable() if self._perf.kind == 'mean' else self._table

    def _check_trajectories(self) -> None:
        """The solvers carry a performance trajectory, and no objective hook that would have to be evaluated."""
        if not perf_spec_of(self._solvers[0]).on:
            raise ValueError('MultiModelPerfCemMpc needs solvers with a performance trajectory (n_perf > 0); '
                             'MultiModelCemMpc solves the others')
        if any(getattr(s, '_objective_hook', None) is not None and getattr(s, '_cost', None) is None for s in self._solvers):
            raise NotImplementedError('a multi-model solve with a performance trajectory has no objective hook: solvers '
                                      'with one act one at a time (get_actions)')

    def set_env(self, env: _lib.SxEnv, objective_hook=None) -> None:
        if objective_hook is not None:
            raise NotImplementedError('a multi-model solve with a performance trajectory has no objective hook')
        super().set_env(env)

    def fused_applies(self) -> bool:
        """Does one launch of each kind serve the models?  The safety rollout as in `MultiModelCemMpc`, and the Taylor or
        the variance form of the performance rollout where its form query answers (sx_cem_perf_rollout_taylor_multi_form,
        sx_cem_perf_rollout_var_multi_form).  The mean-only form adds no condition: it stages (2 n_s + n_u) N doubles in
        LDS, which holds every training set the multi-model safety rollout takes (n_pad <= 1024).  Host only."""
        if not super().fused_applies():
            return False
        return self._perf.kind == 'mean' or self._perf_form() >= 0

    def _perf_form(self) -> int:
        """sx_cem_perf_rollout_{var,taylor}_multi_form of the models: < 0 where they have no single launch.  Host only."""
        query = {'variance': 'sx_cem_perf_rollout_var_multi_form', 'taylor': 'sx_cem_perf_rollout_taylor_multi_form'}
        models = model_array(self._ssms, 'rbf')
        return int(getattr(_lib.lib(), query[self._perf.kind])(models, len(self._ssms), self._perf.n_perf))

    def solve(self, x0: Tensor, noise: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """As `MultiModelCemMpc.solve` with rows of H + T steps: noise [iters x E x P x (H + T) x n_u], and the returned
        best rows [E x (H + T) x n_u] carry the tail behind the safety actions."""
        perf = self._perf
        E, H, T, n_u = len(self._ssms), self._horizon, perf.tail, self._ssms[0].num_actions
        cost = self._solver_cost()
        if perf.kind == 'taylor' and self._perf_form() < 0:
            raise FusedMultiUnsupported(f"perf_type='taylor' has no multi-model launch for these models (N = "
                                        f'{[ssm.device_model.n_train for ssm in self._ssms]}, n_perf = {perf.n_perf}): '
                                        f'the solvers act one model at a time')
        noise, mean, std, status = self._begin(x0, noise)
        noise_safe, noise_tail = noise[:, :, :, :H].contiguous(), noise[:, :, :, H:].contiguous()

        def rollout(it, mean, std, rows):
            r = cem_rollout_multi(self._ssms, self._env, x0, H, mean=mean[:, :H].contiguous(), std=std[:, :H].contiguous(),
                                  noise=noise_safe[it], status=status, table=self._table)
            pr = _launch_perf(perf, self._ssms, self._env, x0, H, r, mean, std, noise_tail[it], status, multi=True,
                              table=self._perf_table, cost=cost)
            return dict(actions=pr['rows'], obj_cost=pr['obj_cost'], con_cost=pr['con_cost'])

        def rank(it, r):
            return cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['actions'], self._num_elites)

        out = _cem_iterations(self._num_iterations, rollout, rank, mean, std)
        return out['best'].view(E, H + T, n_u), out['best_ok'], status

    def get_actions_multi(self, states: Tensor, where: str = 'get_actions_multi') -> Tuple[Tensor, Tensor]:
        """As `MultiModelCemMpc.get_actions_multi`: the H safety actions of every problem's best row; the row's tail
        [1 x T x n_u] becomes solvers[e].last_perf_actions."""
        self._solver_cost()      # mixed costs raise before anything is solved, one model at a time included
        best, found = super().get_actions_multi(states, where)
        if best.size(1) != self._horizon:      # (a solve per model has cut its rows already)
            for e, s in enumerate(self._solvers):
                s.last_perf_actions = best[e:e + 1, self._horizon:]
            best = best[:, :self._horizon]
        return best, found


class StaticCemMpc:
    """The CEM solver of static exploration: the start state is a decision variable of every particle (the reference's
    ``StaticSafeMPCExploration`` NLP over ``[p_0, u_0, k_ff]``, safempc_exploration.py:56-334; DESIGN.md sections 3.10, 5).

    The CEM row is ``[x0 (n_s) | u_0 .. u_{H-1}]`` with one Gaussian per entry, started from ``[start_mean | 0]`` and
    ``[start_std | init_std]``.  An iteration is ``sx_cem_rollout_starts`` and one ranking launch over the long rows, which
    also refits them.  The objective is always the variance objective (SX_OBJ_NEG_VARIANCE); constraints are the
    environment's own plus SX_STATE_VIOLATION_COST for a start outside the safe polytope.  ``n_restarts`` problems with the
    same start distribution and their own draws (seed + e) run in the same launches; ``find`` answers with the feasible one
    of lowest objective.  Exact RBF GPs on one GPU only.

    ``con_set`` (an ``_lib.SxConSet``, ``make_con_set``; DESIGN.md section 3.10, "the constraint set") adds the constraints of
    the reference's static NLP, whose gain is a fixed parameter: an iteration is then ``sx_cem_rollout_starts_cons``.  The
    rule, the same in the fused and the step-by-step rollout: a particle starts from a point, so step 0 pays the action box
    alone; a step t >= 1 pays SX_ACTION_VIOLATION_COST once where its action leaves the box or its control ellipsoid
    (u_t, K Q_t K^T) is not certified inside it; every (p_{t+1}, Q_{t+1}) with t + 1 < H pays SX_STATE_VIOLATION_COST where it
    is not certified inside the obstacle rows; and a start that violates the obstacle rows pays SX_STATE_VIOLATION_COST once,
    beside and independent of the safe-polytope cost of the start (a start outside both pays 20).
    """

    def __init__(self, ssm: GpCemSSM, env: _lib.SxEnv, time_horizon: int, num_rollouts: int, num_elites: int,
                 num_iterations: int, *, start_mean, start_std, n_restarts: int = 1, seed: int = 0, init_std=1.0,
                 device=None, record_rollouts: bool = False, process_group=None, con_set=None):
        self._con_set = _checked_con_set(con_set, ssm)
        _require_exact_rbf([ssm], 'static exploration is')
        if process_group is not None:
            raise NotImplementedError('static exploration is not built for sharded particles (a process group)')
        n_s, n_u = ssm.num_states, ssm.num_actions
        if n_restarts < 1:
            raise ValueError(f'n_restarts={n_restarts} must be at least 1')
        check_rank_limits(num_rollouts, num_elites, num_rollouts)
        self._ssm = ssm
        self._horizon, self._num_rollouts, self._num_elites = time_horizon, num_rollouts, num_elites
        self._num_iterations, self._restarts, self._record = num_iterations, int(n_restarts), record_rollouts
        self._row_len = n_s + time_horizon * n_u
        self._device = torch.device(device if device is not None else 'cuda:0')
        as_row = lambda v, n: torch.as_tensor(v, dtype=torch.float64).reshape(-1).expand(n).clone()
        # the first iteration's distribution of the row: [start_mean | 0], [start_std | init_std]
        self._mean0 = torch.cat([as_row(start_mean, n_s), torch.zeros(time_horizon * n_u, dtype=torch.float64)])
        self._std0 = torch.cat([as_row(start_std, n_s), expand_init_std(init_std, time_horizon, n_u).reshape(-1)])
        self._mean0, self._std0 = self._mean0.to(self._device), self._std0.to(self._device)
        self._seed = int(seed)
        self._gens = None       # one generator per restart (seed + e), made with the first draw
        self.set_env(env)
        self.last_status = 0
        self.stepwise_fallbacks = 0
        self._last_noise = None
        self.last_rows = None           # [E x L] on the host: every restart's best row of the last `find`
        self.last_costs = None          # [E x 2] on the host: their (con, obj)
        self.last_choice = None         # the restart `find` chose, or None

    @property
    def num_iterations(self) -> int:
        return self._num_iterations

    @property
    def n_restarts(self) -> int:
        return self._restarts

    def set_env(self, env: _lib.SxEnv) -> None:
        """New problem constants.  The solver keeps a copy of them with the variance objective: static exploration looks for
        where the model is uncertain (the reference's `cost_func is None` branch, safempc_exploration.py:140-141)."""
        self._env = _lib.SxEnv.from_buffer_copy(env)
        self._env.obj_mode = _lib.SX_OBJ_NEG_VARIANCE

    def sample_noise(self) -> Tensor:
        """[iters x E x P x L] standard normals of one solve: restart e draws from its own generator (seed + e)."""
        if self._gens is None:
            self._gens = []
            for e in range(self._restarts):
                self._gens.append(torch.Generator(device=self._device))
                self._gens[-1].manual_seed(self._seed + e)
        shape = (self._num_iterations, self._num_rollouts, self._row_len)
        return torch.stack([torch.randn(shape, dtype=torch.float64, device=self._device, generator=g) for g in self._gens],
                           dim=1)

    def _rollout_stepwise(self, mean: Tensor, std: Tensor, eps: Tensor, status: Tensor):
        """One iteration's rollout through `cem_rollout_stepwise` with a start per particle, restart by restart; with a
        constraint set the steps are charged by sx_conset_eval and the start by `start_obstacle_cost`."""
        n_s, n_u = self._ssm.num_states, self._ssm.num_actions
        rows = (mean.unsqueeze(1) + std.unsqueeze(1) * eps).contiguous()       # [E x P x L]
        obj, con = [], []
        for e in range(rows.size(0)):
            x0 = rows[e, :, :n_s].contiguous()
            acts = rows[e, :, n_s:].reshape(-1, self._horizon, n_u).contiguous()
            r = cem_rollout_stepwise(self._ssm, self._env, x0, acts, status=status, **_con_set_kw(self._con_set))
            obj.append(r['obj_cost'])
            start = start_constraint_cost(self._env, x0)
            if self._con_set is not None:
                start = start + start_obstacle_cost(self._env, self._con_set, x0)
            con.append(r['con_cost'] + start)
        return dict(rows=rows, traj=None, obj_cost=torch.stack(obj), con_cost=torch.stack(con))

    def solve(self, noise: Optional[Tensor] = None, stepwise: bool = False):
        """The n_restarts solves, in the same launches.  Nothing here synchronises with the host.

        noise: optional [iters x E x P x L] pre-drawn standard normals (parity tests inject them).
        Returns (best [E x L]: every restart's first-ranked row of the last iteration, costs [E x 2]: its (con, obj),
        best_ok int32 [E], rollouts per iteration (if recorded), status int32 [1])."""
        E, P, L, dev = self._restarts, self._num_rollouts, self._row_len, self._device
        if noise is None:
            noise = self.sample_noise()
        if tuple(noise.shape) != (self._num_iterations, E, P, L):
            raise ValueError(f'noise must be [{self._num_iterations} x {E} x {P} x {L}], got {tuple(noise.shape)}')
        self._last_noise = noise
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        history: List[Rollouts] = []
        n_s, n_u = self._ssm.num_states, self._ssm.num_actions
        mean = self._mean0.expand(E, L).contiguous()
        std = self._std0.expand(E, L).contiguous()

        def rollout(it, mean, std, rows):
            eps = noise[it].contiguous()
            if stepwise:
                return self._rollout_stepwise(mean, std, eps, status)
            r = cem_rollout_starts(self._ssm, self._env, self._horizon, mean=mean, std=std, noise=eps,
                                   want_traj=self._record, status=status, **_con_set_kw(getattr(self, '_con_set', None)))
            if self._record:
                for e in range(E):
                    history.append(Rollouts(r['traj'][e], r['rows'][e, :, n_s:].reshape(P, self._horizon, n_u),
                                            r['obj_cost'][e], r['con_cost'][e]))
            return r

        def rank(it, r):
            # the ranking launch refits the long rows; the last one also hands back the elite rows, whose first is the best
            # row with its (con, obj)
            return cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['rows'], self._num_elites,
                                      want_rows=it == self._num_iterations - 1, want_refit=True)

        out = _cem_iterations(self._num_iterations, rollout, rank, mean, std)
        costs = out['elite_rows'][:, 0, :2]
        return out['best'].view(E, L), costs, out['best_ok'], history, status

    @staticmethod
    def choose(found, objectives) -> Optional[int]:
        """The restart whose answer is kept: feasible, lowest objective, lowest index on a tie; None if none is feasible."""
        chosen = None
        for e, (ok, obj) in enumerate(zip(found, objectives)):
            if bool(ok) and (chosen is None or float(obj) < float(objectives[chosen])):
                chosen = e
        return chosen

    def find(self, noise: Optional[Tensor] = None):
        """(x0 [n_s], actions [H x n_u], objective) of the best feasible restart on the host, or None where no restart
        found a feasible row.  One device -> host hand-off; a NaN raises as `FusedCemMpc.get_actions` does, and a solve
        whose status has both SX_STATUS_NAN and SX_STATUS_ZERO_FIX is repeated step by step with the same draws."""
        n_s, n_u, E, L = self._ssm.num_states, self._ssm.num_actions, self._restarts, self._row_len
        best, costs, best_ok, history, status = self.solve(noise)
        # the rows travel with their (con, obj): [E x (L + 2)] in the one hand-off
        words, found, _, host = _hand_off(self, torch.cat([best, costs], dim=1), best_ok, status, None)
        st = fold_status(words)
        both = _lib.SX_STATUS_NAN | _lib.SX_STATUS_ZERO_FIX
        if (st & both) == both:
            # the reference's whole-batch zero fix-up (see _check_solve): the same draws, step by step
            self.stepwise_fallbacks += 1
            best, costs, best_ok, history, status = self.solve(self._last_noise, stepwise=True)
            words, found, _, host = _hand_off(self, torch.cat([best, costs], dim=1), best_ok, status, None)
            st = fold_status(words)
        self.last_status = st
        self.last_rollouts = history
        raise_for_status(st, 'StaticCemMpc.find', dump=lambda: save_failure_state(self._ssm, self._mean0[:n_s], None))
        self.last_rows, self.last_costs = host[:, :L], host[:, L:]
        self.last_choice = e = self.choose(found, host[:, L + 1])
        if e is None:
            return None
        return host[e, :n_s].clone(), host[e, n_s:L].reshape(self._horizon, n_u).clone(), float(host[e, L + 1])


class MultiModelStaticCemMpc(MultiModelCem):
    """S independent static-exploration problems with an exact GP each -- the reference's scenarios, one model per scenario
    (sacred_helper.py's n_scenarios runs of StaticSafeMPCExploration) -- solved together: scenario s with its R restarts is
    the problems e = s R .. s R + R - 1 of ONE ``sx_cem_rollout_starts_multi`` launch (``sx_cem_rollout_starts_cons_multi``
    where the solvers carry a constraint set) and one ranking launch per CEM iteration, where ``StaticCemMpc`` needs a
    solve per scenario ("the multi-model form").

    Scenario s keeps its ``StaticCemMpc`` (``solvers[s]``): it supplies the scenario's start distribution (rows of the
    [E x L] mean and std, so the scenarios' may differ) and noise draws (``sample_noise()``: its generators advance exactly
    as in a solve of its own), decides among its restarts (``StaticCemMpc.choose``), takes the step-by-step repeat of a
    scenario whose status has SX_STATUS_NAN | SX_STATUS_ZERO_FIX, and solves alone where the models have no single launch
    (``fused_applies``).  The solvers share (n_s, n_u), the horizon, particles, elites, iterations, restarts, the device, ONE
    sx_env (byte for byte) and ONE constraint set (or none); ``check_solvers`` runs before every ``solve`` and ``find``."""

    _SHARED = (('(n_s, n_u)', _model_shape), ('time_horizon', '_horizon'), ('num_rollouts', '_num_rollouts'),
               ('num_elites', '_num_elites'), ('num_iterations', '_num_iterations'), ('n_restarts', '_restarts'),
               ('device', '_device'), ('record_rollouts', '_record'),
               ('the environment constants (env: one sx_env)', '_env'))
    _POLICY = SharedPolicy('a multi-model static solve', con_set='all_or_none', exact_rbf=True)

    @classmethod
    def from_solvers(cls, solvers: Sequence[StaticCemMpc]) -> 'MultiModelStaticCemMpc':
        """The multi-model solve over existing single-model solvers, solvers[s] for scenario s, with their settings (which
        `check_solvers` compares)."""
        return cls(solvers)

    def _models(self) -> List[GpCemSSM]:
        """The model of every problem: scenario s's, once per restart."""
        return [s._ssm for s in self._solvers for _ in range(s._restarts)]

    def form(self) -> int:
        """sx_cem_rollout_starts_multi_form of the problems' models: < 0 where they have no single launch.  Host only."""
        ssms = self._models()
        return int(_lib.lib().sx_cem_rollout_starts_multi_form(model_array(ssms, 'rbf'), len(ssms),
                                                               self._solvers[0]._horizon))

    def fused_applies(self) -> bool:
        """Does one launch serve all scenarios (`form`)?  Host only."""
        return self.form() >= 0

    def sample_noise(self) -> Tensor:
        """[iters x S R x P x L]: every solver's own `sample_noise()`, along the problem axis."""
        return torch.cat([s.sample_noise() for s in self._solvers], dim=1)

    def solve(self, noise: Optional[Tensor] = None):
        """The S R solves in the same launches.  Nothing here synchronises with the host.
        noise: optional [iters x S R x P x L] standard normals; by default scenario s draws ``solvers[s].sample_noise()``.
        Returns (best [E x L], costs [E x 2]: (con, obj) of the best rows, best_ok int32 [E], per scenario the rollouts per
        iteration (if recorded), status int32 [E]: one word per problem).
        Raises FusedMultiUnsupported (before any launch) where the single launch does not apply."""
        self.check_solvers(self._solvers)
        first = self._solvers[0]
        S, R, P, L, dev = len(self._solvers), first._restarts, first._num_rollouts, first._row_len, first._device
        E, H, k, iters = S * R, first._horizon, first._num_elites, first._num_iterations
        if noise is None:
            noise = self.sample_noise()
        if tuple(noise.shape) != (iters, E, P, L):
            raise ValueError(f'noise must be [{iters} x {E} x {P} x {L}], got {tuple(noise.shape)}')
        for s, m in enumerate(self._solvers):
            m._last_noise = noise[:, s * R:(s + 1) * R]
        ssms = self._models()
        n_s, n_u = ssms[0].num_states, ssms[0].num_actions
        mean = torch.cat([m._mean0.expand(R, L) for m in self._solvers]).contiguous()
        std = torch.cat([m._std0.expand(R, L) for m in self._solvers]).contiguous()
        status = torch.zeros(E, dtype=torch.int32, device=dev)
        histories: List[List[Rollouts]] = [[] for _ in range(S)]
        con_kw = _con_set_kw(getattr(first, '_con_set', None))

        def rollout(it, mean, std, rows):
            r = cem_rollout_starts_multi(ssms, first._env, H, mean=mean, std=std, noise=noise[it].contiguous(),
                                         want_traj=first._record, status=status, table=self._table, **con_kw)
            if first._record:
                for e in range(E):
                    histories[e // R].append(Rollouts(r['traj'][e], r['rows'][e, :, n_s:].reshape(P, H, n_u),
                                                      r['obj_cost'][e], r['con_cost'][e]))
            return r

        def rank(it, r):
            return cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['rows'], k, want_rows=it == iters - 1,
                                      want_refit=True)

        out = _cem_iterations(iters, rollout, rank, mean, std)
        return out['best'].view(E, L), out['elite_rows'][:, 0, :2], out['best_ok'], histories, status

    def find(self, noise: Optional[Tensor] = None) -> list:
        """Entry s is what ``solvers[s].find(noise_s)`` returns -- (x0 [n_s], actions [H x n_u], objective) of the scenario's
        best feasible restart on the host, or None -- and solver s holds the scenario's `last_rows`, `last_costs`,
        `last_choice` and `last_status`.  ONE device -> host hand-off for all scenarios.  A scenario whose status words carry
        SX_STATUS_NAN | SX_STATUS_ZERO_FIX is repeated alone, step by step, with its own draws; a NaN raises as
        `StaticCemMpc.find` does, naming the scenario.  Where the models have no single launch (`fused_applies`), the
        scenarios are solved one by one with the same noise."""
        self.check_solvers(self._solvers)
        first = self._solvers[0]
        S, R, L, H = len(self._solvers), first._restarts, first._row_len, first._horizon
        n_s, n_u = first._ssm.num_states, first._ssm.num_actions
        if noise is None:
            noise = self.sample_noise()
        if not self.fused_applies():
            self.per_model_solves += 1
            return [m.find(noise[:, s * R:(s + 1) * R].contiguous()) for s, m in enumerate(self._solvers)]
        best, costs, best_ok, histories, status = self.solve(noise)
        words, found, _, host = _hand_off(self, torch.cat([best, costs], dim=1), best_ok, status, None)
        both = _lib.SX_STATUS_NAN | _lib.SX_STATUS_ZERO_FIX
        for s, m in enumerate(self._solvers):
            sl = slice(s * R, (s + 1) * R)
            st = fold_status(words[sl])
            if (st & both) == both:
                # (as StaticCemMpc.find: the reference's whole-batch zero fix-up, for this scenario only)
                self.stepwise_fallbacks += 1
                m.stepwise_fallbacks += 1
                b, c, ok, histories[s], st_s = m.solve(noise[:, sl].contiguous(), stepwise=True)
                w, found[sl], _, host[sl] = _hand_off(m, torch.cat([b, c], dim=1), ok, st_s, None)
                st = fold_status(w)
            m.last_status = st
            m.last_rollouts = histories[s]
        answers = []
        for s, m in enumerate(self._solvers):
            sl = slice(s * R, (s + 1) * R)
            raise_for_status(m.last_status, f'MultiModelStaticCemMpc.find (scenario {s})',
                             dump=lambda m=m: save_failure_state(m._ssm, m._mean0[:n_s], None))
            rows = host[sl].clone()
            m.last_rows, m.last_costs = rows[:, :L], rows[:, L:]
            m.last_choice = e = StaticCemMpc.choose(found[sl], rows[:, L + 1])
            answers.append(None if e is None else (rows[e, :n_s].clone(), rows[e, n_s:L].reshape(H, n_u).clone(),
                                                   float(rows[e, L + 1])))
        return answers


# ---- Cautious MPC ----------------------------------------------------------------------------------
def _cautious_rollout(entry: str, head: tuple, ssms: Sequence, x0: Tensor, T: int, words: int, unsupported, *, mean, std,
                      noise, rows, propagate, want_traj, want_sigma, want_cov, want_margins, status):
    """The buffers and the call of the cautious rollout entries: `head` are the entry's arguments in front of E (the model or
    models and table, env, the cost), `words` the status words of a fresh status, `unsupported(n_s, n_u)` what
    SX_ERR_UNSUPPORTED raises."""
    _require_rbf(ssms, x0)
    dev, n_s, n_u = x0.device, ssms[0].num_states, ssms[0].num_actions
    T = int(T)
    if T < 1:
        raise ValueError(f'the cautious rollout needs T >= 1 steps, got T={T}')
    if x0.dim() != 2 or x0.size(1) != n_s:
        raise ValueError(f'x0 must be [E x {n_s}], got {tuple(x0.shape)}')
    E = x0.size(0)
    if noise is not None:
        if rows is not None:
            raise ValueError('either noise (the rows are drawn) or rows (the rows are given), not both')
        if mean is None or std is None:
            raise ValueError('noise needs mean and std')
        if noise.dim() != 4 or tuple(noise.shape) != (E, noise.size(1), T, n_u) or not noise.is_contiguous():
            raise ValueError(f'noise must be a contiguous [{E} x P x {T} x {n_u}] tensor, got {tuple(noise.shape)}')
        for name, v in (('mean', mean), ('std', std)):
            if tuple(v.shape) != (E, T, n_u) or not v.is_contiguous():
                raise ValueError(f'{name} must be a contiguous [{E} x {T} x {n_u}] tensor, got {tuple(v.shape)}')
        P = noise.size(1)
        rows = torch.empty((E, P, T, n_u), dtype=torch.float64, device=dev)
    elif rows is None or rows.dim() != 4 or tuple(rows.shape) != (E, rows.size(1), T, n_u) or not rows.is_contiguous():
        raise ValueError(f'without noise, rows must be a contiguous [{E} x P x {T} x {n_u}] tensor')
    else:
        P = rows.size(1)
    new = lambda *shape: torch.empty((E, P, T) + shape, dtype=torch.float64, device=dev)
    traj = new(n_s) if want_traj else None
    sigma = new(n_s) if want_sigma else None
    cov = new(n_s, n_s) if want_cov else None
    margins = new(2) if want_margins else None
    obj = torch.empty((E, P), dtype=torch.float64, device=dev)
    con = torch.empty((E, P), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(words, dtype=torch.int32, device=dev)
    code = getattr(_lib.lib(), entry)(*head, E, P, T,
                                      _lib.ptr(x0.contiguous()), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(noise), _lib.ptr(rows),
                                      _lib.ptr(obj), _lib.ptr(con), _lib.ptr(traj), _lib.ptr(sigma), _lib.ptr(cov),
                                      _lib.ptr(margins), int(bool(propagate)), _lib.ptr(status), _lib.stream_ptr(dev))
    if code == _lib.SX_ERR_UNSUPPORTED:
        raise unsupported(n_s, n_u)
    _lib.check(code, entry)
    return dict(rows=rows, obj_cost=obj, con_cost=con, traj=traj, sigma=sigma, cov=cov, margins=margins, status=status)


def cem_cautious_rollout(ssm: GpCemSSM, env: _lib.SxEnv, x0: Tensor, T: int, *, mean: Optional[Tensor] = None,
                         std: Optional[Tensor] = None, noise: Optional[Tensor] = None, rows: Optional[Tensor] = None,
                         propagate: bool = True, want_traj: bool = False, want_sigma: bool = False, want_cov: bool = False,
                         want_margins: bool = False, status: Optional[Tensor] = None, cost=None):
    """Thin wrapper over sx_cem_cautious_rollout: the chance-constrained Taylor rollout of Cautious MPC (exact RBF GPs only).
    x0 [E x n_s]; the rows k_ff_0 .. k_ff_{T-1} either drawn (`mean`, `std` [E x T x n_u], `noise` [E x P x T x n_u]) or
    given as `rows` [E x P x T x n_u].  Every step adds SX_ACTION_VIOLATION_COST where the control k_ff_t +- env.beta
    sqrt(K_c Sigma_t K_c^T) leaves the action box (the plain box at t = 0) and SX_STATE_VIOLATION_COST where the ellipsoid
    (mu_{t+1}, env.beta, Sigma_{t+1}) leaves env's polytope; `propagate=False` starts every GP step from Sigma_t = 0 (the
    reference's 'mean_equivalent').  `cost` (a `costs.SaturatingCost`) selects sx_cem_cautious_rollout_sat: obj_cost is the
    sum of the cost over (mu_{t+1}, Sigma_{t+1}) and env.obj_mode is not read; everything else is unchanged.
    Returns dict(rows, obj_cost [E x P], con_cost [E x P], traj [E x P x T x n_s] | None, sigma (same shape; diag G_t) | None,
    cov [E x P x T x n_s x n_s] | None, margins [E x P x T x 2] (largest state, largest control distance) | None, status)."""
    _require_rbf([ssm], x0)
    entry = 'sx_cem_cautious_rollout' + ('_sat' if cost is not None else '')
    head = (ctypes.byref(ssm.device_model), ctypes.byref(env)) + _cost_args(cost, ssm)
    return _cautious_rollout(entry, head, [ssm], x0, T, 1, _no_form(entry, 'cautious', ssm, int(T)), mean=mean, std=std,
                             noise=noise, rows=rows, propagate=propagate, want_traj=want_traj, want_sigma=want_sigma,
                             want_cov=want_cov, want_margins=want_margins, status=status)


def cem_cautious_rollout_multi(ssms: Sequence[GpCemSSM], env: _lib.SxEnv, x0: Tensor, T: int, *,
                               mean: Optional[Tensor] = None, std: Optional[Tensor] = None, noise: Optional[Tensor] = None,
                               rows: Optional[Tensor] = None, propagate: bool = True, want_traj: bool = False,
                               want_sigma: bool = False, want_cov: bool = False, want_margins: bool = False,
                               status: Optional[Tensor] = None, table: Optional[GpModelTable] = None, cost=None):
    """`cem_cautious_rollout` for E problems with an exact GP each (ssms[e] for problem e) in one launch
    (sx_cem_cautious_rollout_multi; with `cost` sx_cem_cautious_rollout_sat_multi).  There is one `env` -- the feedback gain,
    the action box, the polytope and beta are the same for all problems -- and one `cost`.  Buffers as in the single-model
    wrapper, per problem; `status` is int32 [E], one word per problem.  `table` keeps the device table between calls: the
    `GpModelTable` of `cem_rollout_multi` (a fresh one is built otherwise).  Raises FusedMultiUnsupported where the library
    has no single launch for the models (before any launch)."""
    entry = 'sx_cem_cautious_rollout' + ('_sat' if cost is not None else '') + '_multi'
    _require_rbf(ssms, x0)
    if x0.dim() != 2 or len(ssms) != x0.size(0):
        raise ValueError(f'{len(ssms)} models for x0 of shape {tuple(x0.shape)}: one model per problem')
    E = x0.size(0)
    if status is not None and status.numel() != E:
        raise ValueError(f'status must hold one word per problem ({E}), got {status.numel()}')
    if not isinstance(table, GpModelTable) or table.family != 'rbf':
        table = GpModelTable()
    models, dev_table = table.get(ssms, x0.device)

    def unsupported(n_s, n_u):
        return FusedMultiUnsupported(f'{entry}: no single launch of the cautious rollout for these models ((n_s, n_u) = '
                                     f'({n_s}, {n_u}), N = {[ssm.device_model.n_train for ssm in ssms]}, T = {int(T)})')
    head = (models, _lib.ptr(dev_table), ctypes.byref(env)) + _cost_args(cost, ssms[0])
    return _cautious_rollout(entry, head, ssms, x0, T, E, unsupported, mean=mean, std=std, noise=noise, rows=rows,
                             propagate=propagate, want_traj=want_traj, want_sigma=want_sigma, want_cov=want_cov,
                             want_margins=want_margins, status=status)


class CautiousCemMpc:
    """The CEM solver of Cautious MPC (the reference's ``CautiousMPC`` NLP over ``k_ff``, cautious_mpc.py:136-200; DESIGN.md
    section 3.11): E independent problems, the row ``k_ff_0 .. k_ff_{T-1}`` with one Gaussian per entry.  An iteration is
    one ``sx_cem_cautious_rollout`` -- the Taylor trajectory (``propagate=False``: mean-equivalent) under the fixed gain
    ``env.k_fb`` with the chance constraints at ``env.beta`` on every step -- and one ranking launch, which also refits.
    ``env``'s polytope is the one the states are held in; its objective is the separable one or the variance objective, or
    an ``objective_hook`` evaluated on the recorded means.  Exact RBF GPs on one GPU only.
    """

    def __init__(self, ssm: GpCemSSM, env: _lib.SxEnv, time_horizon: int, num_rollouts: int, num_elites: int,
                 num_iterations: int, *, propagate: bool = True, device=None, seed: int = 0, init_std=1.0,
                 record_rollouts: bool = False, process_group=None):
        if isinstance(ssm, (list, tuple)):
            raise ValueError('CautiousCemMpc solves its problems over ONE model: MultiModelCautiousCemMpc solves over a GP per '
                             'problem')
        _require_exact_rbf([ssm], 'Cautious MPC is')
        if process_group is not None:
            raise NotImplementedError('Cautious MPC is not built for sharded particles (a process group)')
        if time_horizon < 1:
            raise ValueError(f'time_horizon={time_horizon} must be at least 1')
        check_rank_limits(num_rollouts, num_elites, num_rollouts)
        self._ssm = ssm
        self._horizon, self._num_rollouts, self._num_elites = int(time_horizon), int(num_rollouts), int(num_elites)
        self._num_iterations, self._record, self._propagate = int(num_iterations), bool(record_rollouts), bool(propagate)
        self._device = torch.device(device if device is not None else 'cuda:0')
        self._init_std = expand_init_std(init_std, self._horizon, ssm.num_actions).to(self._device)
        self._gen = torch.Generator(device=self._device)
        self._gen.manual_seed(int(seed))
        self._objective_hook = None
        self._cost = None
        self.set_env(env)
        self.last_status = 0
        self.stepwise_fallbacks = 0
        self._last_noise = self._last_actions = None
        self.last_rollouts: List[Rollouts] = []

    @property
    def num_iterations(self) -> int:
        return self._num_iterations

    def set_env(self, env: _lib.SxEnv, objective_hook=None) -> None:
        """New problem constants.  `objective_hook`, if given, is an ``Environment.objective_cost_function`` without a
        kernel form: it is evaluated with torch on the recorded means mu_1 .. mu_T, T small launches per iteration."""
        self._env = env
        self._objective_hook = objective_hook

    def set_cost(self, cost) -> None:
        """The saturating cost (`costs.SaturatingCost`) as the objective, priced in the kernel on (mu_{t+1}, Sigma_{t+1}) of
        every step (sx_cem_cautious_rollout_sat): env's objective is then not read and no objective hook is evaluated.
        None takes it off again."""
        self._cost = _checked_cost(cost, self._ssm.num_states, 'taylor')

    def sample_noise(self, episodes: int = 1) -> Tensor:
        """[iters x E x P x T x n_u] standard normals of one solve, from this solver's generator."""
        return torch.randn((self._num_iterations, episodes, self._num_rollouts, self._horizon, self._ssm.num_actions),
                           dtype=torch.float64, device=self._device, generator=self._gen)

    def solve(self, x0: Tensor, noise: Optional[Tensor] = None, init_mean: Optional[Tensor] = None,
              init_std: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, List[Rollouts], Tensor]:
        """E independent solves from x0 [E x n_s].  Nothing here synchronises with the host.

        noise: optional [iters x E x P x T x n_u] pre-drawn standard normals (parity tests inject them); init_mean /
        init_std [E x T x n_u]: the first iteration's distribution (default: zero mean, the constructor's init_std).
        Returns (best [E x T x n_u], best_ok int32 [E], rollouts per iteration (if recorded), status int32 [1])."""
        T, n_u, E, dev = self._horizon, self._ssm.num_actions, x0.size(0), x0.device
        if noise is None:
            noise = self.sample_noise(E)
        if tuple(noise.shape) != (self._num_iterations, E, self._num_rollouts, T, n_u):
            raise ValueError(f'noise must be [{self._num_iterations} x {E} x {self._num_rollouts} x {T} x {n_u}], got '
                             f'{tuple(noise.shape)}')
        self._last_noise, self._last_actions = noise, None
        mean = (init_mean.to(dev, torch.float64).reshape(E, T, n_u).contiguous() if init_mean is not None
                else torch.zeros((E, T, n_u), dtype=torch.float64, device=dev))
        std = (init_std.to(dev, torch.float64).reshape(E, T, n_u).contiguous() if init_std is not None
               else self._init_std.to(dev).expand(E, T, n_u).contiguous())
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        history: List[Rollouts] = []
        hook, n_s = (self._objective_hook if self._cost is None else None), self._ssm.num_states

        def rollout(it, mean, std, rows):
            r = cem_cautious_rollout(self._ssm, self._env, x0, T, mean=mean.contiguous(), std=std.contiguous(),
                                     noise=noise[it].contiguous(), propagate=self._propagate,
                                     want_traj=self._record or hook is not None, want_sigma=self._record,
                                     want_cov=self._record, status=status,
                                     **({} if self._cost is None else dict(cost=self._cost)))
            if hook is not None:
                r['obj_cost'] = hook_objective(hook, r['traj'], T, n_s, r['obj_cost'])
            self._last_actions = r['rows']
            if self._record:
                for e in range(E):
                    history.append(Rollouts(None, r['rows'][e], r['obj_cost'][e], r['con_cost'][e],
                                            perf_trajectories=r['traj'][e], perf_sigma=r['sigma'][e], perf_cov=r['cov'][e]))
            return r

        def rank(it, r):
            return cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['rows'], self._num_elites, want_refit=True)

        out = _cem_iterations(self._num_iterations, rollout, rank, mean, std)
        return out['best'].view(E, T, n_u), out['best_ok'], history, status

    def _solve_checked(self, x0: Tensor, where: str, q_block: Optional[Tensor] = None, init_mean: Optional[Tensor] = None):
        """`solve` and the ONE device -> host hand-off (`_check_solve`).  Returns (best [E x T x n_u] on the host, found
        bool [E] on the host, rollouts)."""
        if q_block is not None and not q_block.is_contiguous():
            q_block = q_block.contiguous()
        best, best_ok, history, status = self.solve(x0, init_mean=init_mean)
        best_host, found, _ = _check_solve(self, x0, q_block, best, best_ok, status, where, [(self, slice(None))])
        self.last_rollouts = history
        return best_host, found, history

    def get_actions_batch(self, states: Tensor, init_mean: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, List[Rollouts]]:
        """E independent problems at once: flat start states [E x (n_s + n_s^2)], all points (as
        ``FusedCemMpc.get_actions_batch``).  `init_mean` [E x T x n_u]: the warm start.  Returns (rows [E x T x n_u] on the
        host, found bool [E] on the host, rollouts)."""
        x0, q_block = split_flat_states(states, self._ssm.num_states, self._device)
        return self._solve_checked(x0, 'get_actions_batch', q_block=q_block, init_mean=init_mean)

    def get_actions(self, state: Tensor, init_mean: Optional[Tensor] = None) -> Tuple[Optional[Tensor], List[Rollouts]]:
        """state: the flat start state [1 x (n_s + n_s^2)] with an all-zero Q block.  Returns (row [T x n_u] on the host
        | None where no feasible row was found, rollouts)."""
        best, found, history = self.get_actions_batch(state.reshape(1, -1), init_mean=init_mean)
        if not bool(found[0]):
            return None, history
        return best[0], history

    def evaluate(self, x0: Tensor, rows: Tensor):
        """The rollout of given rows [E x P x T x n_u] from x0 [E x n_s] with every output: what a verbose caller reads."""
        return cem_cautious_rollout(self._ssm, self._env, x0.to(self._device, torch.float64), self._horizon,
                                    rows=rows.to(self._device, torch.float64).contiguous(), propagate=self._propagate,
                                    want_traj=True, want_sigma=True, want_cov=True, want_margins=True,
                                    **({} if self._cost is None else dict(cost=self._cost)))


class MultiModelCautiousCemMpc(MultiModelCem):
    """E independent Cautious MPC problems with an exact GP each -- the cautious arm of the reference's experiments, one
    scenario per model (episode_runner.py:40-123) -- solved together: one ``sx_cem_cautious_rollout_multi`` launch
    (``sx_cem_cautious_rollout_sat_multi`` where the solvers carry a ``SaturatingCost``) and one ranking launch per CEM
    iteration for all of them, where ``CautiousCemMpc`` needs one solve per model.

    Problem e keeps a ``CautiousCemMpc`` of its own (``solvers[e]``, built here from the same settings with seed
    ``seed + e`` unless given): it supplies the problem's noise draws (``sample_noise(1)`` of solver e), so a multi-model
    solve samples exactly what E sequential ``get_actions`` calls would, and it takes over where the single launch does not
    apply: a model without a form (``FusedMultiUnsupported``; one solve per solver then, ``per_model_solves``) or a solver
    with an objective hook and no kernel cost.  The solvers share T, particles, elites, iterations, ``propagate``, the
    initial spread, the environment constants (there is ONE sx_env: k_fb, the box, the polytope, beta) and the cost.
    """

    _SHARED = (('time_horizon', '_horizon'), ('num_rollouts', '_num_rollouts'), ('num_elites', '_num_elites'),
               ('num_iterations', '_num_iterations'), ('propagate', '_propagate'), ('device', '_device'),
               ('init_std', '_init_std'),
               ('the environment constants (env: one sx_env with k_fb, the box, the polytope and beta)', '_env'),
               ('the cost (equal SaturatingCosts on all of them, or none on any)', '_cost'))
    _POLICY = SharedPolicy('a multi-model cautious solve')

    def __init__(self, ssms: Sequence[GpCemSSM], env: _lib.SxEnv, time_horizon: int, num_rollouts: int, num_elites: int,
                 num_iterations: int, *, propagate: bool = True, device=None, seed: int = 0, init_std=1.0,
                 process_group=None, solvers: Optional[Sequence[CautiousCemMpc]] = None):
        if process_group is not None:
            raise NotImplementedError('Cautious MPC is not built for sharded particles (a process group)')
        self._ssms = list(ssms)
        if not self._ssms:
            raise ValueError('MultiModelCautiousCemMpc needs at least one model')
        if len({(s.num_states, s.num_actions) for s in self._ssms}) != 1:
            raise ValueError('the models of a multi-model solve must share (n_s, n_u)')
        if solvers is None:
            solvers = [CautiousCemMpc(ssm, env, time_horizon, num_rollouts, num_elites, num_iterations, propagate=propagate,
                                      device=device, seed=seed + e, init_std=init_std) for e, ssm in enumerate(self._ssms)]
        solvers = list(solvers)
        if len(solvers) != len(self._ssms) or any(s._ssm is not m for s, m in zip(solvers, self._ssms)):
            raise ValueError(f'{len(solvers)} solvers for {len(self._ssms)} models: solvers[e] solves over ssms[e]')
        super().__init__(solvers)

    @classmethod
    def from_solvers(cls, solvers: Sequence[CautiousCemMpc]) -> 'MultiModelCautiousCemMpc':
        """The multi-model solve over existing single-model solvers, solvers[e] for problem e, with their settings (which
        `check_solvers` compares)."""
        first = solvers[0]
        return cls([s._ssm for s in solvers], first._env, first._horizon, first._num_rollouts, first._num_elites,
                   first._num_iterations, propagate=first._propagate, device=first._device, solvers=solvers)

    def set_env(self, env: _lib.SxEnv, objective_hook=None) -> None:
        """`CautiousCemMpc.set_env` on every solver."""
        for s in self._solvers:
            s.set_env(env, objective_hook=objective_hook)

    def form(self) -> int:
        """sx_cem_cautious_rollout_multi_form of the models: < 0 where they have no single launch.  Host only."""
        first = self._solvers[0]
        return int(_lib.lib().sx_cem_cautious_rollout_multi_form(model_array(self._ssms, 'rbf'), len(self._ssms),
                                                                 first._horizon))

    def fused_applies(self) -> bool:
        """Does one launch serve the solve?  Every model has a form (`form`), and no solver evaluates an objective hook
        (a hook without a kernel cost: torch on the recorded means, one solver at a time).  Host only."""
        if any(s._objective_hook is not None and s._cost is None for s in self._solvers):
            return False
        return self.form() >= 0

    def solve(self, x0: Tensor, noise: Optional[Tensor] = None, init_mean: Optional[Tensor] = None
              ) -> Tuple[Tensor, Tensor, Tensor]:
        """E = len(models) solves from x0 [E x n_s] in one rollout and one ranking launch per iteration.  Nothing
        synchronises.  noise: optional [iters x E x P x T x n_u] standard normals; by default problem e draws
        ``solvers[e].sample_noise(1)``.  init_mean [E x T x n_u]: the warm start (default zero).
        Returns (best [E x T x n_u], best_ok int32 [E], status int32 [E]: one word per problem).
        Raises FusedMultiUnsupported (before any draw or launch) where the single launch does not apply."""
        self.check_solvers(self._solvers)
        first = self._solvers[0]
        E, T, n_s, n_u = len(self._ssms), first._horizon, self._ssms[0].num_states, self._ssms[0].num_actions
        if x0.shape != (E, n_s):
            raise ValueError(f'x0 must be [{E} x {n_s}], got {tuple(x0.shape)}')
        if not self.fused_applies():
            raise FusedMultiUnsupported(f'no single launch of the cautious solve for these solvers (N = '
                                        f'{[ssm.device_model.n_train for ssm in self._ssms]}, T = {T}, or an objective '
                                        f'hook without a kernel cost): the solvers act one at a time')
        dev = x0.device
        if noise is None:
            noise = torch.stack([s.sample_noise(1)[:, 0] for s in self._solvers], dim=1)
        if tuple(noise.shape) != (first._num_iterations, E, first._num_rollouts, T, n_u):
            raise ValueError(f'noise must be [{first._num_iterations} x {E} x {first._num_rollouts} x {T} x {n_u}], got '
                             f'{tuple(noise.shape)}')
        self._last_noise, self._last_actions = noise, None
        mean = (init_mean.to(dev, torch.float64).reshape(E, T, n_u).contiguous() if init_mean is not None
                else torch.zeros((E, T, n_u), dtype=torch.float64, device=dev))
        std = first._init_std.to(dev).expand(E, T, n_u).contiguous()
        status = torch.zeros(E, dtype=torch.int32, device=dev)
        env, cost, propagate, k = first._env, first._cost, first._propagate, first._num_elites

        def rollout(it, mean, std, rows):
            r = cem_cautious_rollout_multi(self._ssms, env, x0, T, mean=mean.contiguous(), std=std.contiguous(),
                                           noise=noise[it].contiguous(), propagate=propagate, status=status,
                                           table=self._table, **({} if cost is None else dict(cost=cost)))
            self._last_actions = r['rows']
            return r

        def rank(it, r):
            return cem_rank_refit_any(r['con_cost'], r['obj_cost'], r['rows'], k, want_refit=True)

        out = _cem_iterations(first._num_iterations, rollout, rank, mean, std)
        return out['best'].view(E, T, n_u), out['best_ok'], status

    def get_actions_multi(self, flat_states: Tensor, init_mean: Optional[Tensor] = None,
                          where: str = 'get_actions_multi') -> Tuple[Tensor, Tensor]:
        """Flat start states [E x (n_s + n_s^2)], all points, problem e for model e; `init_mean` [E x T x n_u]: every
        problem's warm start.  Returns (rows [E x T x n_u] on the host, found bool [E] on the host); ``found[e] == False``
        is the ``get_actions`` ``None`` of problem e.  Raises like ``CautiousCemMpc.get_actions`` where a problem hit a
        numerical failure, for that problem only (one status word per problem)."""
        self.check_solvers(self._solvers)
        init = {} if init_mean is None else dict(init_mean=init_mean.to(self._device, torch.float64).reshape(
            len(self._ssms), self._solvers[0]._horizon, -1))
        best_host, found = self._get_actions_multi(flat_states, where, **init)
        for s in self._solvers:
            s.last_rollouts = []
        return best_host, found
