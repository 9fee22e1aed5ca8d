"""CPU: the performance trajectory of the CEM solver, host side -- sx_cem_perf_rollout is declared and exported and checks
its arguments before any device access; CemSafeMPC reads conf.cem_n_perf / conf.cem_perf_r; a solver without the setting
launches no performance rollout; the refusals; the iteration loop's plumbing of the long rows (fakes in place of the
launches); and the numpy oracle of the performance rollout against oracle.cem.rollout's first centre."""
import collections
import ctypes
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.gp import ExactGP
from perf_traj_oracle import perf_rollout
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc
from safe_exploration_amd.safempc_cem import CemSafeMPC, get_actions_multi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'sx_cem_perf_rollout'


def test_entry_is_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    assert re.search(r'\bint ' + NAME + r'\(', header)
    assert NAME in _lib.SIGNATURES
    assert hasattr(_lib.lib(), NAME)


def _model(n_s=2, n_u=1, n_train=20):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.x_train = 16       # never dereferenced: every call below is answered before any device access
    for i in range(n_s * (n_s + n_u)):
        m.inv_ls2[i] = 1.0
    for i in range(n_s):
        m.outputscale[i] = 1.0
    return m


def _env(n_s=2, n_u=1, obj_mode=_lib.SX_OBJ_AFFINE_ABS):
    env = _lib.SxEnv()
    env.n_s, env.n_u, env.m, env.obj_mode = n_s, n_u, 4, obj_mode
    return env


def _call(model, env, *, E=1, P=4, H=5, n_perf=8, r=1, alpha=16, x0=16, safe=16, mean=16, std=16, noise=16, rows=16, obj=16,
          con=16, status=16):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return _lib.lib().sx_cem_perf_rollout(None if model is None else ctypes.byref(model), p(alpha),
                                          None if env is None else ctypes.byref(env), E, P, H, n_perf, r, p(x0), p(safe),
                                          p(mean), p(std), p(noise), p(rows), p(obj), p(con), None, p(status), None)


def test_argument_errors_without_a_gpu():
    m, env = _model(), _env()
    for kw in (dict(alpha=None), dict(x0=None), dict(safe=None), dict(rows=None), dict(obj=None), dict(con=None),
               dict(status=None), dict(mean=None), dict(std=None), dict(E=0), dict(P=0), dict(H=0), dict(r=0), dict(r=6),
               dict(n_perf=1), dict(n_perf=3, r=3)):
        assert _call(m, env, **kw) == _lib.SX_ERR_ARG, kw
    assert _call(None, env) == _lib.SX_ERR_ARG and _call(m, None) == _lib.SX_ERR_ARG
    assert _call(_model(n_train=0), env) == _lib.SX_ERR_ARG
    assert _call(_model(2, 2), env) == _lib.SX_ERR_ARG                  # model and env disagree on the shape
    no_x = _model()
    no_x.x_train = None
    assert _call(no_x, env) == _lib.SX_ERR_ARG
    # the variance objective needs the N x N product; a shape without a rollout kernel; a training set beyond the LDS
    assert _call(m, _env(obj_mode=_lib.SX_OBJ_NEG_VARIANCE)) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(3, 2), _env(3, 2)) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(n_train=4096), env) == _lib.SX_ERR_UNSUPPORTED


# ---- CemSafeMPC: the settings and the refusals ---------------------------------------------------------------------------
class Conf:
    mpc_time_horizon = 5
    cem_num_rollouts = 64
    cem_num_elites = 8
    cem_num_iterations = 3
    plot_cem_optimisation = False
    plot_cem_terminal_states = False
    device = 'cpu'
    use_state_constraint = True
    use_prior_model = True
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'


def conf(**kw):
    return type('C', (Conf,), kw)()


def _safempc(c, objective_target=-0.1, ssm=None, mpc=None):
    spec = problems.pendulum(n_train=8, obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=objective_target)
    if ssm is None:
        ssm = mock.Mock()
        ssm.kernel_family = 'rbf'
    return CemSafeMPC(ssm, [], env, c, {'lin_model': (spec.a, spec.b)}, wx_feedback_cost=None, wu_feedback_cost=None,
                      lqr=mock.Mock(), mpc=mpc, beta_safety=2.0, safe_policy=lambda x: spec.k_fb @ x)


def test_performance_trajectory_length_follows_the_setting():
    assert _safempc(conf(cem_n_perf=6)).performance_trajectory_length == 6
    assert _safempc(conf(cem_n_perf=6, cem_perf_r=3)).performance_trajectory_length == 6
    assert _safempc(conf()).performance_trajectory_length == 0
    assert _safempc(conf(cem_n_perf=0)).performance_trajectory_length == 0
    # the casadi settings the reference's CEM configs inherit do not switch it on
    assert _safempc(conf(n_perf=5, r=1, type_perf_traj='taylor')).performance_trajectory_length == 0


@pytest.mark.parametrize('kw', [dict(cem_n_perf=6, cem_perf_r=0), dict(cem_n_perf=6, cem_perf_r=6),
                                dict(cem_n_perf=1, cem_perf_r=1), dict(cem_n_perf=9, cem_perf_r=6)])
def test_settings_out_of_range_are_refused(kw):
    with pytest.raises(ValueError, match='cem_perf_r'):
        _safempc(conf(**kw))
    H = Conf.mpc_time_horizon
    with pytest.raises(ValueError, match='perf_r'):
        FusedCemMpc(_Ssm(), _fused_env(), H, 64, 8, 3, device='cpu', n_perf=kw['cem_n_perf'], perf_r=kw['cem_perf_r'])


class _Ssm:
    """An exact GP as far as the host-side plan reads it (never launched: the wrappers are fakes)."""
    num_states, num_actions, kernel_family = 2, 1, 'rbf'

    def __init__(self, family='rbf', n_train=60):
        m = _lib.SxGpModel()
        m.n_s, m.n_u, m.n_train = 2, 1, n_train
        m.n_pad = (n_train + 1 + 2 + 1 + 15) // 16 * 16
        self.device_model = m
        self.kernel_family = family


def _fused_env(obj_mode=_lib.SX_OBJ_AFFINE_ABS):
    return _env(obj_mode=obj_mode)


@pytest.mark.parametrize('family', ['feature', 'mlp', 'rbf_junk', 'feature_junk', 'mlp_junk', 'stepwise'])
def test_other_model_families_are_refused_at_construction(family):
    with pytest.raises(NotImplementedError, match='exact RBF'):
        FusedCemMpc(_Ssm(family), _fused_env(), 5, 64, 8, 3, device='cpu', n_perf=6)
    ssm = mock.Mock()
    ssm.kernel_family = family
    with pytest.raises(NotImplementedError, match='exact RBF'):
        _safempc(conf(cem_n_perf=6), ssm=ssm)
    FusedCemMpc(_Ssm(family), _fused_env(), 5, 64, 8, 3, device='cpu')      # fine without the setting


def test_a_process_group_is_refused_at_construction():
    with pytest.raises(NotImplementedError, match='process group'):
        FusedCemMpc(_Ssm(), _fused_env(), 5, 64, 8, 3, device='cpu', n_perf=6, process_group=object())


def test_the_variance_objective_is_refused():
    with pytest.raises(ValueError, match='variance objective'):
        _safempc(conf(cem_n_perf=6), objective_target=None)      # objective_cost_function returns None
    with pytest.raises(ValueError, match='variance objective'):
        FusedCemMpc(_Ssm(), _fused_env(_lib.SX_OBJ_NEG_VARIANCE), 5, 64, 8, 3, device='cpu', n_perf=6)
    mpc = FusedCemMpc(_Ssm(), _fused_env(), 5, 64, 8, 3, device='cpu', n_perf=6)
    with pytest.raises(ValueError, match='variance objective'):
        mpc.set_env(_fused_env(_lib.SX_OBJ_NEG_VARIANCE))
    mpc.set_env(_fused_env(_lib.SX_OBJ_NEG_VARIANCE), objective_hook=lambda p: p[:, 0])     # the hook carries the objective


def test_multi_solver_calls_are_refused():
    solvers = [_safempc(conf(cem_n_perf=6)), _safempc(conf())]
    with pytest.raises(NotImplementedError, match='cem_n_perf'):
        get_actions_multi(solvers, np.zeros((2, 2)))
    mpcs = [FusedCemMpc(_Ssm(), _fused_env(), 5, 64, 8, 3, device='cpu', n_perf=6) for _ in range(2)]
    with pytest.raises(NotImplementedError, match='performance trajectory'):
        MultiModelCemMpc.from_solvers(mpcs)


# ---- the iteration loop with fakes in place of the launches ----------------------------------------------------------------
class CountingLib:
    """The loaded library with every entry counted (tests/test_gpu_junk_fused.py counts the same way)."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def _fakes(monkeypatch, k, seen):
    def rollout(ssm, env, x0, horizon, *, noise, mean=None, std=None, elite_rows=None, status=None, **kw):
        E, P = x0.size(0), noise.size(1)
        seen.append(('rollout', tuple(noise.shape), tuple(mean.shape), 'rows' if elite_rows is not None else 'dist'))
        return dict(actions=torch.zeros((E, P, horizon, 1), dtype=torch.float64), obj_cost=torch.zeros((E, P)),
                    con_cost=torch.zeros((E, P)), traj=None, sigma=None, status=status)

    def rank(con, obj, actions, kk, want_rows=False, want_refit=True):
        E, L = con.size(0), actions[0, 0].numel()
        seen.append(('rank', tuple(actions.shape), want_rows, want_refit))
        full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64)
        return dict(elite_rows=full(0, E, k, 2 + L) if want_rows else None, mean=full(1, E, L) if want_refit else None,
                    std=full(2, E, L) if want_refit else None, best=torch.arange(E * L, dtype=torch.float64).view(E, L),
                    best_ok=torch.ones(E, dtype=torch.int32))

    monkeypatch.setattr(cem_mpc, 'cem_rollout', rollout)
    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)


@pytest.mark.parametrize('kw', [dict(), dict(n_perf=0)])
def test_without_the_setting_no_performance_rollout_is_launched(monkeypatch, kw):
    seen = []
    _fakes(monkeypatch, 8, seen)
    perf = mock.Mock()
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout', perf)
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: counting)
    E, P, H, iters = 2, 64, 5, 3
    mpc = FusedCemMpc(_Ssm(), _fused_env(), H, P, 8, iters, device='cpu', init_std=0.2, **kw)
    best, ok, _, _ = mpc.solve(torch.zeros((E, 2), dtype=torch.float64))
    assert counting.calls[NAME] == 0 and perf.call_count == 0
    assert tuple(best.shape) == (E, H, 1)
    assert [s[0] for s in seen] == ['rollout', 'rank'] * iters
    assert all(s[1] == (E, P, H, 1) for s in seen if s[0] == 'rollout')
    assert all(s[1] == (E, P, H, 1) for s in seen if s[0] == 'rank')


def test_with_the_setting_every_iteration_runs_safety_performance_ranking(monkeypatch):
    seen = []
    _fakes(monkeypatch, 8, seen)
    E, P, H, iters, n_perf, r = 2, 64, 5, 3, 9, 2
    T = n_perf - r

    def perf(ssm, env, x0, horizon, n_perf_, r_, *, safe_actions, obj_cost, con_cost, status, tail_mean, tail_std, tail_noise,
             want_traj=False, **kw):
        seen.append(('perf', horizon, n_perf_, r_, tuple(safe_actions.shape), tuple(tail_mean.shape), tuple(tail_std.shape),
                     tuple(tail_noise.shape), want_traj))
        return dict(rows=torch.zeros((E, P, H + T, 1), dtype=torch.float64), obj_cost=obj_cost, con_cost=con_cost,
                    perf_traj=None, status=status)

    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout', perf)
    mpc = FusedCemMpc(_Ssm(), _fused_env(), H, P, 8, iters, device='cpu', init_std=0.2, n_perf=n_perf, perf_r=r)
    noise = torch.randn((iters, E, P, H + T, 1), dtype=torch.float64)
    best, ok, _, _ = mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=noise)
    assert tuple(best.shape) == (E, H + T, 1)
    assert [s[0] for s in seen] == ['rollout', 'perf', 'rank'] * iters
    for s in seen:
        if s[0] == 'rollout':     # the safety rollout samples the first H steps from the distribution, never from elite rows
            assert s[1:] == ((E, P, H, 1), (E, H, 1), 'dist')
        elif s[0] == 'perf':
            assert s[1:] == (H, n_perf, r, (E, P, H, 1), (E, T, 1), (E, T, 1), (E, P, T, 1), False)
        else:                     # the ranking sees the long rows and refits itself
            assert s[1:] == ((E, P, H + T, 1), False, True)
    # the start distribution of the tail: zero mean, the constructor's init_std
    mean, std = mpc.start_distribution(torch.zeros((E, 2), dtype=torch.float64))
    assert tuple(mean.shape) == tuple(std.shape) == (E, H + T, 1)
    assert bool((mean == 0).all()) and bool((std == 0.2).all())


# ---- the numpy oracle ------------------------------------------------------------------------------------------------------
def test_oracle_first_centre_is_the_safety_rollouts():
    """r = 1 from a point: mu_1 is a x + b u + mean, and so is the first centre of oracle.cem.rollout -- exactly."""
    spec = problems.pendulum(n_train=30, obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    gp = ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)
    prob = problems.oracle_problem(spec, ocem)
    rng = np.random.default_rng(3)
    P, H, T = 11, 4, 6
    safe, tail = rng.normal(0, 0.5, size=(P, H, 1)), rng.normal(0, 0.8, size=(P, T, 1))
    x0 = np.array([0.03, -0.02])
    perf = perf_rollout(prob, gp, x0, safe, tail, 1)
    ref = ocem.rollout(prob, gp, x0, safe)
    assert np.array_equal(perf.traj[:, 0], ref.traj_p[:, 0])
    assert tuple(perf.rows.shape) == (P, H + T, 1) and tuple(perf.traj.shape) == (P, 1 + T, 2)
    # costs: the objective over all n_perf means, 3 per tail action outside the box (the shared action is the safety rollout's)
    want = sum(np.abs(spec.obj_target[1] - perf.traj[:, t, 1]) for t in range(1 + T))
    assert np.allclose(perf.obj_cost, want, rtol=1e-14)
    viol = (np.abs(tail[:, :, 0]) > 1.0).sum(axis=1)
    assert viol.sum() > 0 and np.array_equal(perf.violations, viol) and np.array_equal(perf.con_cost, 3.0 * viol)
    # with r = 2 the second action is shared too: the first two means are the safety centres of a deterministic model only
    # in their first step (the safety rollout adds the feedback on the ellipsoid from step 2 on), the first still agrees
    perf2 = perf_rollout(prob, gp, x0, safe, tail[:, 1:], 2)
    assert np.array_equal(perf2.traj[:, 0], ref.traj_p[:, 0])
