"""CPU: the variance form of the CEM solver's performance trajectory, host side -- sx_cem_perf_rollout_var is declared and
exported and checks its arguments before any device access; FusedCemMpc(perf_variance=True) and conf.cem_perf_variance admit
the variance objective and keep every other refusal; with fakes in place of the launches a solve with the setting calls the
new entry once per iteration and sx_cem_perf_rollout never, and a solve without it calls what it called before; and the numpy
oracle (tests/perf_var_oracle.py) against perf_traj_oracle.perf_rollout and a hand-rolled loop."""
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
from perf_var_oracle import perf_var_rollout
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc
from safe_exploration_amd.safempc_cem import CemSafeMPC, get_actions_multi
from safe_exploration_amd.safempc_exploration import DynamicSafeMPCExploration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'sx_cem_perf_rollout_var'
VAR, ABS = _lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS


def test_entry_is_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    assert re.search(r'\bint ' + NAME + r'\(', header)
    assert NAME in _lib.SIGNATURES
    assert hasattr(_lib.lib(), NAME)
    assert callable(cem_mpc.cem_perf_rollout_var)


def _model(n_s=2, n_u=1, n_train=20):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.n_pad = (n_train + 1 + n_s + n_u + 15) // 16 * 16
    m.x_train = m.a_pack = m.stage_tab = 16      # never dereferenced: every call below is answered before any device access
    for i in range(n_s * (n_s + n_u)):
        m.inv_ls2[i] = 1.0
    for i in range(n_s):
        m.outputscale[i] = 1.0
    return m


def _env(n_s=2, n_u=1, obj_mode=VAR):
    env = _lib.SxEnv()
    env.n_s, env.n_u, env.m, env.obj_mode = n_s, n_u, 4, obj_mode
    return env


def _call(model, env, *, E=1, P=4, H=5, n_perf=8, r=1, x0=16, safe=16, mean=16, std=16, noise=16, rows=16, obj=16, con=16,
          status=16):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return _lib.lib().sx_cem_perf_rollout_var(None if model is None else ctypes.byref(model),
                                              None if env is None else ctypes.byref(env), E, P, H, n_perf, r, p(x0), p(safe),
                                              p(mean), p(std), p(noise), p(rows), p(obj), p(con), None, None, p(status), None)


@pytest.mark.parametrize('obj_mode', [VAR, ABS])
def test_argument_errors_without_a_gpu(obj_mode):
    m, env = _model(), _env(obj_mode=obj_mode)
    for kw in (dict(x0=None), dict(safe=None), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None),
               dict(mean=None), dict(std=None), dict(E=0), dict(P=0), dict(H=0), dict(r=0), dict(r=6), dict(n_perf=1),
               dict(n_perf=3, r=3)):
        assert _call(m, env, **kw) == _lib.SX_ERR_ARG, kw
    assert _call(None, env) == _lib.SX_ERR_ARG and _call(m, None) == _lib.SX_ERR_ARG
    assert _call(_model(n_train=0), env) == _lib.SX_ERR_ARG
    assert _call(_model(2, 2), env) == _lib.SX_ERR_ARG                  # model and env disagree on the shape
    for field in ('x_train', 'a_pack', 'stage_tab'):                    # the packed model, not alpha
        bad = _model()
        setattr(bad, field, None)
        assert _call(bad, env) == _lib.SX_ERR_ARG, field
    bad = _model()
    bad.n_pad = 16                                                      # no room for the training rows and the mean row
    assert _call(bad, env) == _lib.SX_ERR_ARG
    assert _call(m, _env(obj_mode=7)) == _lib.SX_ERR_ARG
    # a shape without a rollout kernel; training sets beyond the output-by-output form; one output has no such form:
    assert _call(_model(3, 2), _env(3, 2, obj_mode)) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(n_train=4096), env) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(n_train=1100), env) == _lib.SX_ERR_UNSUPPORTED
    # (1, 1) keeps its one output in LDS up to N = 1021 (n_pad = 1024); N = 1000 has a form, and was refused here only for
    # want of a device to launch on -- on a GPU host that call launched over these pointers
    assert _call(_model(1, 1, n_train=1022), _env(1, 1, obj_mode)) == _lib.SX_ERR_UNSUPPORTED


# ---- FusedCemMpc: the setting and the refusals that stay -------------------------------------------------------------------
class _Ssm:
    """An exact GP as far as the host-side plan reads it (never launched: the wrappers are fakes)."""
    num_states, num_actions, kernel_family = 2, 1, 'rbf'

    def __init__(self, family='rbf', n_train=60):
        m = _lib.SxGpModel()
        m.n_s, m.n_u, m.n_train = 2, 1, n_train
        m.n_pad = (n_train + 1 + 2 + 1 + 15) // 16 * 16
        self.device_model = m
        self.kernel_family = family


def test_the_setting_admits_the_variance_objective():
    mpc = FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_variance=True)
    mpc.set_env(_env(obj_mode=ABS))
    mpc.set_env(_env(obj_mode=VAR))
    # without it the refusals are the parent's, with the parent's words
    with pytest.raises(ValueError, match='variance objective'):
        FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', n_perf=6)
    with pytest.raises(ValueError, match='variance objective'):
        FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_variance=False)
    plain = FusedCemMpc(_Ssm(), _env(obj_mode=ABS), 5, 64, 8, 3, device='cpu', n_perf=6)
    with pytest.raises(ValueError, match='variance objective'):
        plain.set_env(_env(obj_mode=VAR))


@pytest.mark.parametrize('kw', [dict(), dict(n_perf=0)])
def test_the_setting_needs_a_performance_trajectory(kw):
    with pytest.raises(ValueError, match='perf_variance'):
        FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', perf_variance=True, **kw)


@pytest.mark.parametrize('family', ['feature', 'mlp', 'rbf_junk', 'feature_junk', 'mlp_junk', 'stepwise'])
def test_other_model_families_are_still_refused(family):
    with pytest.raises(NotImplementedError, match='exact RBF'):
        FusedCemMpc(_Ssm(family), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_variance=True)
    with pytest.raises(NotImplementedError, match='exact RBF'):
        FusedCemMpc(_Ssm(family), _env(obj_mode=ABS), 5, 64, 8, 3, device='cpu', n_perf=6, perf_variance=True)
    with mock.patch.object(_lib, 'require_gpu', lambda *a: None), pytest.raises(NotImplementedError, match='exact RBF'):
        cem_mpc.cem_perf_rollout_var(_Ssm(family), _env(), torch.zeros((1, 2), dtype=torch.float64), 5, 6, 1,
                                     safe_actions=None, obj_cost=None, con_cost=None, status=None)


def test_a_process_group_and_multi_solver_calls_are_still_refused():
    with pytest.raises(NotImplementedError, match='process group'):
        FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_variance=True, process_group=object())
    mpcs = [FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_variance=True) for _ in range(2)]
    with pytest.raises(NotImplementedError, match='performance trajectory'):
        MultiModelCemMpc.from_solvers(mpcs)
    solvers = [_safempc(conf(cem_n_perf=6, cem_perf_variance=True), objective_target=None), _safempc(conf())]
    with pytest.raises(NotImplementedError, match='cem_n_perf'):
        get_actions_multi(solvers, np.zeros((2, 2)))


# ---- the iteration loop with fakes in place of the launches ----------------------------------------------------------------
def _fakes(monkeypatch, k, seen):
    def rollout(ssm, env, x0, horizon, *, noise, mean=None, std=None, elite_rows=None, status=None, **kw):
        E, P = x0.size(0), noise.size(1)
        seen.append(('rollout', tuple(noise.shape), tuple(mean.shape), 'rows' if elite_rows is not None else 'dist'))
        return dict(actions=torch.zeros((E, P, horizon, 1), dtype=torch.float64), obj_cost=torch.zeros((E, P)),
                    con_cost=torch.zeros((E, P)), traj=torch.zeros((E, P, horizon, 6)) if kw.get('want_traj') else None,
                    sigma=None, status=status)

    def rank(con, obj, actions, kk, want_rows=False, want_refit=True):
        E, L = con.size(0), actions[0, 0].numel()
        seen.append(('rank', tuple(actions.shape), want_rows, want_refit))
        full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64)
        return dict(elite_rows=full(0, E, k, 2 + L) if want_rows else None, mean=full(1, E, L) if want_refit else None,
                    std=full(2, E, L) if want_refit else None, best=torch.arange(E * L, dtype=torch.float64).view(E, L),
                    best_ok=torch.ones(E, dtype=torch.int32))

    monkeypatch.setattr(cem_mpc, 'cem_rollout', rollout)
    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)


E_, P_, H_, ITERS, N_PERF, R_ = 2, 64, 5, 3, 9, 2
T_ = N_PERF - R_


def _perf_fake(seen, name):
    def perf(ssm, env, x0, horizon, n_perf_, r_, *, safe_actions, obj_cost, con_cost, status, tail_mean, tail_std, tail_noise,
             want_traj=False, **kw):
        seen.append((name, horizon, n_perf_, r_, tuple(safe_actions.shape), tuple(tail_mean.shape), tuple(tail_std.shape),
                     tuple(tail_noise.shape), want_traj, dict(kw)))
        z = torch.zeros((E_, P_, n_perf_, 2), dtype=torch.float64)
        return dict(rows=torch.zeros((E_, P_, H_ + T_, 1), dtype=torch.float64), obj_cost=obj_cost, con_cost=con_cost,
                    perf_traj=z if want_traj else None, perf_sigma=z + 1 if kw.get('want_sigma') else None, status=status)
    return perf


@pytest.mark.parametrize('record', [False, True])
def test_with_the_setting_every_iteration_calls_the_variance_rollout(monkeypatch, record):
    seen = []
    _fakes(monkeypatch, 8, seen)
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout', _perf_fake(seen, 'perf'))
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout_var', _perf_fake(seen, 'perf_var'))
    mpc = FusedCemMpc(_Ssm(), _env(), H_, P_, 8, ITERS, device='cpu', init_std=0.2, n_perf=N_PERF, perf_r=R_,
                      perf_variance=True, record_rollouts=record)
    noise = torch.randn((ITERS, E_, P_, H_ + T_, 1), dtype=torch.float64)
    best, ok, history, _ = mpc.solve(torch.zeros((E_, 2), dtype=torch.float64), noise=noise)
    assert tuple(best.shape) == (E_, H_ + T_, 1)
    assert [s[0] for s in seen] == ['rollout', 'perf_var', 'rank'] * ITERS
    for s in seen:
        if s[0] == 'rollout':
            assert s[1:] == ((E_, P_, H_, 1), (E_, H_, 1), 'dist')
        elif s[0] == 'perf_var':
            assert s[1:] == (H_, N_PERF, R_, (E_, P_, H_, 1), (E_, T_, 1), (E_, T_, 1), (E_, P_, T_, 1), record,
                             dict(want_sigma=record))
        else:
            assert s[1:] == ((E_, P_, H_ + T_, 1), False, True)
    # recorded rollouts keep the variances beside the means
    assert len(history) == (ITERS * E_ if record else 0)
    for h in history:
        assert tuple(h.perf_trajectories.shape) == tuple(h.perf_sigma.shape) == (P_, N_PERF, 2)
        assert bool((h.perf_sigma == 1).all())


def test_the_library_entries_a_solve_reaches(monkeypatch):
    """Through the real wrappers with a mocked library: the setting calls sx_cem_perf_rollout_var once per iteration and
    sx_cem_perf_rollout never; without it the other way round."""
    for variance in (True, False):
        seen = []
        _fakes(monkeypatch, 8, seen)
        fake = mock.Mock()
        fake.sx_cem_perf_rollout.return_value = fake.sx_cem_perf_rollout_var.return_value = _lib.SX_OK
        ssm = _Ssm()
        ssm._alpha = None
        with mock.patch.object(_lib, 'lib', lambda: fake), mock.patch.object(_lib, 'require_gpu', lambda *a: None), \
                mock.patch.object(_lib, 'stream_ptr', lambda dev: None):
            mpc = FusedCemMpc(ssm, _env(obj_mode=ABS), H_, P_, 8, ITERS, device='cpu', init_std=0.2, n_perf=N_PERF, perf_r=R_,
                              **({'perf_variance': True} if variance else {}))
            mpc.solve(torch.zeros((E_, 2), dtype=torch.float64))
        calls = (fake.sx_cem_perf_rollout_var.call_count, fake.sx_cem_perf_rollout.call_count)
        assert calls == ((ITERS, 0) if variance else (0, ITERS))
        entry = fake.sx_cem_perf_rollout_var if variance else fake.sx_cem_perf_rollout
        assert len(entry.call_args[0]) == 19
        assert entry.call_args[0][2 + (0 if variance else 1):7 + (0 if variance else 1)] == (E_, P_, H_, N_PERF, R_)


@pytest.mark.parametrize('kw', [dict(), dict(n_perf=0), dict(n_perf=N_PERF, perf_r=R_), dict(n_perf=N_PERF, perf_r=R_,
                                                                                              perf_variance=False)])
def test_without_the_setting_a_solve_calls_what_it_called(monkeypatch, kw):
    seen = []
    _fakes(monkeypatch, 8, seen)
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout', _perf_fake(seen, 'perf'))
    var = mock.Mock()
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout_var', var)
    mpc = FusedCemMpc(_Ssm(), _env(obj_mode=ABS), H_, P_, 8, ITERS, device='cpu', init_std=0.2, **kw)
    mpc.solve(torch.zeros((E_, 2), dtype=torch.float64))
    assert var.call_count == 0
    perf = kw.get('n_perf', 0) > 0
    assert [s[0] for s in seen] == (['rollout', 'perf', 'rank'] if perf else ['rollout', 'rank']) * ITERS
    for s in seen:
        if s[0] == 'perf':       # the keyword arguments of the parent's call, no more
            assert s[1:] == (H_, N_PERF, R_, (E_, P_, H_, 1), (E_, T_, 1), (E_, T_, 1), (E_, P_, T_, 1), False, {})


# ---- CemSafeMPC ------------------------------------------------------------------------------------------------------------
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


def test_cem_safempc_reads_the_setting():
    solver = _safempc(conf(cem_n_perf=6, cem_perf_variance=True), objective_target=None)    # exploration: no objective
    assert solver.performance_trajectory_length == 6
    assert _safempc(conf(cem_n_perf=6, cem_perf_variance=True)).performance_trajectory_length == 6
    with pytest.raises(ValueError, match='variance objective'):
        _safempc(conf(cem_n_perf=6), objective_target=None)
    with pytest.raises(ValueError, match='variance objective'):
        _safempc(conf(cem_n_perf=6, cem_perf_variance=False), objective_target=None)
    with pytest.raises(ValueError, match='cem_n_perf'):
        _safempc(conf(cem_perf_variance=True), objective_target=None)
    ssm = mock.Mock()
    ssm.kernel_family = 'feature'
    with pytest.raises(NotImplementedError, match='exact RBF'):
        _safempc(conf(cem_n_perf=6, cem_perf_variance=True), objective_target=None, ssm=ssm)


def test_cem_safempc_builds_the_solver_with_the_setting():
    """_solver() hands perf_variance on, and the sx_env of an objective-less environment carries the variance objective."""
    from safe_exploration_amd import safempc_cem
    from safe_exploration_amd.safempc_cem import construct_constraints
    spec = problems.pendulum(n_train=8)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=None)
    c = conf(cem_n_perf=6, cem_perf_variance=True)
    ssm = mock.Mock()
    ssm.kernel_family, ssm.num_states, ssm.num_actions = 'rbf', 2, 1
    lqr = mock.Mock()
    lqr.get_control_matrix.return_value = spec.k_fb
    solver = CemSafeMPC(ssm, construct_constraints(c, env), env, c, {'lin_model': (spec.a, spec.b)}, wx_feedback_cost=None,
                        wu_feedback_cost=None, lqr=lqr, beta_safety=2.0, safe_policy=lambda x: spec.k_fb @ x)
    with mock.patch.object(safempc_cem, 'FusedCemMpc') as fused:
        solver._solver()
    assert fused.call_args[1]['n_perf'] == 6 and fused.call_args[1]['perf_variance'] is True
    sx_env, hook = fused.return_value.set_env.call_args[0][0], fused.return_value.set_env.call_args[1]['objective_hook']
    assert sx_env.obj_mode == VAR and hook is None
    explorer = DynamicSafeMPCExploration(solver, env)
    assert (explorer.n_safe, explorer.n_perf) == (5, 6)


# ---- the numpy oracle ------------------------------------------------------------------------------------------------------
def _oracle_case(obj_mode):
    spec = problems.pendulum(n_train=30, obj_mode=obj_mode)
    gp = ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)
    rng = np.random.default_rng(3)
    P, H, T = 11, 4, 6
    safe, tail = rng.normal(0, 0.5, size=(P, H, 1)), rng.normal(0, 0.8, size=(P, T, 1))
    return spec, gp, problems.oracle_problem(spec, ocem), np.array([0.03, -0.02]), safe, tail


@pytest.mark.parametrize('r', [1, 2])
def test_oracle_means_are_the_mean_only_oracles(r):
    spec, gp, prob, x0, safe, tail = _oracle_case(ABS)
    got, ref = perf_var_rollout(prob, gp, x0, safe, tail[:, r - 1:], r), perf_rollout(prob, gp, x0, safe, tail[:, r - 1:], r)
    for name in ('rows', 'traj', 'obj_cost', 'con_cost', 'violations'):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert got.violations.sum() > 0


def test_oracle_variance_objective_is_a_hand_rolled_loop():
    spec, gp, prob, x0, safe, tail = _oracle_case(VAR)
    got = perf_var_rollout(prob, gp, x0, safe, tail, 1)
    P, n_perf = safe.shape[0], 1 + tail.shape[1]
    assert tuple(got.sigma.shape) == (P, n_perf, 2) and tuple(got.queries.shape) == (P, n_perf, 3)
    for c in range(P):
        mu, total = x0.copy(), 0.0
        for t in range(n_perf):
            v = safe[c, 0] if t == 0 else tail[c, t - 1]
            z = np.concatenate((mu, v))
            # one particle at a time against the batch: the same operations in another BLAS summation order, a few ulp per
            # step, carried along the chain; the variance s + noise - |L^-1 k*|^2 loses up to s / var ~ 1e4 of them
            # (states of order 1: an absolute 1e-13 is a few hundred ulp)
            np.testing.assert_allclose(got.queries[c, t], z, rtol=1e-12, atol=1e-13)
            mean, var, _ = gp.predict(z[None], jacobians=False)
            np.testing.assert_allclose(got.sigma[c, t], var[0], rtol=1e-9, atol=0)
            total -= var[0].sum()
            mu = spec.a @ mu + spec.b @ v + mean[0]
            np.testing.assert_allclose(got.traj[c, t], mu, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(got.obj_cost[c], total, rtol=1e-9)
        np.testing.assert_allclose(got.obj_cost[c], -got.sigma[c].sum(), rtol=1e-14)
    assert (got.sigma > 0).all()
