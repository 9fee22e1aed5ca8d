"""CPU: the Taylor form of the CEM solver's performance trajectory, host side -- the numpy oracle
(tests/perf_taylor_oracle.py) against itself and against perf_var_oracle; sx_cem_perf_rollout_taylor and its form query are
declared, exported and check their arguments before any device access; FusedCemMpc(perf_type=...) and conf.cem_perf_type /
conf.cem_perf_terminal_safety raise what they must; get_actions_multi routes solvers with the Taylor form one model at a
time; and a solver without the settings calls what it called before."""
import ctypes
import dataclasses
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.gp import ExactGP
from perf_taylor_oracle import block_step, perf_taylor_rollout
from perf_var_oracle import perf_var_rollout
from safe_exploration_amd import _lib, cem_mpc, problems, safempc_cem
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelPerfCemMpc
from safe_exploration_amd.safempc_cem import get_actions_multi
from test_perf_var_host import (E_, H_, ITERS, N_PERF, P_, R_, T_, _env, _fakes, _model, _perf_fake, _safempc, _Ssm, conf)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, FORM = 'sx_cem_perf_rollout_taylor', 'sx_cem_perf_rollout_taylor_form'
VAR, ABS = _lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS


# ---- the numpy oracle ------------------------------------------------------------------------------------------------------
def _oracle_case(obj_mode=VAR):
    spec = problems.pendulum(n_train=30, obj_mode=obj_mode)
    gp = ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)
    rng = np.random.default_rng(3)
    P, H, T = 11, 4, 6
    safe, tail = rng.normal(0, 0.5, size=(P, H, 1)), rng.normal(0, 0.8, size=(P, T, 1))
    return spec, gp, problems.oracle_problem(spec, ocem), np.array([0.03, -0.02]), safe, tail


def test_oracle_first_step_and_positive_semi_definite_covariances():
    spec, gp, prob, x0, safe, tail = _oracle_case()
    got = perf_taylor_rollout(prob, gp, x0, safe, tail, 1)
    P, n_perf = safe.shape[0], 1 + tail.shape[1]
    assert tuple(got.cov.shape) == (P, n_perf, 2, 2) and tuple(got.sigma.shape) == (P, n_perf, 2)
    _, var0, _ = gp.predict(got.queries[:, 0], jacobians=True)
    # Sigma_0 = 0: every block of sigma_z is an exact zero
    assert np.array_equal(got.cov[:, 0], var0[:, :, None] * np.eye(2)[None])
    assert np.array_equal(got.sigma[:, 0], var0) and np.array_equal(got.var[:, 0], var0)
    # (the block products are symmetric up to the order of their sums)
    scale = np.abs(got.cov).max(axis=(2, 3), keepdims=True)
    assert (np.abs(got.cov - np.swapaxes(got.cov, 2, 3)) <= 1e-14 * scale).all()
    sym = 0.5 * (got.cov + np.swapaxes(got.cov, 2, 3))
    assert (np.linalg.eigvalsh(sym) >= -1e-14 * scale[..., 0]).all()
    assert (got.sigma >= got.var).all() and (got.sigma[:, 1:] > got.var[:, 1:]).any()
    assert np.array_equal(got.obj_cost, -got.sigma.sum(axis=(1, 2))) or np.allclose(got.obj_cost, -got.sigma.sum(axis=(1, 2)),
                                                                                     rtol=1e-14, atol=0)


@pytest.mark.parametrize('r', [1, 2])
@pytest.mark.parametrize('obj_mode', [VAR, ABS])
def test_oracle_without_feedback_and_jacobian_is_the_variance_oracle(obj_mode, r):
    """K = 0 and J = 0: sigma_g = diag(var), the means and every cost are perf_var_oracle's, bit for bit."""
    spec, gp, prob, x0, safe, tail = _oracle_case(obj_mode)
    prob0 = dataclasses.replace(prob, k_fb=np.zeros_like(prob.k_fb))

    class NoJacobian:
        def predict(self, z, jacobians=True):
            mean, var, jac = gp.predict(z, jacobians=jacobians)
            return mean, var, None if jac is None else np.zeros_like(jac)

    got = perf_taylor_rollout(prob0, NoJacobian(), x0, safe, tail[:, r - 1:], r)
    ref = perf_var_rollout(prob, gp, x0, safe, tail[:, r - 1:], r)
    for mine, theirs in (('rows', 'rows'), ('traj', 'traj'), ('sigma', 'sigma'), ('var', 'sigma'), ('queries', 'queries'),
                         ('obj_cost', 'obj_cost'), ('con_cost', 'con_cost'), ('violations', 'violations')):
        assert np.array_equal(getattr(got, mine), getattr(ref, theirs)), mine
    assert got.violations.sum() > 0


def test_oracle_block_product_is_the_short_form():
    """[a b I] sigma_all [a b I]^T = H Sigma H^T + diag(var), H = a + b K + J_x + J_u K, and diag(sigma_g) = var +
    diag(M Sigma M^T), M = J_x + J_u K: to 1e-14 of the largest entry, along a whole rollout."""
    spec, gp, prob, x0, safe, tail = _oracle_case()
    got = perf_taylor_rollout(prob, gp, x0, safe, tail, 1)
    n_s = prob.n_s
    sigma = np.zeros((safe.shape[0], n_s, n_s))
    for t in range(got.traj.shape[1]):
        _, var, jac = gp.predict(got.queries[:, t], jacobians=True)
        m = jac[:, :, :n_s] + jac[:, :, n_s:] @ prob.k_fb
        h = prob.a + prob.b @ prob.k_fb + m
        g = var + np.einsum('pij,pjk,pik->pi', m, sigma, m)
        nxt = h @ sigma @ np.swapaxes(h, 1, 2) + var[:, :, None] * np.eye(n_s)[None]
        sigma_g, blocks = block_step(prob, sigma, var, jac)
        for a, b in ((blocks, nxt), (got.cov[:, t], nxt), (np.diagonal(sigma_g, axis1=1, axis2=2), g), (got.sigma[:, t], g)):
            assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max(), t
        sigma = got.cov[:, t]


def test_oracle_terminal_safety():
    spec, gp, prob, x0, safe, tail = _oracle_case()
    H = safe.shape[1]
    off, on = perf_taylor_rollout(prob, gp, x0, safe, tail, 1), perf_taylor_rollout(prob, gp, x0, safe, tail, 1, True)
    assert tuple(off.distances.shape) == (safe.shape[0], prob.h_mat.shape[0])
    s = H + 2
    for c in range(safe.shape[0]):
        mu, cov = off.traj[c, s - 1], off.cov[c, s - 1]
        d = prob.h_mat @ mu + np.sqrt(np.einsum('mi,ij,mj->m', prob.h_mat, cov, prob.h_mat)) - prob.h_vec.reshape(-1)
        np.testing.assert_allclose(off.distances[c], d, rtol=1e-13, atol=1e-15)
    assert np.array_equal(on.con_cost, off.con_cost + ocem.STATE_VIOLATION_COST * off.unsafe)
    assert np.array_equal(off.con_cost, ocem.ACTION_VIOLATION_COST * off.violations)
    with pytest.raises(ValueError, match='n_perf'):
        perf_taylor_rollout(prob, gp, x0, safe, tail[:, :H], 1, True)          # n_perf = H + 1
    assert perf_taylor_rollout(prob, gp, x0, safe, tail[:, :H], 1).distances is None


# ---- the entries -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name in (NAME, FORM):
        assert re.search(r'\bint ' + name + r'\(', header)
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        doc = header[:header.index('int ' + name + '(')].rsplit('/*', 1)[1]
        assert 'uncertainty_propagation_casadi.py:11-149' in doc and 'safempc_simple.py:471-479' in doc, name
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == 21
    assert argtypes[2:7] == [ctypes.c_int] * 5 and argtypes[7:18] == [ctypes.c_void_p] * 11
    assert argtypes[18] is ctypes.c_int and argtypes[19:] == [ctypes.c_void_p] * 2
    assert _lib.SIGNATURES[FORM][1][1:] == [ctypes.c_int]
    assert callable(cem_mpc.cem_perf_rollout_taylor)


def _call(model, env, *, E=1, P=4, H=5, n_perf=8, r=1, x0=16, safe=16, mean=16, std=16, noise=16, rows=16, obj=16, con=16,
          status=16, terminal=0):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return _lib.lib().sx_cem_perf_rollout_taylor(None if model is None else ctypes.byref(model),
                                                 None if env is None else ctypes.byref(env), E, P, H, n_perf, r, p(x0),
                                                 p(safe), p(mean), p(std), p(noise), p(rows), p(obj), p(con), None, None, None,
                                                 terminal, p(status), None)


@pytest.mark.parametrize('obj_mode', [VAR, ABS])
def test_argument_errors_without_a_gpu(obj_mode):
    m, env = _model(), _env(obj_mode=obj_mode)
    for kw in (dict(x0=None), dict(safe=None), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None),
               dict(mean=None), dict(std=None), dict(E=0), dict(P=0), dict(H=0), dict(r=0), dict(r=6), dict(n_perf=1),
               dict(n_perf=3, r=3), dict(terminal=1, n_perf=6), dict(terminal=1, n_perf=5, r=2)):
        assert _call(m, env, **kw) == _lib.SX_ERR_ARG, kw
    assert _call(None, env) == _lib.SX_ERR_ARG and _call(m, None) == _lib.SX_ERR_ARG
    assert _call(_model(n_train=0), env) == _lib.SX_ERR_ARG
    assert _call(_model(2, 2), env) == _lib.SX_ERR_ARG                  # model and env disagree on the shape
    for field in ('x_train', 'a_pack', 'stage_tab'):
        bad = _model()
        setattr(bad, field, None)
        assert _call(bad, env) == _lib.SX_ERR_ARG, field
    assert _call(m, _env(obj_mode=7)) == _lib.SX_ERR_ARG
    no_rows = _env(obj_mode=obj_mode)
    no_rows.m = 0
    assert _call(m, no_rows, terminal=1, n_perf=7) == _lib.SX_ERR_ARG    # nothing to check against
    # a shape without a rollout kernel; training sets beyond the output-by-output form; one output has no such form:
    assert _call(_model(3, 2), _env(3, 2, obj_mode)) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(n_train=1100), env) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(n_train=1100), env, terminal=1, n_perf=7) == _lib.SX_ERR_UNSUPPORTED
    # (1, 1) keeps its one output in LDS up to N = 1021 (n_pad = 1024); N = 1000 has a form, and was refused here only for
    # want of a device to launch on -- on a GPU host that call launched over these pointers
    assert _call(_model(1, 1, n_train=1022), _env(1, 1, obj_mode)) == _lib.SX_ERR_UNSUPPORTED


def test_the_form_query_without_a_gpu():
    form = lambda m, n_perf=8: int(_lib.lib().sx_cem_perf_rollout_taylor_form(None if m is None else ctypes.byref(m), n_perf))
    SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
    assert form(_model(n_train=200)) == SX_FORM_STREAM and form(_model(n_train=590)) == SX_FORM_BYOUT
    assert form(_model(n_train=1100)) < 0 and form(None) < 0 and form(_model(), 1) < 0 and form(_model(3, 2)) < 0
    bad = _model()
    bad.a_pack = None
    assert form(bad) < 0
    # the variance kernel's rule over its LDS plus the step constants: the same answers away from the boundary
    for n in (7, 200, 400, 590, 1000, 1100):
        assert form(_model(n_train=n), 15) == int(_lib.lib().sx_cem_perf_rollout_var_form(ctypes.byref(_model(n_train=n)), 15))


# ---- FusedCemMpc -------------------------------------------------------------------------------------------------------------
def test_fused_cem_mpc_settings_raise_what_they_must():
    mk = lambda env=None, **kw: FusedCemMpc(_Ssm(), env or _env(), 5, 64, 8, 3, device='cpu', **kw)
    mpc = mk(n_perf=6, perf_type='taylor')                       # carries the variance objective by itself
    mpc.set_env(_env(obj_mode=ABS))
    mpc.set_env(_env(obj_mode=VAR))
    assert mpc._perf.type == 'taylor' and not mpc._perf.terminal_safety and not mpc._perf.variance
    assert mk(n_perf=7, perf_type='taylor', perf_terminal_safety=True)._perf.terminal_safety
    with pytest.raises(ValueError, match='perf_type'):
        mk(n_perf=6, perf_type='unscented')
    for kw in (dict(), dict(n_perf=0)):
        with pytest.raises(ValueError, match='taylor'):
            mk(perf_type='taylor', **kw)
    with pytest.raises(ValueError, match='n_perf'):
        mk(n_perf=6, perf_type='taylor', perf_terminal_safety=True)          # H + 2 = 7
    with pytest.raises(ValueError, match='taylor'):
        mk(_env(obj_mode=ABS), n_perf=7, perf_terminal_safety=True)
    with pytest.raises(ValueError, match='variance objective'):               # the parent's refusal stays
        mk(n_perf=6, perf_type='mean_equivalent')
    with pytest.raises(NotImplementedError, match='exact RBF'):
        FusedCemMpc(_Ssm('feature'), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_type='taylor')
    with mock.patch.object(_lib, 'require_gpu', lambda *a: None), pytest.raises(ValueError, match='n_perf'):
        cem_mpc.cem_perf_rollout_taylor(_Ssm(), _env(), torch.zeros((1, 2), dtype=torch.float64), 5, 6, 1, safe_actions=None,
                                        obj_cost=None, con_cost=None, status=None, terminal_safety=True)


def _taylor_fake(seen):
    inner = _perf_fake(seen, 'perf_taylor')

    def perf(*a, **kw):
        out = inner(*a, **kw)
        if kw.get('want_cov'):
            out['perf_cov'] = torch.zeros((E_, P_, N_PERF, 2, 2), dtype=torch.float64) + 2
        else:
            out['perf_cov'] = None
        return out
    return perf


@pytest.mark.parametrize('record', [False, True])
@pytest.mark.parametrize('safety', [False, True])
def test_with_the_setting_every_iteration_calls_the_taylor_rollout(monkeypatch, record, safety):
    seen = []
    _fakes(monkeypatch, 8, seen)
    for name in ('cem_perf_rollout', 'cem_perf_rollout_var'):
        monkeypatch.setattr(cem_mpc, name, mock.Mock(side_effect=AssertionError(name)))
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout_taylor', _taylor_fake(seen))
    mpc = FusedCemMpc(_Ssm(), _env(), H_, P_, 8, ITERS, device='cpu', init_std=0.2, n_perf=N_PERF, perf_r=R_,
                      perf_type='taylor', perf_terminal_safety=safety, record_rollouts=record)
    noise = torch.randn((ITERS, E_, P_, H_ + T_, 1), dtype=torch.float64)
    best, ok, history, _ = mpc.solve(torch.zeros((E_, 2), dtype=torch.float64), noise=noise)
    assert tuple(best.shape) == (E_, H_ + T_, 1)
    assert [s[0] for s in seen] == ['rollout', 'perf_taylor', 'rank'] * ITERS
    for s in seen:
        if s[0] == 'perf_taylor':
            assert s[1:] == (H_, N_PERF, R_, (E_, P_, H_, 1), (E_, T_, 1), (E_, T_, 1), (E_, P_, T_, 1), record,
                             dict(want_sigma=record, want_cov=record, terminal_safety=safety))
    assert len(history) == (ITERS * E_ if record else 0)
    for h in history:
        assert tuple(h.perf_cov.shape) == (P_, N_PERF, 2, 2) and bool((h.perf_cov == 2).all())
        assert tuple(h.perf_sigma.shape) == (P_, N_PERF, 2)


def test_the_library_entry_a_solve_reaches():
    """Through the real wrappers with a mocked library: 21 arguments, the flag in its place."""
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        _fakes(mp, 8, seen)
        fake = mock.Mock()
        fake.sx_cem_perf_rollout_taylor.return_value = _lib.SX_OK
        with mock.patch.object(_lib, 'lib', lambda: fake), mock.patch.object(_lib, 'require_gpu', lambda *a: None), \
                mock.patch.object(_lib, 'stream_ptr', lambda dev: None):
            mpc = FusedCemMpc(_Ssm(), _env(obj_mode=ABS), H_, P_, 8, ITERS, device='cpu', init_std=0.2, n_perf=N_PERF,
                              perf_r=R_, perf_type='taylor', perf_terminal_safety=True)
            mpc.solve(torch.zeros((E_, 2), dtype=torch.float64))
    entry = fake.sx_cem_perf_rollout_taylor
    assert entry.call_count == ITERS and fake.sx_cem_perf_rollout.call_count == fake.sx_cem_perf_rollout_var.call_count == 0
    args = entry.call_args[0]
    assert len(args) == 21 and args[2:7] == (E_, P_, H_, N_PERF, R_) and args[18] == 1


@pytest.mark.parametrize('kw', [dict(), dict(n_perf=0), dict(n_perf=N_PERF, perf_r=R_),
                                dict(n_perf=N_PERF, perf_r=R_, perf_type='mean_equivalent', perf_terminal_safety=False),
                                dict(n_perf=N_PERF, perf_r=R_, perf_variance=True)])
def test_without_the_settings_a_solve_calls_what_it_called(monkeypatch, kw):
    seen = []
    _fakes(monkeypatch, 8, seen)
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout', _perf_fake(seen, 'perf'))
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout_var', _perf_fake(seen, 'perf_var'))
    taylor = mock.Mock()
    monkeypatch.setattr(cem_mpc, 'cem_perf_rollout_taylor', taylor)
    mpc = FusedCemMpc(_Ssm(), _env(obj_mode=ABS), H_, P_, 8, ITERS, device='cpu', init_std=0.2, **kw)
    mpc.solve(torch.zeros((E_, 2), dtype=torch.float64))
    assert taylor.call_count == 0
    middle = [] if kw.get('n_perf', 0) <= 0 else ['perf_var'] if kw.get('perf_variance') else ['perf']
    assert [s[0] for s in seen] == (['rollout'] + middle + ['rank']) * ITERS
    for s in seen:
        if s[0] == 'perf':       # the keyword arguments of the parent's call, no more
            assert s[1:] == (H_, N_PERF, R_, (E_, P_, H_, 1), (E_, T_, 1), (E_, T_, 1), (E_, P_, T_, 1), False, {})
        if s[0] == 'perf_var':
            assert s[-1] == dict(want_sigma=False)


# ---- CemSafeMPC and get_actions_multi --------------------------------------------------------------------------------------
def test_cem_safempc_reads_the_settings():
    solver = _safempc(conf(cem_n_perf=6, cem_perf_type='taylor'), objective_target=None)      # exploration: no objective
    assert solver.performance_trajectory_length == 6 and solver._perf.type == 'taylor'
    assert _safempc(conf(cem_n_perf=7, cem_perf_type='taylor', cem_perf_terminal_safety=True))._perf.terminal_safety
    plain = _safempc(conf(cem_n_perf=6))
    assert plain._perf.type == 'mean_equivalent' and not plain._perf.terminal_safety
    # the casadi solver's settings stay unread
    assert _safempc(conf(type_perf_traj='taylor', perf_safety_constr=True))._perf.type == 'mean_equivalent'
    with pytest.raises(ValueError, match='cem_perf_type'):
        _safempc(conf(cem_n_perf=6, cem_perf_type='unscented'))
    with pytest.raises(ValueError, match='cem_n_perf'):
        _safempc(conf(cem_perf_type='taylor'))
    with pytest.raises(ValueError, match='cem_n_perf'):
        _safempc(conf(cem_n_perf=6, cem_perf_type='taylor', cem_perf_terminal_safety=True))     # mpc_time_horizon + 2 = 7
    with pytest.raises(ValueError, match='taylor'):
        _safempc(conf(cem_n_perf=7, cem_perf_terminal_safety=True))
    with pytest.raises(ValueError, match='variance objective'):
        _safempc(conf(cem_n_perf=6, cem_perf_type='mean_equivalent'), objective_target=None)


def _built_solver(c):
    from safe_exploration_amd.safempc_cem import CemSafeMPC, construct_constraints
    spec = problems.pendulum(n_train=8)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=None)
    ssm = mock.Mock()
    ssm.kernel_family, ssm.num_states, ssm.num_actions = 'rbf', 2, 1
    lqr = mock.Mock()
    lqr.get_control_matrix.return_value = spec.k_fb
    return CemSafeMPC(ssm, construct_constraints(c, env), env, c, {'lin_model': (spec.a, spec.b)}, wx_feedback_cost=None,
                      wu_feedback_cost=None, lqr=lqr, beta_safety=2.0, safe_policy=lambda x: spec.k_fb @ x)


def test_cem_safempc_builds_the_solver_with_the_settings():
    solver = _built_solver(conf(cem_n_perf=7, cem_perf_type='taylor', cem_perf_terminal_safety=True))
    with mock.patch.object(safempc_cem, 'FusedCemMpc') as fused:
        solver._solver()
    kw = fused.call_args[1]
    assert kw['n_perf'] == 7 and kw['perf_type'] == 'taylor' and kw['perf_terminal_safety'] is True
    assert 'perf_variance' not in kw
    sx_env, hook = fused.return_value.set_env.call_args[0][0], fused.return_value.set_env.call_args[1]['objective_hook']
    assert sx_env.obj_mode == VAR and hook is None
    # without the settings: the keyword arguments of the parent's construction, no more
    plain = _built_solver(conf(cem_n_perf=6, cem_perf_variance=True))
    with mock.patch.object(safempc_cem, 'FusedCemMpc') as fused:
        plain._solver()
    assert sorted(fused.call_args[1]) == sorted(['device', 'seed', 'init_std', 'warm_start', 'record_rollouts', 'n_perf',
                                                 'perf_r', 'perf_variance'])


def test_multi_model_solves_go_one_model_at_a_time():
    mpcs = [FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_type='taylor') for _ in range(2)]
    with mock.patch.object(cem_mpc, 'multi_family', lambda ssms: 'rbf'):
        multi = MultiModelPerfCemMpc.from_solvers(mpcs)
        assert multi.fused_applies() is False
        with pytest.raises(cem_mpc.FusedMultiUnsupported, match='taylor'):
            multi.solve(torch.zeros((2, 2), dtype=torch.float64))
        per = [(torch.full((1, 6 + 5 - 1, 1), float(e)), torch.ones(1, dtype=torch.bool)) for e in range(2)]
        for e, s in enumerate(mpcs):
            s._solve_checked = mock.Mock(return_value=per[e])
        best, found = multi.get_actions_multi(torch.zeros((2, 6), dtype=torch.float64))
        assert multi.per_model_solves == 1 and all(s._solve_checked.call_count == 1 for s in mpcs)
        assert tuple(best.shape) == (2, 5, 1) and bool(found.all())
    # solvers that differ in the setting are refused, as for every other setting of the performance trajectory
    mixed = [mpcs[0], FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', n_perf=6, perf_variance=True)]
    with pytest.raises(ValueError, match='perf_type'):
        cem_mpc.MultiModelCemMpc.check_solvers(mixed)


def test_get_actions_multi_refuses_mixed_settings_and_routes_shared_ones(monkeypatch):
    solvers = [_safempc(conf(cem_n_perf=6, cem_perf_type='taylor'), objective_target=None),
               _safempc(conf(cem_n_perf=6, cem_perf_variance=True), objective_target=None)]
    with pytest.raises(ValueError, match='cem_perf_type'):
        get_actions_multi(solvers, np.zeros((2, 2)))
    # a shared 'taylor' setting: MultiModelPerfCemMpc is built from the solvers' optimisers and asked
    solvers = [_safempc(conf(cem_n_perf=6, cem_perf_type='taylor'), objective_target=None, mpc=mock.Mock()) for _ in range(2)]
    for s in solvers:
        monkeypatch.setattr(s, '_solver', lambda s=s: s._mpc)
        monkeypatch.setattr(s, '_flat_points', lambda st: torch.zeros((1, 6), dtype=torch.float64))
        monkeypatch.setattr(s, '_batch_ladder', lambda i, st, best, found: (best[0], 'found' if found else 'none'))
    built = mock.Mock()
    built.solvers = [s._mpc for s in solvers]
    built.get_actions_multi.return_value = (torch.zeros((2, 5, 1), dtype=torch.float64), [True, True])
    perf_cls = mock.Mock()
    perf_cls.from_solvers.return_value = built
    monkeypatch.setattr(safempc_cem, 'MultiModelPerfCemMpc', perf_cls)
    monkeypatch.setattr(safempc_cem.MultiModelCemMpc, 'check_solvers', staticmethod(lambda mpcs: None))
    monkeypatch.setattr(safempc_cem, 'multi_solve_applies', lambda mpcs: True)
    actions, results = get_actions_multi(solvers, np.zeros((2, 2)))
    assert perf_cls.from_solvers.call_count == 1 and built.get_actions_multi.call_count == 1
    assert actions.shape == (2, 1) and results == ['found', 'found']
