"""CPU: Cautious MPC, host side -- the numpy oracle (tests/cautious_oracle.py) against a hand-multiplied covariance step
and at T = 1; sx_cem_cautious_rollout and its form query are declared, exported and check their arguments before any device
access; the wrapper's argument checks; the ladder and the warm start of CautiousCemMPC over an injected fake optimiser."""
import ctypes
import dataclasses
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from cautious_oracle import box_rows, cautious_rollout, cem_solve_cautious, distances_at
from oracle import cem as ocem
from oracle.gp import ExactGP
from perf_taylor_oracle import block_step, perf_taylor_rollout
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cautious_mpc import CautiousCemMPC
from safe_exploration_amd.cem_mpc import CautiousCemMpc
from safe_exploration_amd.safempc_cem import MpcResult
from test_perf_var_host import _env, _model, _Ssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, FORM = 'sx_cem_cautious_rollout', 'sx_cem_cautious_rollout_form'
VAR, ABS = _lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS


# ---- the numpy oracle ------------------------------------------------------------------------------------------------------
def _oracle_case(obj_mode=VAR, T=6, beta=2.0):
    spec = problems.pendulum(n_train=30, obj_mode=obj_mode, beta=beta)
    gp = ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)
    rng = np.random.default_rng(5)
    return spec, gp, problems.oracle_problem(spec, ocem), np.array([0.03, -0.02]), rng.normal(0, 0.8, size=(11, T, 1))


def test_block_form_against_the_hand_multiplied_step():
    """[a b I] sigma_all [a b I]^T against Hm Sigma Hm^T + diag(var), and diag(sigma_g) against var + diag(M Sigma M^T), on
    random inputs: to 1e-13 of the largest entry."""
    rng = np.random.default_rng(0)
    for n_s, n_u in ((2, 1), (4, 1), (2, 2), (3, 2)):
        P = 9
        prob = ocem.Problem(n_s, n_u, rng.normal(size=(n_s, n_s)), rng.normal(size=(n_s, n_u)), rng.normal(size=(n_u, n_s)),
                            np.zeros(n_s), np.zeros(n_s), 2.0, np.zeros((0, n_s)), np.zeros((0, 1)), -np.ones(n_u),
                            np.ones(n_u))
        root = rng.normal(size=(P, n_s, n_s))
        sigma = root @ np.swapaxes(root, 1, 2)
        var, jac = rng.uniform(0.1, 1.0, size=(P, n_s)), rng.normal(size=(P, n_s, n_s + n_u))
        m = jac[:, :, :n_s] + jac[:, :, n_s:] @ prob.k_fb
        hm = prob.a + prob.b @ prob.k_fb + m
        want_next = hm @ sigma @ np.swapaxes(hm, 1, 2) + var[:, :, None] * np.eye(n_s)[None]
        want_g = var + np.einsum('pij,pjk,pik->pi', m, sigma, m)
        sigma_g, nxt = block_step(prob, sigma, var, jac)
        assert np.abs(nxt - want_next).max() <= 1e-13 * np.abs(want_next).max()
        assert np.abs(np.diagonal(sigma_g, axis1=1, axis2=2) - want_g).max() <= 1e-13 * np.abs(want_g).max()


def test_one_step_is_the_plain_box_and_the_gp_variance():
    spec, gp, prob, x0, rows = _oracle_case(T=1)
    got = cautious_rollout(prob, gp, x0, rows)
    _, var0, _ = gp.predict(np.concatenate((np.broadcast_to(x0, (11, 2)), rows[:, 0]), axis=1), jacobians=True)
    assert np.array_equal(got.cov[:, 0], var0[:, :, None] * np.eye(2)[None]) and np.array_equal(got.sigma[:, 0], var0)
    box = ((rows[:, 0] < prob.u_min[None]) | (rows[:, 0] > prob.u_max[None])).any(axis=1)
    assert np.array_equal(got.ctrl_viol[:, 0], box) and box.any() and not box.all()
    assert np.array_equal(got.spread, np.zeros_like(got.spread))
    d = prob.h_mat @ got.traj[0, 0] + prob.beta * np.sqrt(np.einsum('mi,i,mi->m', prob.h_mat, var0[0], prob.h_mat)) \
        - prob.h_vec.reshape(-1)
    np.testing.assert_allclose(got.state_d[0, 0], d, rtol=1e-13, atol=1e-15)
    assert np.array_equal(got.con_cost, 3.0 * got.ctrl_viol.sum(axis=1) + 10.0 * got.state_viol.sum(axis=1))
    # mean-equivalent: the same single step
    me = cautious_rollout(prob, gp, x0, rows, propagate=False)
    for name in ('traj', 'sigma', 'cov', 'state_d', 'ctrl_d', 'con_cost', 'obj_cost'):
        assert np.array_equal(getattr(me, name), getattr(got, name)), name


@pytest.mark.parametrize('obj_mode', [VAR, ABS])
def test_oracle_trajectory_is_the_taylor_oracles(obj_mode):
    """With H = r = 1, n_perf = T the Taylor oracle's trajectory, covariances and objective, bit for bit; the control
    distances are the box rows' ellipsoid distances; mean-equivalent carries diag(var) only."""
    spec, gp, prob, x0, rows = _oracle_case(obj_mode)
    got = cautious_rollout(prob, gp, x0, rows)
    ref = perf_taylor_rollout(prob, gp, x0, rows[:, :1], rows[:, 1:], 1)
    for mine, theirs in (('traj', 'traj'), ('sigma', 'sigma'), ('cov', 'cov'), ('var', 'var'), ('obj_cost', 'obj_cost')):
        assert np.array_equal(getattr(got, mine), getattr(ref, theirs)), mine
    hu, bu = box_rows(prob)
    for t in range(1, rows.shape[1]):
        s = prob.beta * np.sqrt(np.einsum('ci,pij,cj->pc', prob.k_fb, got.cov[:, t - 1], prob.k_fb))
        np.testing.assert_allclose(got.spread[:, t], s, rtol=1e-13, atol=0)
        want = np.concatenate((rows[:, t] + s - prob.u_max[None], prob.u_min[None] - rows[:, t] + s), axis=1)
        np.testing.assert_allclose(got.ctrl_d[:, t], want, rtol=1e-12, atol=1e-15)
    assert (got.spread[:, 1:] > 0).all()
    np.testing.assert_allclose(distances_at(prob, x0, rows, got.traj, got.cov), got.margins, rtol=1e-12, atol=1e-15)
    me = cautious_rollout(prob, gp, x0, rows, propagate=False)
    assert np.array_equal(me.sigma, me.var)
    assert np.array_equal(me.cov, me.var[..., None] * np.eye(2)[None, None])
    no_rows = dataclasses.replace(prob, h_mat=np.zeros((0, 2)), h_vec=np.zeros((0, 1)))
    free = cautious_rollout(no_rows, gp, x0, rows)
    assert not free.state_viol.any() and np.isneginf(free.margins[..., 0]).all()
    best, trace = cem_solve_cautious(no_rows, gp, x0, np.random.default_rng(1).normal(size=(3, 40, 4, 1)), 8, 0.3)
    assert best is not None and len(trace) == 3 and tuple(best.shape) == (4, 1)


# ---- the entries -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name in (NAME, FORM):
        assert re.search(r'\bint ' + name + r'\(', header)
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        doc = header[:header.index('int ' + name + '(')].rsplit('/*', 1)[1]
        assert 'cautious_mpc.py' in doc, name
    doc = header[:header.index('int ' + NAME + '(')].rsplit('/*', 1)[1]
    assert 'cautious_mpc.py:337-442' in doc
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == 19
    assert argtypes[2:5] == [ctypes.c_int] * 3 and argtypes[5:16] == [ctypes.c_void_p] * 11
    assert argtypes[16] is ctypes.c_int and argtypes[17:] == [ctypes.c_void_p] * 2
    assert _lib.SIGNATURES[FORM][1][1:] == [ctypes.c_int]
    assert callable(cem_mpc.cem_cautious_rollout)


def _call(model, env, *, E=1, P=4, T=8, x0=16, mean=16, std=16, noise=16, rows=16, obj=16, con=16, status=16, propagate=1):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return _lib.lib().sx_cem_cautious_rollout(None if model is None else ctypes.byref(model),
                                              None if env is None else ctypes.byref(env), E, P, T, p(x0), p(mean), p(std),
                                              p(noise), p(rows), p(obj), p(con), None, None, None, None, propagate, p(status),
                                              None)


@pytest.mark.parametrize('obj_mode', [VAR, ABS])
def test_argument_errors_without_a_gpu(obj_mode):
    m, env = _model(), _env(obj_mode=obj_mode)
    for kw in (dict(x0=None), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None), dict(mean=None),
               dict(std=None), dict(E=0), dict(P=0), dict(T=0), dict(T=-3)):
        assert _call(m, env, **kw) == _lib.SX_ERR_ARG, kw
    assert _call(None, env) == _lib.SX_ERR_ARG and _call(m, None) == _lib.SX_ERR_ARG
    assert _call(_model(n_train=0), env) == _lib.SX_ERR_ARG
    assert _call(_model(2, 2), env) == _lib.SX_ERR_ARG                  # model and env disagree on the shape
    for field in ('x_train', 'a_pack', 'stage_tab'):
        bad = _model()
        setattr(bad, field, None)
        assert _call(bad, env) == _lib.SX_ERR_ARG, field
    assert _call(m, _env(obj_mode=7)) == _lib.SX_ERR_ARG
    neg = _env(obj_mode=obj_mode)
    neg.m = -1
    assert _call(m, neg) == _lib.SX_ERR_ARG
    many = _env(obj_mode=obj_mode)
    many.m = _lib.SX_MAX_M + 1
    assert _call(m, many) == _lib.SX_ERR_UNSUPPORTED
    # a shape without a rollout kernel; training sets beyond the output-by-output form; one output has no such form:
    assert _call(_model(3, 2), _env(3, 2, obj_mode)) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(n_train=1100), env) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_model(n_train=1100), env, noise=None, mean=None, std=None) == _lib.SX_ERR_UNSUPPORTED
    # (1, 1) keeps its one output in LDS up to N = 1021 (n_pad = 1024); N = 1000 has a form, and was refused here only for
    # want of a device to launch on -- on a GPU host that call launched over these pointers
    assert _call(_model(1, 1, n_train=1022), _env(1, 1, obj_mode)) == _lib.SX_ERR_UNSUPPORTED


def test_the_form_query_without_a_gpu():
    form = lambda m, T=8: int(_lib.lib().sx_cem_cautious_rollout_form(None if m is None else ctypes.byref(m), T))
    taylor = lambda m, n: int(_lib.lib().sx_cem_perf_rollout_taylor_form(ctypes.byref(m), n))
    SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
    assert form(_model(n_train=200)) == SX_FORM_STREAM and form(_model(n_train=590)) == SX_FORM_BYOUT
    assert form(_model(n_train=1100)) < 0 and form(None) < 0 and form(_model(), 0) < 0 and form(_model(3, 2)) < 0
    assert form(_model(), 1) == SX_FORM_STREAM               # one step is a rollout here
    bad = _model()
    bad.a_pack = None
    assert form(bad) < 0
    # the Taylor kernel's rule over one more constant: the same answers away from the boundary
    for n in (7, 200, 400, 590, 1000, 1100):
        assert form(_model(n_train=n), 15) == taylor(_model(n_train=n), 15)


# ---- the wrapper -----------------------------------------------------------------------------------------------------------
def test_wrapper_argument_checks():
    z = lambda *s: torch.zeros(s, dtype=torch.float64)
    ssm, env, x0 = _Ssm(), _env(), z(2, 2)
    fake = mock.Mock()
    fake.sx_cem_cautious_rollout.return_value = _lib.SX_OK
    with mock.patch.object(_lib, 'require_gpu', lambda *a: None), mock.patch.object(_lib, 'lib', lambda: fake), \
            mock.patch.object(_lib, 'stream_ptr', lambda dev: None):
        call = lambda T=3, **kw: cem_mpc.cem_cautious_rollout(ssm, env, x0, T, **kw)
        for kw, word in ((dict(T=0, rows=z(2, 4, 3, 1)), 'T'), (dict(noise=z(2, 4, 3, 1)), 'mean and std'),
                         (dict(noise=z(2, 4, 3, 1), mean=z(2, 3, 1), std=z(2, 3, 1), rows=z(2, 4, 3, 1)), 'not both'),
                         (dict(noise=z(2, 4, 2, 1), mean=z(2, 3, 1), std=z(2, 3, 1)), 'noise'),
                         (dict(noise=z(2, 4, 3, 1), mean=z(2, 2, 1), std=z(2, 3, 1)), 'mean'),
                         (dict(noise=z(2, 4, 3, 1), mean=z(2, 3, 1), std=z(1, 3, 1)), 'std'),
                         (dict(), 'rows'), (dict(rows=z(2, 4, 3, 2)), 'rows'), (dict(rows=z(1, 4, 3, 1)), 'rows')):
            with pytest.raises(ValueError, match=word):
                call(**kw)
        with pytest.raises(ValueError, match='x0'):
            cem_mpc.cem_cautious_rollout(ssm, env, z(2, 3), 3, rows=z(2, 4, 3, 1))
        assert fake.sx_cem_cautious_rollout.call_count == 0
        with pytest.raises(NotImplementedError, match='exact RBF'):
            cem_mpc.cem_cautious_rollout(_Ssm('feature'), env, x0, 3, rows=z(2, 4, 3, 1))
        out = call(noise=z(2, 4, 3, 1), mean=z(2, 3, 1), std=z(2, 3, 1), want_traj=True, want_margins=True, propagate=False)
        args = fake.sx_cem_cautious_rollout.call_args[0]
        assert len(args) == 19 and args[2:5] == (2, 4, 3) and args[16] == 0
        assert tuple(out['rows'].shape) == (2, 4, 3, 1) and tuple(out['traj'].shape) == (2, 4, 3, 2)
        assert tuple(out['margins'].shape) == (2, 4, 3, 2) and out['sigma'] is None and out['cov'] is None
        assert tuple(out['con_cost'].shape) == (2, 4)
        fake.sx_cem_cautious_rollout.return_value = _lib.SX_ERR_UNSUPPORTED
        with pytest.raises(_lib.SxError, match='no form of the cautious'):
            call(rows=z(2, 4, 3, 1))
        fake.sx_cem_cautious_rollout.return_value = _lib.SX_ERR_ARG
        with pytest.raises(_lib.SxError):
            call(rows=z(2, 4, 3, 1))


def test_cautious_cem_mpc_settings_raise_what_they_must():
    mk = lambda ssm=None, **kw: CautiousCemMpc(ssm or _Ssm(), _env(), 5, 64, 8, 3, device='cpu', **kw)
    assert mk().num_iterations == 3 and mk(propagate=False)._propagate is False
    with pytest.raises(NotImplementedError, match='exact RBF'):
        mk(_Ssm('feature'))
    with pytest.raises(NotImplementedError, match='process group'):
        mk(process_group=object())
    with pytest.raises(ValueError, match='ONE model'):
        mk([_Ssm(), _Ssm()])
    with pytest.raises(ValueError, match='num_elites'):
        CautiousCemMpc(_Ssm(), _env(), 5, 64, 65, 3, device='cpu')
    with pytest.raises(ValueError, match='time_horizon'):
        CautiousCemMpc(_Ssm(), _env(), 0, 64, 8, 3, device='cpu')


def test_a_solve_is_one_rollout_and_one_ranking_per_iteration(monkeypatch):
    seen = []
    E, P, T, iters = 2, 64, 5, 3

    def rollout(ssm, env, x0, T_, *, mean, std, noise, propagate, status, **kw):
        seen.append(('rollout', T_, tuple(mean.shape), tuple(noise.shape), propagate, kw))
        z = torch.zeros((E, P), dtype=torch.float64)
        return dict(rows=mean.unsqueeze(1) + std.unsqueeze(1) * noise, obj_cost=z, con_cost=z, traj=None, sigma=None,
                    cov=None, margins=None, status=status)

    def rank(con, obj, rows, k, **kw):
        seen.append(('rank', k, kw))
        return dict(mean=torch.zeros((E, T)), std=torch.ones((E, T)), best=rows[:, 0].reshape(E, -1),
                    best_ok=torch.ones(E, dtype=torch.int32), elite_rows=None)

    monkeypatch.setattr(cem_mpc, 'cem_cautious_rollout', rollout)
    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)
    mpc = CautiousCemMpc(_Ssm(), _env(), T, P, 8, iters, device='cpu', init_std=0.2, propagate=False)
    init = torch.full((E, T, 1), 0.5, dtype=torch.float64)
    best, ok, history, status = mpc.solve(torch.zeros((E, 2), dtype=torch.float64), init_mean=init)
    assert [s[0] for s in seen] == ['rollout', 'rank'] * iters and tuple(best.shape) == (E, T, 1) and history == []
    assert seen[0][1:5] == (T, (E, T, 1), (E, P, T, 1), False)
    assert seen[0][5] == dict(want_traj=False, want_sigma=False, want_cov=False)
    assert seen[1][1:] == (8, dict(want_refit=True))
    with pytest.raises(ValueError, match='noise'):
        mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=torch.zeros((iters, E, P, T + 1, 1), dtype=torch.float64))


# ---- CautiousCemMPC: the ladder and the warm start -------------------------------------------------------------------------
class Conf:
    T = 4
    beta_safety = 2.0
    type_perf_traj = 'taylor'
    cem_num_rollouts = 64
    cem_num_elites = 8
    cem_num_iterations = 3
    device = 'cpu'


class FakeMpc:
    """Answers get_actions / get_actions_batch from a script of rows (None: nothing found) and keeps what it was asked."""

    def __init__(self, script):
        self.script, self.inits = list(script), []

    def get_actions(self, state, init_mean=None):
        self.inits.append(init_mean.clone())
        row = self.script.pop(0)
        return (None if row is None else torch.tensor(row)), []

    def get_actions_batch(self, states, init_mean=None):
        self.inits.append(init_mean.clone())
        rows = self.script.pop(0)
        T = Conf.T
        best = torch.stack([torch.zeros((T, 1), dtype=torch.float64) if r is None else torch.tensor(r) for r in rows])
        return best, torch.tensor([r is not None for r in rows]), []


def _cautious(script, conf=None, opt_env=None, safe_policy=None):
    spec = problems.pendulum(n_train=8, obj_mode=ABS)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=-0.1)
    lqr = mock.Mock()
    lqr.get_control_matrix.return_value = spec.k_fb
    opt = {'lin_model': (spec.a, spec.b), 'ctrl_bounds': np.array([[-1.0, 1.0]]), 'h_mat_safe': spec.h_mat,
           'h_safe': spec.h_vec, 'h_mat_obs': None, 'h_obs': None}
    opt.update(opt_env or {})
    ssm = mock.Mock()
    ssm.kernel_family, ssm.num_states, ssm.num_actions = 'rbf', 2, 1
    mpc = FakeMpc(script) if script is not None else None
    return CautiousCemMPC(ssm, env, conf or Conf(), opt, None, None, beta_safety=None, safe_policy=safe_policy, lqr=lqr,
                          mpc=mpc), spec


def test_the_ladder_and_the_warm_start():
    row = np.arange(1.0, 5.0).reshape(4, 1)
    solver, spec = _cautious([None, row, None, None, None, None, None, 2 * row])
    mpc, x = solver._mpc, np.array([0.1, -0.2])
    assert solver.n_fail == Conf.T - 1 and np.array_equal(solver.k_fb, spec.k_fb) and solver.beta_safety == 2.0
    solver.init_solver()
    # no solution yet: k_fb x, from a zero start
    action, result = solver.get_action(x)
    assert result == MpcResult.SAFE_CONTROLLER and np.array_equal(action, spec.k_fb @ x) and solver.n_fail == Conf.T
    action, result = solver.get_action(x)
    assert result == MpcResult.FOUND_SOLUTION and np.array_equal(action, row[0]) and solver.n_fail == 0
    assert all(bool((i == 0).all()) for i in mpc.inits[:2])
    # failures: the entries 1, 2, 3 of the kept row, then k_fb x; the first of them starts from the shifted row
    for n in (1, 2, 3):
        action, result = solver.get_action(x)
        assert result == MpcResult.PREVIOUS_SOLUTION and np.array_equal(action, row[n]) and solver.n_fail == n
    for n in (4, 5):
        action, result = solver.get_action(x)
        assert result == MpcResult.SAFE_CONTROLLER and np.array_equal(action, spec.k_fb @ x) and solver.n_fail == n
    assert np.array_equal(mpc.inits[2][0].numpy(), np.array([[2.0], [3.0], [4.0], [4.0]]))
    assert all(bool((i == 0).all()) for i in mpc.inits[3:7])
    action, result = solver.get_action(x)
    assert result == MpcResult.FOUND_SOLUTION and np.array_equal(action, 2 * row[0])
    assert np.array_equal(solver.k_ff_old, 2 * row) and tuple(mpc.inits[-1].shape) == (1, 4, 1)


def test_the_batch_ladder_keeps_an_episode_each():
    row = np.arange(1.0, 5.0).reshape(4, 1)
    solver, spec = _cautious([[row, None], [None, -row], [None, None]], safe_policy=lambda x: np.array([7.0]))
    states = np.array([[0.1, -0.2], [0.0, 0.3]])
    acts, res = solver.get_action_batch(states)
    assert res == [MpcResult.FOUND_SOLUTION, MpcResult.SAFE_CONTROLLER] and acts[0, 0] == 1.0 and acts[1, 0] == 7.0
    acts, res = solver.get_action_batch(states, episode_ids=[0, 1], num_episodes=2)
    assert res == [MpcResult.PREVIOUS_SOLUTION, MpcResult.FOUND_SOLUTION] and acts[0, 0] == 2.0 and acts[1, 0] == -1.0
    init = solver._mpc.inits[1].numpy()
    assert np.array_equal(init[0, :, 0], [2.0, 3.0, 4.0, 4.0]) and not init[1].any()
    acts, res = solver.get_action_batch(states)
    assert res == [MpcResult.PREVIOUS_SOLUTION] * 2 and acts[0, 0] == 3.0 and acts[1, 0] == -2.0
    init = solver._mpc.inits[2].numpy()
    assert not init[0].any() and np.array_equal(init[1, :, 0], [-2.0, -3.0, -4.0, -4.0])


def test_the_settings_the_class_reads():
    solver, spec = _cautious(None)
    env, hook = solver._build_env()
    assert env.m == 0 and not hook and env.beta == 2.0 and env.obj_mode == ABS
    assert (env.u_min[0], env.u_max[0]) == (-1.0, 1.0) and solver._perf_trajectory == 'taylor'
    safe = type('C', (Conf,), dict(cautious_state_polytope='safe', type_perf_traj='mean_equivalent', beta_safety=1.5))()
    solver, spec = _cautious(None, safe)
    env, _ = solver._build_env()
    m = spec.h_mat.shape[0]
    assert env.m == m and np.array_equal(np.array(env.h_mat[:2 * m]).reshape(m, 2), spec.h_mat) and env.beta == 1.5
    assert np.array_equal(np.array(env.h_vec[:m]), spec.h_vec.reshape(-1))
    obs = dict(h_mat_obs=np.array([[1.0, 0.0]]), h_obs=np.array([[0.4]]))
    env, _ = _cautious(None, opt_env=obs)[0]._build_env()
    assert env.m == 1 and env.h_vec[0] == 0.4
    with mock.patch('safe_exploration_amd.cautious_mpc.CautiousCemMpc') as built:
        _cautious(None, safe)[0]._solver()
    assert built.call_args[1]['propagate'] is False and built.call_args[0][2:6] == (4, 64, 8, 3)
    with pytest.raises(NotImplementedError, match='type_perf_traj'):
        _cautious(None, type('C', (Conf,), dict(type_perf_traj='unscented'))())
    with pytest.raises(ValueError, match='cautious_state_polytope'):
        _cautious(None, type('C', (Conf,), dict(cautious_state_polytope='both'))())
    with pytest.raises(ValueError, match='ctrl_bounds'):
        _cautious(None, opt_env=dict(ctrl_bounds=None))
