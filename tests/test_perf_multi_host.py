"""CPU: performance trajectories in multi-model CEM solves, host side -- the entries of the multi-model performance rollout
are declared and exported, check their arguments before any device access and answer their form queries without one; a
MultiModelPerfCemMpc solve makes one safety launch, one performance launch and one ranking per iteration over rows of
H + T steps (fakes in place of the launches); get_actions_multi reaches it over CemSafeMPCs that all have the setting and
refuses mixed or disagreeing lists; every solver keeps its tail as last_perf_actions."""
import collections
import ctypes
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc
from safe_exploration_amd.safempc_cem import CemSafeMPC, get_actions_multi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['sx_cem_perf_table_bytes', 'sx_cem_perf_table', 'sx_cem_perf_rollout_multi', 'sx_cem_perf_rollout_var_multi',
           'sx_cem_perf_rollout_var_form', 'sx_cem_perf_rollout_var_multi_form']
ABS, VAR = _lib.SX_OBJ_AFFINE_ABS, _lib.SX_OBJ_NEG_VARIANCE
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3


@pytest.mark.parametrize('name', ENTRIES)
def test_entries_are_declared_and_exported(name):
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    assert re.search(r'\bint(64_t)? ' + name + r'\(', header)
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.lib(), name)


def _model(n_s=2, n_u=1, n_train=20, packed=True):
    """A model as far as the host reads it: the pointers are never dereferenced (every call below is answered before any
    device access)."""
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.n_pad = (n_train + n_s + n_u) // 16 * 16 + 16
    m.x_train = 16
    if packed:
        m.a_pack, m.stage_tab = 16, 16
    for i in range(n_s * (n_s + n_u)):
        m.inv_ls2[i] = 1.0
    for i in range(n_s):
        m.outputscale[i] = 1.0
    return m


def _models(*ms):
    return (_lib.SxGpModel * len(ms))(*ms)


def _env(n_s=2, n_u=1, obj_mode=ABS):
    env = _lib.SxEnv()
    env.n_s, env.n_u, env.m, env.obj_mode = n_s, n_u, 4, obj_mode
    return env


def _call(entry, models, env, *, E=2, P=4, H=5, n_perf=8, r=1, table=16, x0=16, safe=16, mean=16, std=16, noise=16, rows=16,
          obj=16, con=16, status=16):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    outs = (None,) if entry == 'sx_cem_perf_rollout_multi' else (None, None)
    return getattr(_lib.lib(), entry)(models, p(table), None if env is None else ctypes.byref(env), E, P, H, n_perf, r,
                                      p(x0), p(safe), p(mean), p(std), p(noise), p(rows), p(obj), p(con), *outs, p(status),
                                      None)


@pytest.mark.parametrize('entry', ['sx_cem_perf_rollout_multi', 'sx_cem_perf_rollout_var_multi'])
def test_argument_errors_without_a_gpu(entry):
    ms, env = _models(_model(n_train=20), _model(n_train=70)), _env()
    for kw in (dict(table=None), dict(x0=None), dict(safe=None), dict(rows=None), dict(obj=None), dict(con=None),
               dict(status=None), dict(mean=None), dict(std=None), dict(E=0), dict(P=0), dict(H=0), dict(r=0), dict(r=6),
               dict(n_perf=1), dict(n_perf=3, r=3)):
        assert _call(entry, ms, env, **kw) == _lib.SX_ERR_ARG, kw
    assert _call(entry, None, env) == _lib.SX_ERR_ARG and _call(entry, ms, None) == _lib.SX_ERR_ARG
    assert _call(entry, _models(_model(), _model(n_train=0)), env) == _lib.SX_ERR_ARG
    assert _call(entry, _models(_model(), _model(2, 2)), env) == _lib.SX_ERR_ARG       # the models disagree on the shape
    assert _call(entry, _models(_model(2, 2), _model(2, 2)), env) == _lib.SX_ERR_ARG   # models and env disagree
    no_x = _model()
    no_x.x_train = None
    assert _call(entry, _models(_model(), no_x), env) == _lib.SX_ERR_ARG
    bad_mode = _env(obj_mode=7)
    assert _call(entry, ms, bad_mode) == _lib.SX_ERR_ARG
    # a shape without a rollout kernel
    assert _call(entry, _models(_model(3, 2), _model(3, 2)), _env(3, 2)) == _lib.SX_ERR_UNSUPPORTED


def test_mean_only_entry_refuses_what_the_single_model_entry_refuses():
    entry, env = 'sx_cem_perf_rollout_multi', _env()
    ms = _models(_model(), _model(n_train=70))
    assert _call(entry, ms, _env(obj_mode=VAR)) == _lib.SX_ERR_UNSUPPORTED      # the variance needs the N x N product
    # one training set beyond the kernel's LDS makes the launch unsupported: the launch asks for the largest model's
    assert _call(entry, _models(_model(), _model(n_train=4096)), env) == _lib.SX_ERR_UNSUPPORTED


def test_variance_entry_needs_packed_models_and_a_form_for_each():
    entry, env = 'sx_cem_perf_rollout_var_multi', _env(obj_mode=VAR)
    assert _call(entry, _models(_model(), _model(packed=False)), env) == _lib.SX_ERR_ARG
    odd = _model()
    odd.n_pad = 20                     # not a multiple of 16 / no room for the mean and Jacobian rows
    assert _call(entry, _models(_model(), odd), env) == _lib.SX_ERR_ARG
    # n_pad > 1024: no form (no workspace path), answered before any launch
    assert _call(entry, _models(_model(), _model(n_train=1100)), env) == _lib.SX_ERR_UNSUPPORTED
    # n_s = 1 has no output-by-output form: past the all-outputs form (here: 600 steps of actions beside Kstar) there is none
    assert _call(entry, _models(_model(1, 1), _model(1, 1, n_train=1000)), _env(1, 1, VAR), n_perf=600) \
        == _lib.SX_ERR_UNSUPPORTED


def test_table_entries_check_their_arguments():
    lib = _lib.lib()
    assert lib.sx_cem_perf_table_bytes(2, 1, 3) > 0 and lib.sx_cem_perf_table_bytes(2, 1, 3) % 3 == 0
    assert lib.sx_cem_perf_table_bytes(2, 1, 6) == 2 * lib.sx_cem_perf_table_bytes(2, 1, 3)
    for args in ((2, 1, 0), (0, 1, 3), (5, 1, 3), (2, 3, 3), (3, 2, 3)):      # (3, 2): no rollout kernel
        assert lib.sx_cem_perf_table_bytes(*args) < 0, args
    ms = _models(_model(), _model(n_train=70))
    alphas = (ctypes.c_void_p * 2)(16, 16)
    table = ctypes.c_void_p(16)
    assert lib.sx_cem_perf_table(None, alphas, 2, table, None) == _lib.SX_ERR_ARG
    assert lib.sx_cem_perf_table(ms, None, 2, table, None) == _lib.SX_ERR_ARG
    assert lib.sx_cem_perf_table(ms, alphas, 2, None, None) == _lib.SX_ERR_ARG
    assert lib.sx_cem_perf_table(ms, alphas, 0, table, None) == _lib.SX_ERR_ARG
    assert lib.sx_cem_perf_table(ms, (ctypes.c_void_p * 2)(16, None), 2, table, None) == _lib.SX_ERR_ARG
    assert lib.sx_cem_perf_table(_models(_model(), _model(2, 2)), alphas, 2, table, None) == _lib.SX_ERR_ARG
    assert lib.sx_cem_perf_table(_models(_model(3, 2), _model(3, 2)), alphas, 2, table, None) == _lib.SX_ERR_UNSUPPORTED


def test_form_queries_without_a_gpu():
    lib = _lib.lib()
    one = lambda m, n_perf=15: int(lib.sx_cem_perf_rollout_var_form(ctypes.byref(m), n_perf))
    multi = lambda ms, n_perf=15: int(lib.sx_cem_perf_rollout_var_multi_form(_models(*ms), len(ms), n_perf))
    small, mid, big = _model(n_train=7), _model(n_train=200), _model(n_train=590)
    assert one(small) == one(mid) == SX_FORM_STREAM and one(big) == SX_FORM_BYOUT
    assert multi([small, mid]) == SX_FORM_STREAM
    assert multi([small, mid, big]) == SX_FORM_BYOUT          # output by output for all where one model needs it
    # < 0: bad arguments, and wherever the entry answers SX_ERR_UNSUPPORTED
    assert lib.sx_cem_perf_rollout_var_form(None, 15) < 0 and lib.sx_cem_perf_rollout_var_multi_form(None, 2, 15) < 0
    assert one(small, n_perf=1) < 0 and multi([small, mid], n_perf=1) < 0
    assert int(lib.sx_cem_perf_rollout_var_multi_form(_models(small, mid), 0, 15)) < 0
    assert one(_model(packed=False)) < 0 and multi([small, _model(packed=False)]) < 0
    assert multi([small, _model(2, 2)]) < 0
    assert one(_model(n_train=1100)) < 0 and multi([small, _model(n_train=1100)]) < 0
    assert one(_model(3, 2)) < 0 and multi([_model(3, 2)]) < 0
    # n_s = 1 past the all-outputs form (600 steps of actions beside Kstar); the same model has a form for 40 steps
    assert one(_model(1, 1, n_train=1000), 40) == SX_FORM_STREAM and one(_model(1, 1, n_train=1000), 600) < 0
    assert multi([_model(1, 1), _model(1, 1, n_train=1000)], 600) < 0 and multi([_model(1, 1), _model(1, 1)], 600) >= 0


# ---- the solve with fakes in place of the launches -----------------------------------------------------------------------
class _Ssm:
    """An exact GP as far as the host-side plan reads it (never launched: the library is a fake)."""
    num_states, num_actions, kernel_family = 2, 1, 'rbf'

    def __init__(self, n_train=20, family='rbf'):
        self.kernel_family = family
        self.device_model = _model(n_train=n_train)
        self._alpha = torch.zeros((2, n_train), dtype=torch.float64)


class FakeLib:
    """The loaded library with every entry counted; the host-only queries answer for real, every entry that would touch
    the device answers SX_OK and records the row length it was handed."""
    HOST_ONLY = ('_bytes', '_form')

    def __init__(self, lib):
        self._lib = lib
        self.calls = collections.Counter()
        self.args = collections.defaultdict(list)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            self.args[name].append(args)
            return fn(*args) if name.endswith(self.HOST_ONLY) else _lib.SX_OK
        return counted


def _fake_device(monkeypatch, k, seen):
    fake = FakeLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: fake)
    monkeypatch.setattr(_lib, 'require_gpu', lambda *a: None)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda dev: None)

    def rank(con, obj, actions, kk, want_rows=False, want_refit=True):
        E, L = con.size(0), actions[0, 0].numel()
        seen.append(('rank', tuple(actions.shape), want_rows, want_refit))
        full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64)
        return dict(elite_rows=None, mean=full(1, E, L), std=full(2, E, L),
                    best=torch.arange(E * L, dtype=torch.float64).view(E, L), best_ok=torch.ones(E, dtype=torch.int32))

    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)
    return fake


@pytest.mark.parametrize('variance', [False, True])
def test_every_iteration_is_one_safety_launch_one_performance_launch_and_one_ranking(monkeypatch, variance):
    from safe_exploration_amd.cem_mpc import MultiModelPerfCemMpc
    seen = []
    fake = _fake_device(monkeypatch, 8, seen)
    E, P, H, iters, n_perf, r = 3, 64, 5, 4, 9, 2
    T = n_perf - r
    env = _env(obj_mode=VAR if variance else ABS)
    mpc = MultiModelPerfCemMpc([_Ssm(7), _Ssm(200), _Ssm(590)], env, H, P, 8, iters, device='cpu', init_std=0.2,
                               n_perf=n_perf, perf_r=r, perf_variance=variance)
    assert mpc.fused_applies()
    noise = torch.randn((iters, E, P, H + T, 1), dtype=torch.float64)
    fake.calls.clear()
    best, ok, status = mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=noise)
    assert tuple(best.shape) == (E, H + T, 1) and tuple(status.shape) == (E,)
    perf = 'sx_cem_perf_rollout_var_multi' if variance else 'sx_cem_perf_rollout_multi'
    other = 'sx_cem_perf_rollout_multi' if variance else 'sx_cem_perf_rollout_var_multi'
    assert fake.calls['sx_cem_rollout_multi'] == iters and fake.calls[perf] == iters and fake.calls[other] == 0
    assert fake.calls['sx_cem_rollout_elites_multi'] == 0            # no prologue refit: the ranking refits the long rows
    assert fake.calls['sx_cem_perf_rollout'] == fake.calls['sx_cem_perf_rollout_var'] == fake.calls['sx_cem_rollout'] == 0
    # the tables are built once per model change, not per launch: the mean-only form has one of its own
    assert fake.calls['sx_gp_model_table'] == 1
    assert fake.calls['sx_cem_perf_table'] == (0 if variance else 1)
    for args in fake.args[perf]:                                    # (models, table, env, E, P, H, n_perf, r, ...)
        assert args[3:8] == (E, P, H, n_perf, r)
    for args in fake.args['sx_cem_rollout_multi']:                  # the safety rollout runs over the first H steps
        assert args[3:6] == (E, P, H)
    assert seen == [('rank', (E, P, H + T, 1), False, True)] * iters
    # a second solve builds no table
    mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=noise)
    assert fake.calls['sx_gp_model_table'] == 1 and fake.calls['sx_cem_perf_table'] == (0 if variance else 1)
    # ... until a model changes
    mpc._ssms[1]._alpha = torch.zeros((2, 200), dtype=torch.float64)
    mpc._ssms[1].device_model = _model(n_train=200)
    mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=noise)
    assert fake.calls['sx_gp_model_table'] == 2 and fake.calls['sx_cem_perf_table'] == (0 if variance else 2)


def test_problem_e_draws_from_its_own_solver(monkeypatch):
    from safe_exploration_amd.cem_mpc import MultiModelPerfCemMpc
    _fake_device(monkeypatch, 8, [])
    E, P, H, iters, n_perf = 3, 16, 4, 2, 6
    solvers = [FusedCemMpc(_Ssm(20 + e), _env(), H, P, 8, iters, device='cpu', init_std=0.2, seed=e, n_perf=n_perf)
               for e in range(E)]
    mpc = MultiModelPerfCemMpc.from_solvers(solvers)
    twins = [FusedCemMpc(_Ssm(20 + e), _env(), H, P, 8, iters, device='cpu', init_std=0.2, seed=e, n_perf=n_perf)
             for e in range(E)]
    mpc.solve(torch.zeros((E, 2), dtype=torch.float64))
    assert tuple(mpc._last_noise.shape) == (iters, E, P, H + n_perf - 1, 1)          # row length
    for e, twin in enumerate(twins):
        assert torch.equal(mpc._last_noise[:, e], twin._next_noise(1)[:, 0])


def test_the_refusals():
    from safe_exploration_amd.cem_mpc import MultiModelPerfCemMpc
    mk = lambda **kw: FusedCemMpc(_Ssm(), _env(), 5, 64, 8, 3, device='cpu', **kw)
    # the base class keeps its refusal, and points to this one
    with pytest.raises(NotImplementedError, match='performance trajectory.*MultiModelPerfCemMpc'):
        MultiModelCemMpc.from_solvers([mk(n_perf=6), mk(n_perf=6)])
    for a, b in ((dict(n_perf=6), dict(n_perf=7)), (dict(n_perf=6, perf_r=1), dict(n_perf=6, perf_r=2)),
                 (dict(n_perf=6), dict(n_perf=6, perf_variance=True)), (dict(n_perf=6), dict())):
        with pytest.raises(ValueError, match='n_perf, perf_r'):
            MultiModelPerfCemMpc.from_solvers([mk(**a), mk(**b)])
    with pytest.raises(ValueError, match='n_perf > 0'):
        MultiModelPerfCemMpc.from_solvers([mk(), mk()])
    with pytest.raises(ValueError, match='n_perf > 0'):
        MultiModelPerfCemMpc([_Ssm(), _Ssm()], _env(), 5, 64, 8, 3, device='cpu')
    with pytest.raises(NotImplementedError, match='process group'):
        MultiModelPerfCemMpc([_Ssm(), _Ssm()], _env(), 5, 64, 8, 3, device='cpu', n_perf=6, process_group=object())
    hooked = mk(n_perf=6)
    hooked.set_env(_env(), objective_hook=lambda p: p[:, 0])
    with pytest.raises(NotImplementedError, match='objective hook'):
        MultiModelPerfCemMpc.from_solvers([mk(n_perf=6), hooked])
    mpc = MultiModelPerfCemMpc.from_solvers([mk(n_perf=6), mk(n_perf=6)])
    with pytest.raises(NotImplementedError, match='objective hook'):
        mpc.set_env(_env(), objective_hook=lambda p: p[:, 0])
    # the variance objective without perf_variance stays refused, by the solvers
    with pytest.raises(ValueError, match='variance objective'):
        MultiModelPerfCemMpc([_Ssm(), _Ssm()], _env(obj_mode=VAR), 5, 64, 8, 3, device='cpu', n_perf=6)
    # check_solvers compares the three settings
    for a, b in ((dict(n_perf=6), dict(n_perf=7)), (dict(n_perf=6, perf_r=1), dict(n_perf=6, perf_r=2)),
                 (dict(n_perf=6), dict(n_perf=6, perf_variance=True))):
        with pytest.raises(ValueError, match='CEM settings'):
            MultiModelCemMpc.check_solvers([mk(**a), mk(**b)])
    MultiModelCemMpc.check_solvers([mk(n_perf=6, perf_variance=True), mk(n_perf=6, perf_variance=True)])


def test_no_form_for_a_model_means_one_solve_per_model(monkeypatch):
    from safe_exploration_amd.cem_mpc import MultiModelPerfCemMpc
    _fake_device(monkeypatch, 8, [])
    mk = lambda n: FusedCemMpc(_Ssm(n), _env(1, 1, VAR), 5, 16, 4, 2, device='cpu', n_perf=600, perf_variance=True)
    # (n_s = 1 past the all-outputs form: the safety rollout of H = 5 steps still has a form, the 600 performance steps none)
    ok, none = _model(1, 1, n_train=20), _model(1, 1, n_train=1000)
    assert int(_lib.lib().sx_cem_rollout_multi_form(_models(ok, none), 2, 5)) >= 0
    solvers = [mk(20), mk(1000)]
    for s, m in zip(solvers, (ok, none)):
        s._ssm.num_states = 1
        s._ssm.device_model = m
    mpc = MultiModelPerfCemMpc.from_solvers(solvers)
    assert not mpc.fused_applies()
    for s in solvers:
        s._solve_checked = mock.Mock(return_value=(torch.zeros((1, 5, 1), dtype=torch.float64), torch.ones(1, dtype=torch.bool),
                                                   []))
    best, found = mpc.get_actions_multi(torch.zeros((2, 2), dtype=torch.float64))
    assert mpc.per_model_solves == 1 and all(s._solve_checked.call_count == 1 for s in solvers)
    assert tuple(best.shape) == (2, 5, 1)


# ---- get_actions_multi over CemSafeMPCs -------------------------------------------------------------------------------------
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


def _safempc(c, objective_target=-0.1, mpc=None):
    spec = problems.pendulum(n_train=8, obj_mode=ABS)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=objective_target)
    ssm = mock.Mock()
    ssm.kernel_family = 'rbf'
    return CemSafeMPC(ssm, [], env, c, {'lin_model': (spec.a, spec.b)}, wx_feedback_cost=None, wu_feedback_cost=None,
                      lqr=mock.Mock(), mpc=mpc, beta_safety=2.0, safe_policy=lambda x: spec.k_fb @ x)


@pytest.mark.parametrize('variance', [False, True])
def test_get_actions_multi_reaches_the_multi_model_solve_and_keeps_every_tail(monkeypatch, variance):
    from safe_exploration_amd.cem_mpc import MultiModelPerfCemMpc
    seen = []
    fake = _fake_device(monkeypatch, 8, seen)
    # the hand-off of the checked solve: the best rows as they are, every problem feasible
    monkeypatch.setattr(cem_mpc, '_check_solve', lambda owner, x0, q, best, ok, status, where, problems_:
                        (best.clone(), torch.ones(best.size(0), dtype=torch.bool), False))
    E, H, n_perf, r = 3, Conf.mpc_time_horizon, 7, 2
    T = n_perf - r
    env = _env(obj_mode=VAR if variance else ABS)
    kw = dict(cem_n_perf=n_perf, cem_perf_r=r, **({'cem_perf_variance': True} if variance else {}))
    target = None if variance else -0.1
    mpcs = [FusedCemMpc(_Ssm(20 + 50 * e), env, H, 64, 8, 3, device='cpu', init_std=0.2, seed=e, n_perf=n_perf, perf_r=r,
                        perf_variance=variance) for e in range(E)]
    solvers = [_safempc(conf(**kw), objective_target=target, mpc=m) for m in mpcs]
    actions, results = get_actions_multi(solvers, np.zeros((E, 2)))
    assert actions.shape == (E, 1) and len(results) == E
    multi = solvers[0]._multi[1]
    assert isinstance(multi, MultiModelPerfCemMpc) and multi.per_model_solves == 0
    perf = 'sx_cem_perf_rollout_var_multi' if variance else 'sx_cem_perf_rollout_multi'
    assert fake.calls['sx_cem_rollout_multi'] == fake.calls[perf] == 3 and len(seen) == 3
    # the plan is the H safety actions of the best row (the fake ranking's row e counts from e (H + T)); the tail stays
    L = H + T
    for e, (s, m) in enumerate(zip(solvers, mpcs)):
        assert s._batch_last_actions[0].shape == (H, 1)
        assert np.array_equal(s._batch_last_actions[0][:, 0], np.arange(e * L, e * L + H))
        assert tuple(m.last_perf_actions.shape) == (1, T, 1)
        assert np.array_equal(m.last_perf_actions[0, :, 0].numpy(), np.arange(e * L + H, (e + 1) * L))
    # the solve is cached like the one without a performance trajectory
    get_actions_multi(solvers, np.zeros((E, 2)))
    assert solvers[0]._multi[1] is multi


def test_get_actions_multi_refuses_mixed_and_disagreeing_lists():
    mk = lambda **kw: _safempc(conf(**kw), objective_target=None if kw.get('cem_perf_variance') else -0.1)
    with pytest.raises(NotImplementedError, match='cem_n_perf'):
        get_actions_multi([mk(cem_n_perf=6), mk()], np.zeros((2, 2)))
    with pytest.raises(NotImplementedError, match='cem_n_perf'):
        get_actions_multi([mk(), mk(cem_n_perf=6, cem_perf_variance=True)], np.zeros((2, 2)))
    with pytest.raises(ValueError, match='cem_perf_r'):
        get_actions_multi([mk(cem_n_perf=6, cem_perf_r=1), mk(cem_n_perf=6, cem_perf_r=2)], np.zeros((2, 2)))
    with pytest.raises(ValueError, match='cem_perf_variance'):
        get_actions_multi([mk(cem_n_perf=6), mk(cem_n_perf=6, cem_perf_variance=True)], np.zeros((2, 2)))
    with pytest.raises(ValueError, match='cem_n_perf'):
        get_actions_multi([mk(cem_n_perf=6), mk(cem_n_perf=7)], np.zeros((2, 2)))


def test_find_max_variance_multi_wraps_get_actions_multi(monkeypatch):
    from safe_exploration_amd import safempc_cem, safempc_exploration
    calls = []

    def fake(solvers, states):
        calls.append((list(solvers), states))
        return np.arange(3.0)[:, None], ['r0', 'r1', 'r2']

    monkeypatch.setattr(safempc_cem, 'get_actions_multi', fake)
    explorations = [mock.Mock(safempc=object()) for _ in range(3)]
    x0 = np.arange(6.0).reshape(3, 2)
    x, u, results = safempc_exploration.find_max_variance_multi(explorations, x0)
    assert calls[0][0] == [e.safempc for e in explorations] and np.array_equal(calls[0][1], x0)
    assert np.array_equal(x, x0) and u.shape == (3, 1) and results == ['r0', 'r1', 'r2']
