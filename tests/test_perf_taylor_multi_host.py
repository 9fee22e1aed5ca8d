"""CPU: Taylor uncertainty propagation in multi-model CEM solves, host side -- sx_cem_perf_rollout_taylor_multi and its form
query are declared and exported, refuse their arguments before any device access, and the form query answers by the rule of
the single-model query over all models; a MultiModelPerfCemMpc solve with perf_type='taylor' makes one safety launch, one
Taylor performance launch and one ranking per iteration (fakes in place of the launches), and goes one model at a time
where a model has no form; solves without the setting issue the entries they issued before."""
import ctypes
import os
import re
from unittest import mock

import pytest
import torch

from safe_exploration_amd import _lib, cem_mpc
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelPerfCemMpc
from test_perf_multi_host import ABS, SX_FORM_BYOUT, SX_FORM_STREAM, VAR, FakeLib, _env, _fake_device, _model, _models, _Ssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, FORM = 'sx_cem_perf_rollout_taylor_multi', 'sx_cem_perf_rollout_taylor_multi_form'


# ---- 1: the entries ---------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name in (NAME, FORM):
        assert re.search(r'\bint ' + name + r'\(', header)
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    restype, argtypes = _lib.SIGNATURES[NAME]
    # (models, table, env, E, P, H, n_perf, r, 11 buffers, terminal_safety, status, stream)
    assert restype is ctypes.c_int and len(argtypes) == 22
    assert argtypes[1] is ctypes.c_void_p and argtypes[3:8] == [ctypes.c_int] * 5
    assert argtypes[8:19] == [ctypes.c_void_p] * 11 and argtypes[19] is ctypes.c_int
    assert argtypes[20:] == [ctypes.c_void_p] * 2
    assert _lib.SIGNATURES[FORM][1][1:] == [ctypes.c_int, ctypes.c_int]
    assert callable(cem_mpc.cem_perf_rollout_taylor_multi)


# ---- 2: the argument checks -------------------------------------------------------------------------------------------------
def _call(models, env, *, E=2, P=4, H=5, n_perf=8, r=1, table=16, x0=16, safe=16, mean=16, std=16, noise=16, rows=16, obj=16,
          con=16, status=16, terminal=0):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return _lib.lib().sx_cem_perf_rollout_taylor_multi(models, p(table), None if env is None else ctypes.byref(env), E, P, H,
                                                       n_perf, r, p(x0), p(safe), p(mean), p(std), p(noise), p(rows), p(obj),
                                                       p(con), None, None, None, terminal, p(status), None)


@pytest.mark.parametrize('obj_mode', [VAR, ABS])
def test_argument_errors_without_a_gpu(obj_mode):
    """Every pointer below is the fake 16: an entry that touched the device with one of these calls would not come back."""
    ms, env = _models(_model(n_train=20), _model(n_train=70)), _env(obj_mode=obj_mode)
    # what sx_cem_perf_rollout_var_multi refuses ...
    for kw in (dict(table=None), dict(x0=None), dict(safe=None), dict(rows=None), dict(obj=None), dict(con=None),
               dict(status=None), dict(mean=None), dict(std=None), dict(E=0), dict(P=0), dict(H=0), dict(r=0), dict(r=6),
               dict(n_perf=1), dict(n_perf=3, r=3),
               # ... and what sx_cem_perf_rollout_taylor refuses: the checked state H + 2 lies past the trajectory
               dict(terminal=1, n_perf=6), dict(terminal=1, n_perf=5, r=2)):
        assert _call(ms, env, **kw) == _lib.SX_ERR_ARG, kw
    assert _call(None, env) == _lib.SX_ERR_ARG and _call(ms, None) == _lib.SX_ERR_ARG
    assert _call(_models(_model(), _model(n_train=0)), env) == _lib.SX_ERR_ARG
    assert _call(_models(_model(), _model(2, 2)), env) == _lib.SX_ERR_ARG       # the models disagree on the shape
    assert _call(_models(_model(2, 2), _model(2, 2)), env) == _lib.SX_ERR_ARG   # models and env disagree
    assert _call(_models(_model(), _model(packed=False)), env) == _lib.SX_ERR_ARG
    for field in ('x_train', 'a_pack', 'stage_tab'):
        bad = _model()
        setattr(bad, field, None)
        assert _call(_models(_model(), bad), env) == _lib.SX_ERR_ARG, field
    odd = _model()
    odd.n_pad = 20                     # not a multiple of 16 / no room for the mean and Jacobian rows
    assert _call(_models(_model(), odd), env) == _lib.SX_ERR_ARG
    assert _call(ms, _env(obj_mode=7)) == _lib.SX_ERR_ARG
    no_rows = _env(obj_mode=obj_mode)
    no_rows.m = 0
    assert _call(ms, no_rows, terminal=1, n_perf=7) == _lib.SX_ERR_ARG          # nothing to check against
    negative = _env(obj_mode=obj_mode)
    negative.m = -1
    assert _call(ms, negative) == _lib.SX_ERR_ARG
    # SX_ERR_UNSUPPORTED, before any launch: more polytope rows than the step constants hold, with and without the flag
    many = _env(obj_mode=obj_mode)
    many.m = 17
    assert _call(ms, many) == _lib.SX_ERR_UNSUPPORTED and _call(ms, many, terminal=1) == _lib.SX_ERR_UNSUPPORTED
    # a model with n_pad > 1024 among the E has no form (no workspace path)
    big = _model(n_train=1100)
    assert big.n_pad > 1024
    for models in (_models(_model(), big), _models(big, _model())):
        assert _call(models, env) == _lib.SX_ERR_UNSUPPORTED
        assert _call(models, env, terminal=1) == _lib.SX_ERR_UNSUPPORTED
    # a shape without a rollout kernel; one output has no output-by-output form
    assert _call(_models(_model(3, 2), _model(3, 2)), _env(3, 2, obj_mode)) == _lib.SX_ERR_UNSUPPORTED
    assert _call(_models(_model(1, 1), _model(1, 1, n_train=1000)), _env(1, 1, obj_mode), n_perf=600) \
        == _lib.SX_ERR_UNSUPPORTED


# ---- 3: the form query ------------------------------------------------------------------------------------------------------
def _one(name, m, n_perf):
    return int(getattr(_lib.lib(), name)(ctypes.byref(m), n_perf))


def _multi(name, ms, n_perf):
    return int(getattr(_lib.lib(), name)(_models(*ms), len(ms), n_perf))


def _rule(own):
    return -1 if any(f < 0 for f in own) else SX_FORM_BYOUT if any(f == SX_FORM_BYOUT for f in own) else SX_FORM_STREAM


@pytest.mark.parametrize('n_perf', [2, 30])
@pytest.mark.parametrize('n_s,n_u', [(2, 1), (4, 2)])
def test_the_multi_form_is_the_single_model_forms_combined(n_s, n_u, n_perf):
    """Every N from 7 to 1100 in pairs and triples with other sizes: the multi-model answer is -1 iff a model's own answer
    is -1, else output by output iff a model's own answer is, else all outputs at once."""
    models = {N: _model(n_s, n_u, N) for N in range(7, 1101)}
    own = {N: _one('sx_cem_perf_rollout_taylor_form', m, n_perf) for N, m in models.items()}
    assert {SX_FORM_STREAM, SX_FORM_BYOUT, -1} == set(own.values())      # the sweep crosses both thresholds
    for N in range(7, 1101):
        others = (7, 1100 + 7 - N, 7 + (3 * N) % 1094)                   # a small one, the sweep mirrored, a scattered one
        for sizes in ((N,), (7, N), (N, others[1]), (others[2], N, others[1]), (N, N)):
            got = _multi(FORM, [models[s] for s in sizes], n_perf)
            assert got == _rule([own[s] for s in sizes]), (sizes, got, [own[s] for s in sizes])


def test_the_step_constants_tip_a_model_output_by_output_where_the_variance_form_keeps_all_outputs():
    """At (2, 1) with n_perf = 2, N = 525 .. 540 (one n_pad) fit the variance kernel's LDS with all outputs but not with
    the Taylor form's step constants behind the actions: the Taylor launch over (7, N) goes output by output, the variance
    launch over the same models does not.  Found by the sweep; the test searches again rather than trusting the figure."""
    n_perf, tipped = 2, []
    for N in range(7, 1101):
        m = _model(2, 1, N)
        if (_one('sx_cem_perf_rollout_taylor_form', m, n_perf) == SX_FORM_BYOUT
                and _one('sx_cem_perf_rollout_var_form', m, n_perf) == SX_FORM_STREAM):
            tipped.append(N)
    print(f'(2, 1), n_perf = {n_perf}: the step constants tip N = {tipped[:1]} .. {tipped[-1:]} ({len(tipped)} sizes)')
    assert tipped
    for N in tipped:
        ms = [_model(2, 1, 7), _model(2, 1, N)]
        assert _multi(FORM, ms, n_perf) == SX_FORM_BYOUT
        assert _multi('sx_cem_perf_rollout_var_multi_form', ms, n_perf) == SX_FORM_STREAM


def test_the_form_query_refuses_what_the_entry_refuses():
    small, mid = _model(n_train=7), _model(n_train=200)
    lib = _lib.lib()
    assert _multi(FORM, [small, mid], 8) == SX_FORM_STREAM and _multi(FORM, [small, mid, _model(n_train=590)], 8) == SX_FORM_BYOUT
    assert int(lib.sx_cem_perf_rollout_taylor_multi_form(None, 2, 8)) < 0
    assert int(lib.sx_cem_perf_rollout_taylor_multi_form(_models(small, mid), 0, 8)) < 0
    assert _multi(FORM, [small, mid], 1) < 0
    assert _multi(FORM, [small, _model(packed=False)], 8) < 0                  # unpacked models: as the variance query
    assert _multi(FORM, [small, _model(2, 2)], 8) < 0
    assert _multi(FORM, [_model(3, 2)], 8) < 0


# ---- 4: the solve with fakes in place of the launches ----------------------------------------------------------------------
class OrderedFakeLib(FakeLib):
    """FakeLib that also appends every entry that would touch the device to `order`, the list the fake ranking writes to."""

    def __init__(self, lib, order):
        super().__init__(lib)
        self.order = order

    def __getattr__(self, name):
        counted = super().__getattr__(name)

        def ordered(*args):
            if not name.endswith(self.HOST_ONLY):
                self.order.append(name)
            return counted(*args)
        return ordered


def _ordered_device(monkeypatch, order):
    _fake_device(monkeypatch, 8, order)                 # require_gpu, stream_ptr and the ranking, which appends ('rank', ...)
    fake = OrderedFakeLib(_lib.lib()._lib, order)
    monkeypatch.setattr(_lib, 'lib', lambda: fake)
    return fake


@pytest.mark.parametrize('safety', [False, True])
def test_every_iteration_is_one_safety_launch_one_taylor_launch_and_one_ranking(monkeypatch, safety):
    order = []
    fake = _ordered_device(monkeypatch, order)
    E, P, H, iters, n_perf, r = 3, 64, 5, 4, 9, 2
    T = n_perf - r
    mpc = MultiModelPerfCemMpc([_Ssm(7), _Ssm(200), _Ssm(590)], _env(obj_mode=VAR), H, P, 8, iters, device='cpu',
                               init_std=0.2, n_perf=n_perf, perf_r=r, perf_type='taylor', perf_terminal_safety=safety)
    assert all(s._perf.type == 'taylor' and s._perf.terminal_safety == safety for s in mpc.solvers)
    assert mpc.fused_applies() is True
    noise = torch.randn((iters, E, P, H + T, 1), dtype=torch.float64)
    fake.calls.clear()
    del order[:]
    best, ok, status = mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=noise)
    assert tuple(best.shape) == (E, H + T, 1) and tuple(status.shape) == (E,)
    rank = ('rank', (E, P, H + T, 1), False, True)                  # rows of H + T steps; the ranking refits
    assert order == ['sx_gp_model_table'] + ['sx_cem_rollout_multi', NAME, rank] * iters
    assert fake.calls['sx_cem_rollout_multi'] == iters and fake.calls[NAME] == iters
    for other in ('sx_cem_perf_rollout_taylor', 'sx_cem_perf_rollout_var_multi', 'sx_cem_perf_rollout_multi',
                  'sx_cem_perf_table', 'sx_cem_rollout_elites_multi', 'sx_cem_rollout'):
        assert fake.calls[other] == 0, other
    for args in fake.args[NAME]:         # (models, table, env, E, P, H, n_perf, r, 11 buffers, terminal_safety, status, stream)
        assert len(args) == 22 and args[3:8] == (E, P, H, n_perf, r) and args[19] == int(safety)
        assert args[16] is None and args[17] is None and args[18] is None       # a solve records no trajectories
    for args in fake.args['sx_cem_rollout_multi']:                  # the safety rollout runs over the first H steps
        assert args[3:6] == (E, P, H)
    # the safety launch and the Taylor launch read one device table, built once
    table = lambda name: {getattr(a[1], 'value', a[1]) for a in fake.args[name]}
    assert table(NAME) == table('sx_cem_rollout_multi') and len(table(NAME)) == 1 and None not in table(NAME)
    mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=noise)
    assert fake.calls['sx_gp_model_table'] == 1
    # get_actions_multi takes the same road: no solve goes one model at a time
    for s in mpc.solvers:
        s._solve_checked = mock.Mock(side_effect=AssertionError('a per-model solve'))
    monkeypatch.setattr(cem_mpc, '_check_solve', lambda owner, x0, q, best, ok, status, where, problems_:
                        (best.clone(), torch.ones(best.size(0), dtype=torch.bool), False))
    before = fake.calls[NAME]
    best, found = mpc.get_actions_multi(torch.zeros((E, 6), dtype=torch.float64))
    assert mpc.per_model_solves == 0 and fake.calls[NAME] == before + iters
    assert tuple(best.shape) == (E, H, 1) and all(tuple(s.last_perf_actions.shape) == (1, T, 1) for s in mpc.solvers)


def test_from_solvers_takes_the_settings_from_the_solvers(monkeypatch):
    order = []
    fake = _ordered_device(monkeypatch, order)
    mk = lambda n: FusedCemMpc(_Ssm(n), _env(obj_mode=VAR), 5, 16, 4, 2, device='cpu', n_perf=8, perf_type='taylor',
                               perf_terminal_safety=True)
    mpc = MultiModelPerfCemMpc.from_solvers([mk(20), mk(70)])
    assert mpc.fused_applies() is True
    mpc.solve(torch.zeros((2, 2), dtype=torch.float64))
    assert fake.calls[NAME] == 2 and all(a[19] == 1 and a[3:8] == (2, 16, 5, 8, 1) for a in fake.args[NAME])


def test_a_model_without_a_form_means_one_solve_per_model(monkeypatch):
    order = []
    fake = _ordered_device(monkeypatch, order)
    H = 5
    solvers = [FusedCemMpc(_Ssm(n), _env(obj_mode=VAR), H, 16, 4, 2, device='cpu', n_perf=8, perf_type='taylor')
               for n in (20, 1100)]
    assert solvers[1]._ssm.device_model.n_pad > 1024
    mpc = MultiModelPerfCemMpc.from_solvers(solvers)
    assert mpc.fused_applies() is False
    with pytest.raises(cem_mpc.FusedMultiUnsupported, match='taylor'):
        mpc.solve(torch.zeros((2, 2), dtype=torch.float64))
    for s in solvers:
        s._solve_checked = mock.Mock(return_value=(torch.zeros((1, H, 1), dtype=torch.float64),
                                                   torch.ones(1, dtype=torch.bool), []))
    best, found = mpc.get_actions_multi(torch.zeros((2, 6), dtype=torch.float64))
    assert mpc.per_model_solves == 1 and all(s._solve_checked.call_count == 1 for s in solvers)
    assert tuple(best.shape) == (2, H, 1) and fake.calls[NAME] == 0 and fake.calls['sx_cem_rollout_multi'] == 0


def test_the_wrapper_checks_what_it_can_before_the_library(monkeypatch):
    order = []
    fake = _ordered_device(monkeypatch, order)
    ssms, env = [_Ssm(7), _Ssm(70)], _env(obj_mode=VAR)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    kw = dict(safe_actions=z(2, 4, 5, 1), obj_cost=z(2, 4), con_cost=z(2, 4), tail_mean=z(2, 5, 1), tail_std=z(2, 5, 1),
              tail_noise=z(2, 4, 5, 1))
    with pytest.raises(ValueError, match='one word per problem'):
        cem_mpc.cem_perf_rollout_taylor_multi(ssms, env, z(2, 2), 5, 6, 1, status=torch.zeros(1, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match='2 models for 3 problems'):
        cem_mpc.cem_perf_rollout_taylor_multi(ssms, env, z(3, 2), 5, 6, 1, status=torch.zeros(3, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match='n_perf'):
        cem_mpc.cem_perf_rollout_taylor_multi(ssms, env, z(2, 2), 5, 6, 1, status=torch.zeros(2, dtype=torch.int32),
                                              terminal_safety=True, **kw)
    assert fake.calls[NAME] == 0
    out = cem_mpc.cem_perf_rollout_taylor_multi(ssms, env, z(2, 2), 5, 6, 1, status=torch.zeros(2, dtype=torch.int32),
                                                want_traj=True, want_sigma=True, want_cov=True, **kw)
    assert tuple(out['rows'].shape) == (2, 4, 10, 1) and tuple(out['perf_cov'].shape) == (2, 4, 6, 2, 2)
    assert tuple(out['perf_sigma'].shape) == tuple(out['perf_traj'].shape) == (2, 4, 6, 2)
    # SX_ERR_UNSUPPORTED from the entry is FusedMultiUnsupported
    class Refusing(OrderedFakeLib):
        def __getattr__(self, name):
            return (lambda *args: _lib.SX_ERR_UNSUPPORTED) if name == NAME else super().__getattr__(name)

    refusing = Refusing(fake._lib, order)
    monkeypatch.setattr(_lib, 'lib', lambda: refusing)
    with pytest.raises(cem_mpc.FusedMultiUnsupported, match='taylor'):
        cem_mpc.cem_perf_rollout_taylor_multi(ssms, env, z(2, 2), 5, 6, 1, status=torch.zeros(2, dtype=torch.int32), **kw)


# ---- 5: without the setting -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variance', [False, True])
def test_without_the_setting_a_multi_model_solve_issues_what_it_issued(monkeypatch, variance):
    """The ordered list of everything that would touch the device, against the list of the solve before the Taylor form
    had a multi-model launch: the tables once, then per iteration the safety launch, the performance launch of the
    setting and the ranking."""
    order = []
    fake = _ordered_device(monkeypatch, order)
    E, P, H, iters, n_perf, r = 3, 64, 5, 4, 9, 2
    T = n_perf - r
    mpc = MultiModelPerfCemMpc([_Ssm(7), _Ssm(200), _Ssm(590)], _env(obj_mode=VAR if variance else ABS), H, P, 8, iters,
                               device='cpu', init_std=0.2, n_perf=n_perf, perf_r=r, perf_variance=variance)
    assert mpc.fused_applies()
    del order[:]
    fake.calls.clear()
    mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=torch.randn((iters, E, P, H + T, 1), dtype=torch.float64))
    rank = ('rank', (E, P, H + T, 1), False, True)
    perf = 'sx_cem_perf_rollout_var_multi' if variance else 'sx_cem_perf_rollout_multi'
    first = ['sx_gp_model_table', 'sx_cem_rollout_multi'] + ([] if variance else ['sx_cem_perf_table']) + [perf, rank]
    assert order == first + ['sx_cem_rollout_multi', perf, rank] * (iters - 1)
    assert not any('taylor' in name for name in fake.calls), sorted(fake.calls)
    assert len(fake.args[perf][0]) == (20 if variance else 19)               # the entries' own argument lists
