"""CPU-side checks of the SafeMPC constraint set in multi-model CEM solves ("the multi-model form"):
the declarations of sx_cem_rollout_cons_multi, sx_cem_rollout_elites_cons_multi and sx_cem_rollout_cons_multi_form, their
argument errors without a GPU and in their order, the form query, the plumbing of MultiModelConsCemMpc over a fake library,
the refusals, get_actions_multi over CemSafeMPCs with the two conf settings, and the conditions on the inputs of the GPU
solve test (tests/conset_multi_oracle.py)."""
import ctypes
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

import conset_multi_oracle as cmo
import conset_oracle as co
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc, MultiModelConsCemMpc
from safe_exploration_amd.gp_reachability_pytorch import make_con_set
from safe_exploration_amd.safempc_cem import get_actions_multi
from test_conset_host import (_bad_sets, _fake, _plan_model, _rollout_entries, _safempc_with, _set, _shift0_shapes)
from test_perf_multi_host import _env, _model, _models, _safempc, _Ssm, conf
from test_sat_cost_host import COST2, _bad_costs, _cost, _hook, p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
ENTRIES = {'sx_cem_rollout_cons_multi': 'sx_cem_rollout_multi', 'sx_cem_rollout_elites_cons_multi': 'sx_cem_rollout_elites_multi'}


# ---- declarations --------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_with_the_parents_arguments_plus_the_set_and_the_cost():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name, parent in ENTRIES.items():
        assert re.search(r'\bint ' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        ours, theirs = _lib.SIGNATURES[name][1], _lib.SIGNATURES[parent][1]
        assert len(ours) == len(theirs) + 2
        assert ours[:3] == theirs[:3] and ours[3] == ctypes.POINTER(_lib.SxConSet) and ours[4] == ctypes.POINTER(_lib.SxSatCost)
        assert ours[5:] == theirs[3:]
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        assert len(decl.split(',')) == len(ours)
        assert re.search(r'const sx_env\* env, const sx_con_set\* cons,\s+const sx_sat_cost\* cost', decl)
    name = 'sx_cem_rollout_cons_multi_form'
    assert re.search(r'\bint ' + name + r'\(', header) and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES['sx_cem_rollout_multi_form']


def test_both_translation_units_are_built():
    text = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'build.sh')).read()
    for src in ('sx_stream_cons_multi.hip', 'sx_stream_cons_sat_multi.hip'):
        assert src in text and os.path.exists(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', src))


# ---- argument errors, before any device access ---------------------------------------------------------------------------------------
def _call(cons, cost=None, *, elites=False, models='ok', table=16, env=None, E=2, P=4, H=5, x0=16, mean=16, std=16, noise=16,
          actions=16, obj=16, con=16, status=16, rows=16, k=3, mean_out=None, std_out=None):
    env = env if env is not None else _env()
    models = _models(_model(n_train=20), _model(n_train=70)) if models == 'ok' else models
    head = (models, p(table), ctypes.byref(env), None if cons is None else ctypes.byref(cons),
            None if cost is None else ctypes.byref(cost))
    entry = 'sx_cem_rollout' + ('_elites' if elites else '') + '_cons_multi'
    dist = (p(rows), k) if elites else (p(mean), p(std))
    tail = (p(mean_out), p(std_out)) if elites else ()
    return getattr(_lib.lib(), entry)(*head, E, P, H, p(x0), None, *dist, p(noise), p(actions), None, None, p(obj), p(con),
                                      p(status), *tail, None)


@pytest.mark.parametrize('with_cost', [False, True])
@pytest.mark.parametrize('elites', [False, True])
def test_rollout_argument_errors_without_a_gpu(elites, with_cost):
    ok_cost = _cost() if with_cost else None
    call = lambda cons='ok', cost='ok', **kw: _call(_set() if cons == 'ok' else cons, ok_cost if cost == 'ok' else cost,
                                                    elites=elites, **kw)
    too_big = _models(_model(n_train=20), _model(n_train=1100))      # no streaming form: SX_ERR_UNSUPPORTED, after the checks
    assert call(models=too_big) == UNSUPPORTED
    # what sx_cem_rollout[_elites]_multi refuses: a NULL table, NULL models, differing shapes, models[0] not of env's shape
    assert call(table=None) == ARG and call(models=None) == ARG
    assert call(models=_models(_model(), _model(2, 2))) == ARG
    assert call(models=_models(_model(2, 2), _model(2, 2))) == ARG
    assert call(models=_models(_model(), _model(n_train=0))) == ARG
    for kw in (dict(x0=None), dict(actions=None), dict(obj=None), dict(con=None), dict(status=None), dict(E=0), dict(P=0),
               dict(H=0)):
        assert call(**kw) == ARG, kw
    if elites:
        for kw in (dict(rows=None), dict(noise=None), dict(k=0), dict(mean_out=16), dict(std_out=16)):
            assert call(**kw) == ARG, kw
    else:
        assert call(mean=None) == ARG and call(std=None) == ARG
    # the set: NULL or invalid
    assert call(None) == ARG
    for what, bad in _bad_sets():
        assert call(bad) == ARG, what
    # garbage in the rows NOT in use is not read
    unused = _set(m_obs=1)
    unused.h_mat_obs[2], unused.h_obs[1] = float('nan'), float('inf')
    assert call(unused, table=None) == ARG and call(unused, models=too_big) == UNSUPPORTED
    # a bad cost
    for what, bad in _bad_costs():
        assert call(cost=bad) == ARG, what
    # every check comes before the plan: a bad table, set or cost over models without a form is the argument's error
    assert call(table=None, models=too_big) == ARG
    assert call(_bad_sets()[0][1], models=too_big) == ARG
    if with_cost:
        assert call(cost=_cost(rank=0), models=too_big) == ARG
    # SX_ERR_UNSUPPORTED exactly where sx_cem_rollout_sat_multi answers it: m beyond SX_MAX_M, a shape without a kernel, the
    # workspace path (above), neither streaming form, the elite-row limit
    many = _env()
    many.m = _lib.SX_MAX_M + 1
    assert call(env=many) == UNSUPPORTED
    cost3 = _cost(3, 0, 1) if with_cost else None
    assert call(_set(3), cost3, models=_models(_model(3, 2), _model(3, 2)), env=_env(3, 2)) == UNSUPPORTED
    cost1 = _cost(1, 0, 1) if with_cost else None
    assert call(_set(1), cost1, models=_models(_model(1, 1), _model(1, 1, n_train=1000)), env=_env(1, 1), H=600) == UNSUPPORTED
    if elites:
        assert call(H=385) == UNSUPPORTED


def _sat_multi(elites, models, env, cost, **kw):
    """sx_cem_rollout[_elites]_sat_multi on the arguments of `_call`."""
    a = dict(E=2, P=4, H=5, rows=16, k=3)
    a.update(kw)
    entry = 'sx_cem_rollout' + ('_elites' if elites else '') + '_sat_multi'
    dist = (p(a['rows']), a['k']) if elites else (p(16), p(16))
    tail = (None, None) if elites else ()
    return getattr(_lib.lib(), entry)(models, p(16), ctypes.byref(env), ctypes.byref(cost), a['E'], a['P'], a['H'], p(16), None,
                                      *dist, p(16), p(16), None, None, p(16), p(16), p(16), *tail, None)


@pytest.mark.parametrize('elites', [False, True])
def test_unsupported_is_answered_exactly_where_the_sat_multi_entry_answers_it(elites):
    """(Only arguments that are refused: a call that is accepted would launch.)"""
    many = _env()
    many.m = _lib.SX_MAX_M + 1
    cases = [(_models(_model(n_train=20), _model(n_train=70)), many, 2, {}),
             (_models(_model(n_train=20), _model(n_train=1100)), _env(), 2, {}),
             (_models(_model(n_train=1100), _model(n_train=20)), _env(), 2, {}),
             (_models(_model(3, 2), _model(3, 2)), _env(3, 2), 3, {}),
             (_models(_model(1, 1), _model(1, 1, n_train=1000)), _env(1, 1), 1, dict(H=600))]
    if elites:
        cases.append((_models(_model(n_train=20), _model(n_train=70)), _env(), 2, dict(H=385)))
    for models, env, n_s, kw in cases:
        cost = _cost(n_s, 0, 1) if n_s != 2 else _cost()
        assert _sat_multi(elites, models, env, cost, **kw) == UNSUPPORTED, (n_s, kw)
        assert _call(_set(n_s), cost, elites=elites, models=models, env=env, **kw) == UNSUPPORTED, (n_s, kw)
        assert _call(_set(n_s), None, elites=elites, models=models, env=env, **kw) == UNSUPPORTED, (n_s, kw)


# ---- the form query --------------------------------------------------------------------------------------------------------------------
def test_the_form_query_is_the_multi_model_plan_on_the_compiled_shapes():
    lib = _lib.lib()
    form = lambda ms, H: int(lib.sx_cem_rollout_cons_multi_form(_models(*ms), len(ms), H))
    parent = lambda ms, H: int(lib.sx_cem_rollout_multi_form(_models(*ms), len(ms), H))
    compiled = _shift0_shapes()
    assert compiled == [(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2)]
    seen = set()
    for n_s, n_u in compiled:
        for H in (3, 15, 40):
            # the sizes on both sides of the output-by-output threshold of this shape and horizon
            single = [int(lib.sx_cem_rollout_cons_form(ctypes.byref(_plan_model(n_s, n_u, N)), H)) for N in range(1, 1100)]
            edges = [N + 1 for N in range(1, 1099) if single[N] != single[N - 1]]      # single[N - 1] is the form of N
            sizes = sorted({7, 200, 1000} | {N for edge in edges for N in (edge - 1, edge)})
            for N in sizes:
                for other in (7, N):
                    ms = [_plan_model(n_s, n_u, other), _plan_model(n_s, n_u, N)]
                    got = form(ms, H)
                    assert got == parent(ms, H), (n_s, n_u, H, other, N)
                    # the fold: no form where any model has none, output by output where any model needs it
                    alone = [single[other - 1], single[N - 1]]
                    want = -1 if min(alone) < 0 else SX_FORM_BYOUT if SX_FORM_BYOUT in alone else SX_FORM_STREAM
                    assert got == want, (n_s, n_u, H, other, N)
                    seen.add(got)
    assert seen == {SX_FORM_STREAM, SX_FORM_BYOUT, -1}
    # a mixed pair whose larger model forces the output-by-output form for the launch
    small, mid, big = _plan_model(4, 1, 33), _plan_model(4, 1, 200), _plan_model(4, 1, 590)
    assert form([small, mid], 3) == SX_FORM_STREAM and form([big, mid, small], 3) == form([small, big], 15) == SX_FORM_BYOUT
    # -1 where multi_models_ok fails, as sx_cem_rollout_multi_form
    for ms, E, H in ((None, 2, 5), (_models(small, mid), 0, 5), (_models(small, _plan_model(2, 1, 20)), 2, 5),
                     (_models(small, _plan_model(4, 1, 0)), 2, 5), (_models(small, mid), 2, 0),
                     (_models(_plan_model(3, 2, 20)), 1, 5)):
        assert int(lib.sx_cem_rollout_cons_multi_form(ms, E, H)) == int(lib.sx_cem_rollout_multi_form(ms, E, H)) == -1


# ---- the plumbing over a fake library ------------------------------------------------------------------------------------------------
def _solvers(sizes, H, P, iters, con_sets, with_cost=False, **kw):
    out = []
    for e, (n, cons) in enumerate(zip(sizes, con_sets)):
        ssm = _Ssm(n)
        ssm.workspace = lambda nbytes: None
        s = FusedCemMpc(ssm, _env(), H, P, 8, iters, device='cpu', init_std=0.2, seed=e, cost_on_safety=with_cost,
                        **({} if cons is None else dict(con_set=cons)), **kw)
        if with_cost:
            s.set_env(_env(), objective_hook=_hook)
            s.set_cost(COST2)
        out.append(s)
    return out


@pytest.mark.parametrize('with_cost', [False, True])
def test_a_multi_model_solve_with_a_set_reaches_the_cons_multi_entries_only(monkeypatch, with_cost):
    fake = _fake(monkeypatch)
    iters, P, H, E = 3, 4096, 4, 3     # (4096 candidates: the counting ranking, whose refit moves into the rollout's prologue)
    solvers = _solvers((7, 200, 590), H, P, iters, [_set()] * E, with_cost)
    mpc = MultiModelConsCemMpc.from_solvers(solvers)
    assert mpc.fused_applies() and solvers[0]._refit_in_prologue(E)
    assert fake.calls['sx_cem_rollout_cons_multi_form'] == 1 and fake.calls['sx_cem_rollout_multi_form'] == 0
    fake.calls.clear()
    best, ok, status = mpc.solve(torch.zeros((E, 2), dtype=torch.float64))
    assert tuple(best.shape) == (E, H, 1) and tuple(status.shape) == (E,)
    assert _rollout_entries(fake) == {'sx_cem_rollout_cons_multi': 1, 'sx_cem_rollout_elites_cons_multi': iters - 1}
    assert fake.calls['sx_gp_model_table'] == 1
    first = fake.args['sx_cem_rollout_cons_multi'][0]
    assert len(first) == 20 and first[5:8] == (E, P, H)
    assert [first[0][e].n_train for e in range(E)] == [7, 200, 590]
    got = ctypes.cast(first[3], ctypes.POINTER(_lib.SxConSet)).contents
    assert (got.m_obs, got.ctrl_ellipsoid) == (2, 1) and bytes(got) == bytes(_set())
    if with_cost:
        assert ctypes.cast(first[4], ctypes.POINTER(_lib.SxSatCost)).contents.rank == COST2.rank
    else:
        assert first[4] is None
    for args in fake.args['sx_cem_rollout_elites_cons_multi']:
        assert len(args) == 22 and args[5:8] == (E, P, H) and args[11] == 8
        assert bytes(ctypes.cast(args[3], ctypes.POINTER(_lib.SxConSet)).contents) == bytes(_set())
        assert (args[4] is None) == (not with_cost)
    # built from the models, as the parent class is
    fake.calls.clear()
    own = MultiModelConsCemMpc([_Ssm(7), _Ssm(200)], _env(), H, 64, 8, iters, device='cpu', init_std=0.2, con_set=_set())
    assert all(bytes(s._con_set) == bytes(_set()) for s in own.solvers)
    own.solve(torch.zeros((2, 2), dtype=torch.float64))
    assert set(_rollout_entries(fake)) <= set(ENTRIES) and sum(_rollout_entries(fake).values()) == iters
    # without a set the multi-model solve calls exactly what it called before
    fake.calls.clear()
    plain = MultiModelCemMpc.from_solvers(_solvers((7, 200, 590), H, P, iters, [None] * E, with_cost))
    plain.solve(torch.zeros((E, 2), dtype=torch.float64))
    sfx = '_sat_multi' if with_cost else '_multi'
    assert _rollout_entries(fake) == {'sx_cem_rollout' + sfx: 1, 'sx_cem_rollout_elites' + sfx: iters - 1}
    assert len(fake.args['sx_cem_rollout' + sfx][0]) == (19 if with_cost else 18)


def test_no_form_for_a_model_means_one_solve_per_model(monkeypatch):
    """A training set on the workspace path: the solvers, which carry the set, solve one model at a time."""
    _fake(monkeypatch)
    solvers = _solvers((20, 1100), 5, 64, 3, [_set()] * 2)
    mpc = MultiModelConsCemMpc.from_solvers(solvers)
    assert not mpc.fused_applies()
    for s in solvers:
        s._solve_checked = mock.Mock(return_value=(torch.zeros((1, 5, 1), dtype=torch.float64), torch.ones(1, dtype=torch.bool),
                                                   []))
    best, found = mpc.get_actions_multi(torch.zeros((2, 6), dtype=torch.float64))
    assert mpc.per_model_solves == 1 and all(s._solve_checked.call_count == 1 for s in solvers)
    assert tuple(best.shape) == (2, 5, 1)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_refusals(monkeypatch):
    _fake(monkeypatch)
    x0, noise = torch.zeros((2, 2), dtype=torch.float64), torch.zeros((2, 4, 3, 1), dtype=torch.float64)
    mean = torch.zeros((2, 3, 1), dtype=torch.float64)
    # the wrapper: the 'rbf' family only, with the message of the single-model wrapper, for every model
    for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
        for ssms in ([_Ssm(family=family)] * 2, [_Ssm(), _Ssm(family=family)]):
            with pytest.raises(NotImplementedError, match='con_set.*exact RBF GPs.*' + family):
                cem_mpc.cem_rollout_multi(ssms, _env(), x0, 3, mean=mean, std=mean, noise=noise, con_set=_set())
    with pytest.raises(TypeError, match='SxConSet'):
        cem_mpc.cem_rollout_multi([_Ssm(), _Ssm()], _env(), x0, 3, mean=mean, std=mean, noise=noise, con_set='set')
    # the new guard: the base class no longer builds a solve that silently drops the set
    with_set, without = _solvers((20, 70), 4, 32, 2, [_set()] * 2), _solvers((20, 70), 4, 32, 2, [None] * 2)
    with pytest.raises(NotImplementedError, match='con_set.*MultiModelConsCemMpc'):
        MultiModelCemMpc.from_solvers(with_set)
    with pytest.raises(NotImplementedError, match='con_set'):
        MultiModelCemMpc.from_solvers([with_set[0], without[1]])
    with pytest.raises(NotImplementedError, match='con_set'):
        MultiModelCemMpc.check_solvers(with_set)       # (pinned by tests/test_conset_host.py too)
    MultiModelCemMpc.from_solvers(without)
    # MultiModelConsCemMpc: one set on all solvers
    MultiModelConsCemMpc.check_solvers(with_set)
    equal = _solvers((20, 70), 4, 32, 2, [_set(), _set()])            # two structs with the same bytes
    MultiModelConsCemMpc.check_solvers(equal)
    for other in (_set(ctrl=False), _set(m_obs=1), make_con_set(2, h_mat_obs=[[1.0, 2.0], [3.0, 4.5]], h_obs=[1.0, 1.0],
                                                                ctrl_ellipsoid=True)):
        differing = _solvers((20, 70), 4, 32, 2, [_set(), other])
        with pytest.raises(ValueError, match='constraint set'):
            MultiModelConsCemMpc.check_solvers(differing)
        with pytest.raises(ValueError, match='constraint set'):
            MultiModelConsCemMpc.from_solvers(differing)
    for some in ([with_set[0], without[1]], [without[0], with_set[1]]):
        with pytest.raises(NotImplementedError, match='con_set'):
            MultiModelConsCemMpc.check_solvers(some)
        with pytest.raises(NotImplementedError, match='con_set'):
            MultiModelConsCemMpc.from_solvers(some)
    with pytest.raises(NotImplementedError, match='con_set'):
        MultiModelConsCemMpc.from_solvers(without)
    # the settings and the environment are compared as in the parent class
    with pytest.raises(ValueError, match='CEM settings'):
        MultiModelConsCemMpc.check_solvers([with_set[0], _solvers((20,), 5, 32, 2, [_set()])[0]])
    moved = _solvers((20,), 4, 32, 2, [_set()])[0]
    env = _env()
    env.beta = 7.0
    moved.set_env(env)
    with pytest.raises(ValueError, match='environment constants'):
        MultiModelConsCemMpc.check_solvers([with_set[0], moved])
    with pytest.raises(ValueError, match='con_set'):
        MultiModelConsCemMpc([_Ssm(), _Ssm()], _env(), 4, 32, 8, 2, device='cpu')
    with pytest.raises(NotImplementedError, match='process group'):
        MultiModelConsCemMpc([_Ssm(), _Ssm()], _env(), 4, 32, 8, 2, device='cpu', con_set=_set(), process_group=mock.Mock())


# ---- get_actions_multi over CemSafeMPCs -----------------------------------------------------------------------------------------------
OBS = {'h_mat_obs': np.array([[1.0, 0.0], [-1.0, 0.0]]), 'h_obs': np.array([[0.7], [0.7]])}
BOTH = dict(cem_obstacle_constraint=True, cem_ctrl_ellipsoid_constraint=True)


def test_get_actions_multi_builds_the_multi_model_solve_with_the_set(monkeypatch):
    import safe_exploration_amd.safempc_cem as sc
    fake = _fake(monkeypatch)
    monkeypatch.setattr(cem_mpc, '_check_solve', lambda owner, x0, q, best, ok, status, where, problems_:
                        (best.clone(), torch.ones(best.size(0), dtype=torch.bool), False))
    built = []

    class Spy(MultiModelConsCemMpc):
        @classmethod
        def from_solvers(cls, solvers):
            built.append(list(solvers))
            return super().from_solvers(solvers)

    monkeypatch.setattr(sc, 'MultiModelConsCemMpc', Spy)
    E, H, iters = 2, conf().mpc_time_horizon, conf().cem_num_iterations
    safempcs = [_safempc_with(conf(**BOTH), OBS) for _ in range(E)]
    # (the optimisers CemSafeMPC would build over a real model, with the set it made from conf and opt_env)
    for e, s in enumerate(safempcs):
        s._mpc = FusedCemMpc(_Ssm(20 + 50 * e), _env(), H, 64, 8, iters, device='cpu', init_std=0.2, seed=e, con_set=s._con_set)
        s._injected_mpc = True
    actions, results = get_actions_multi(safempcs, np.zeros((E, 2)))
    assert actions.shape == (E, 1) and len(results) == E
    multi = safempcs[0]._multi[1]
    assert type(multi) is Spy and built == [[s._mpc for s in safempcs]] and multi.per_model_solves == 0
    assert set(_rollout_entries(fake)) <= set(ENTRIES) and sum(_rollout_entries(fake).values()) == iters
    sent = ctypes.cast(fake.args['sx_cem_rollout_cons_multi'][0][3], ctypes.POINTER(_lib.SxConSet)).contents
    assert (sent.m_obs, sent.ctrl_ellipsoid) == (2, 1) and list(sent.h_obs)[:2] == [0.7, 0.7]
    # the solve is cached, by class
    get_actions_multi(safempcs, np.zeros((E, 2)))
    assert safempcs[0]._multi[1] is multi and len(built) == 1
    # differing sets: ValueError
    other = _safempc_with(conf(**BOTH), dict(OBS, h_obs=np.array([[0.7], [0.6]])))
    other._mpc = FusedCemMpc(_Ssm(70), _env(), H, 64, 8, iters, device='cpu', init_std=0.2, con_set=other._con_set)
    other._injected_mpc = True
    with pytest.raises(ValueError, match='constraint set'):
        get_actions_multi([safempcs[0], other], np.zeros((E, 2)))


def test_get_actions_multi_refuses_a_mixed_list():
    for kw, name in ((dict(cem_ctrl_ellipsoid_constraint=True), 'cem_ctrl_ellipsoid_constraint'),
                     (dict(cem_obstacle_constraint=True), 'cem_obstacle_constraint'),
                     (BOTH, 'cem_ctrl_ellipsoid_constraint / cem_obstacle_constraint')):
        for solvers in ([_safempc_with(conf(**kw), OBS), _safempc(conf())], [_safempc(conf()), _safempc_with(conf(**kw), OBS)]):
            with pytest.raises(NotImplementedError, match='^get_actions_multi.*' + name):
                get_actions_multi(solvers, np.zeros((2, 2)))


def test_the_batch_runners_say_that_they_take_solvers_with_a_set():
    from safe_exploration_amd import episode_runner, safempc_exploration
    assert 'constraint set' in episode_runner.do_rollout_batch.__doc__
    assert 'constraint set' in safempc_exploration.find_max_variance_multi.__doc__


# ---- the inputs of the GPU solve test ----------------------------------------------------------------------------------------------------
def test_the_gpu_multi_solve_inputs_are_decided():
    """Per problem (training sets of 200, 100 and 37 points): in every iteration the last elite and the first non-elite differ
    by more than 1e-6 (or in their constraint cost, which is exact); no distance sits within 1e-6 of the boundary; the last
    iteration ends feasible; and the same solve without the set picks another elite set (here: in every iteration).
    Smallest elite gap 6.65e-5 (problem 0, iteration 3; per problem 6.65e-5, 3.04e-4, 1.22e-3), smallest |d| 2.41e-5 (problem 2,
    iteration 0; per problem 5.95e-5, 1.28e-4, 2.41e-5)."""
    solves = cmo.solves()
    assert len(solves) == cmo.E == 3 and solves[0] is co.solve()
    assert len({s[0].X.shape[0] for s in solves}) == 3, 'the training-set sizes must differ: a wrong table entry would not show'
    specs = [s[0] for s in solves]
    for spec in specs[1:]:      # one environment, one set
        for name in ('a', 'b', 'k_fb', 'l_mu', 'l_sigma', 'h_mat', 'h_vec', 'u_min', 'u_max', 'obj_target'):
            assert np.array_equal(getattr(spec, name), getattr(specs[0], name)), name
    for e, (spec, con, H, x0, init_std, noise, best, trace, plain_best, plain_trace) in enumerate(solves):
        assert con is solves[0][1]
        gaps, plain_gaps = co.elite_gaps(trace, co.K), co.elite_gaps(plain_trace, co.K)
        cost, obj, idx, _ = trace[-1]
        order = ocem.rank(cost, obj, 2)
        best_two = abs(obj[order[0]] - obj[order[1]])
        differ = [set(a[2]) != set(b[2]) for a, b in zip(trace, plain_trace)]
        print(f'problem {e}: elite gaps {gaps}, without the set {plain_gaps}, best two {best_two}, smallest |d| '
              f'{[t[3] for t in trace]}, rows with a violation {[int((t[0] > 0).sum()) for t in trace]}, elite sets differ {differ}')
        assert all(g > co.GAP for g in gaps) and all(g > co.GAP for g in plain_gaps)
        assert cost[order[0]] != cost[order[1]] or best_two > co.GAP
        assert all(t[3] >= co.MARGIN for t in trace)
        assert best is not None and cost[order[0]] == 0 and plain_best is not None
        assert any(differ), f'problem {e}: the set never changes an elite set'
