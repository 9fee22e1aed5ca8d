"""CPU: static exploration in multi-model CEM solves, host side ("the multi-model form") -- the inputs
of tests/test_gpu_static_multi.py's solve are sound on the oracle's numbers alone (tests/static_multi_oracle.py);
sx_cem_rollout_starts_multi, sx_cem_rollout_starts_cons_multi and sx_cem_rollout_starts_multi_form are declared, exported and
bound, check their arguments before any device access and answer SX_ERR_UNSUPPORTED exactly where the plan has no form; the form
query is the fold of sx_cem_rollout_starts_form over the models; MultiModelStaticCemMpc.check_solvers names every mismatch; a
fused find is one launch of the new entry per iteration and a find without a form one single-model launch per scenario and
iteration (a counting fake library in place of the launches); find_max_variance_static_multi refuses a dynamic exploration."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import static_multi_oracle as smo
from safe_exploration_amd import _lib, cem_mpc
from safe_exploration_amd.cem_mpc import MultiModelStaticCemMpc, StaticCemMpc
from test_conset_host import _bad_sets, _fake, _plan_model, _rollout_entries, _set, _shift0_shapes
from test_perf_multi_host import _models, _Ssm
from test_static_explore_host import _env, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
PLAIN, CONS, FORM = 'sx_cem_rollout_starts_multi', 'sx_cem_rollout_starts_cons_multi', 'sx_cem_rollout_starts_multi_form'


# ---- 1: the inputs of the GPU solve -------------------------------------------------------------------------------------------------
def test_the_multi_model_solve_is_decided_and_its_scenarios_differ():
    """Seed 0 (noise seed 300): with the set, smallest elite gap 1.16e-4, smallest |d| 1.24e-5, chosen restarts [1, 2, 2],
    the closest two answers 0.34 apart; without it 2.59e-3, 2.23e-6, [2, 2, 1], 0.46."""
    d = smo.solve()
    assert len(d['specs']) == smo.S == 3 and [s.X.shape[0] for s in d['specs']] == [60, 45, 30]
    assert not np.array_equal(d['specs'][0].X[:30], d['specs'][2].X)           # different training seeds
    assert d['noise'].shape == (smo.ITERS, smo.S * smo.R, smo.P, 2 + smo.H)
    for label, found in (('with the set', d['found']), ('without the set', d['plain_found'])):
        gap, margin, feasible, mixed, apart = smo.conditions(found)
        print(f'seed {d["seed"]} {label}: smallest elite gap {gap:.2e}, smallest |d| {margin:.2e}, chosen restarts '
              f'{[c for _, c, _ in found]}, feasible restarts {[[bool(p[2]) for p in per] for _, _, per in found]}, the closest '
              f'two answers differ by {apart:.3f}')
        assert gap > smo.GAP                                                    # every elite gap of every scenario
        assert margin >= smo.MARGIN                                             # every distance
        assert feasible and all(any(p[2] for p in per) for _, _, per in found)  # every scenario has a feasible restart
        assert mixed and len({c for _, c, _ in found}) > 1                      # the chosen restarts are not all equal
        assert apart > smo.APART                                                # a wrong table entry shows
    assert d['seed'] in smo.SEEDS and smo.holds(smo.conditions(d['found'])) and smo.holds(smo.conditions(d['plain_found']))


# ---- 2: the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name in (PLAIN, CONS, FORM):
        assert re.search(r'\bint ' + name + r'\(', header) and name in _lib.SIGNATURES
        fn = getattr(_lib.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1])
    ours, parent = _lib.SIGNATURES[PLAIN][1], _lib.SIGNATURES['sx_cem_rollout_starts'][1]
    assert ours == parent[:1] + [ctypes.c_void_p] + parent[1:] and len(ours) == 16           # the table behind the models
    cons = _lib.SIGNATURES[CONS][1]
    assert cons == ours[:3] + [ctypes.POINTER(_lib.SxConSet)] + ours[3:]
    assert _lib.SIGNATURES[FORM] == _lib.SIGNATURES['sx_cem_rollout_multi_form']
    build = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'build.sh')).read()
    for src in ('sx_stream_starts_multi.hip', 'sx_stream_starts_cons_multi.hip'):
        assert src in build and os.path.exists(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', src))
        for hdr in ('sx_stream_launch.hpp', 'sx_stream_impl.hpp'):
            assert src in open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', hdr)).read()


def _call(entry=PLAIN, cons='ok', *, models='ok', table=16, env=(), no_env=False, E=2, P=4, H=5, mean=16, std=16, noise=16,
          rows=16, obj=16, con=16, status=16):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    e = _env(*env)
    models = _models(_model(n_train=20), _model(n_train=70)) if isinstance(models, str) else models
    head = (models, p(table), None if no_env else ctypes.byref(e))
    if entry == CONS:
        cons = _set(e.n_s) if isinstance(cons, str) else cons
        head += (None if cons is None else ctypes.byref(cons),)
    return getattr(_lib.lib(), entry)(*head, E, P, H, p(mean), p(std), p(noise), p(rows), None, None, p(obj), p(con), p(status),
                                      None)


ARG_CASES = [('a null model array', dict(models=None)), ('a null table', dict(table=None)), ('a null env', dict(no_env=True)),
             ('a null rows pointer', dict(rows=None)), ('a null obj_cost pointer', dict(obj=None)),
             ('a null con_cost pointer', dict(con=None)), ('a null status pointer', dict(status=None)),
             ('noise without mean', dict(mean=None)), ('noise without std', dict(std=None)), ('E = 0', dict(E=0)),
             ('E < 0', dict(E=-2)), ('P = 0', dict(P=0)), ('H = 0', dict(H=0)),
             ('the second model of another shape than env', dict(models=_models(_model(), _model(2, 2)))),
             ('the first model of another shape than env', dict(models=_models(_model(4, 1), _model()))),
             ('every model of another shape than env', dict(models=_models(_model(2, 2), _model(2, 2)))),
             ('a model without a training set', dict(models=_models(_model(), _model(n_train=0))))]


@pytest.mark.parametrize('entry', [PLAIN, CONS])
def test_argument_errors_without_a_gpu(entry):
    too_big = _models(_model(n_train=20), _model(n_train=1100))         # no streaming form
    for what, kw in ARG_CASES:
        assert _call(entry, **kw) == ARG, what
        if 'models' not in kw:
            # every check comes before the plan: over models without a form it is still the argument's error
            assert _call(entry, models=too_big, **kw) == ARG, what
    if entry == CONS:
        assert _call(entry, None) == ARG
        for what, bad in _bad_sets():
            assert _call(entry, bad) == ARG, what
            assert _call(entry, bad, models=too_big) == ARG, what
        # the parent's checks come first, and garbage in the rows NOT in use is not read
        unused = _set(m_obs=1)
        unused.h_mat_obs[2], unused.h_obs[1] = float('nan'), float('inf')
        assert _call(entry, unused, table=None) == ARG and _call(entry, unused, models=too_big) == UNSUPPORTED


@pytest.mark.parametrize('entry', [PLAIN, CONS])
def test_unsupported_is_answered_exactly_where_the_plan_has_no_form(entry):
    """(Only arguments that are refused: a call that is accepted would launch.)"""
    lib = _lib.lib()
    many = _env()
    many.m = _lib.SX_MAX_M + 1
    cases = [(_models(_model(n_train=20), _model(n_train=1100)), (), {}),
             (_models(_model(n_train=1100), _model(n_train=20)), (), {}),
             (_models(_model(3, 2), _model(3, 2)), (3, 2), {}),
             (_models(_model(1, 1), _model(1, 1, n_train=1000)), (1, 1), dict(H=600))]
    for models, env, kw in cases:
        assert int(lib.sx_cem_rollout_starts_multi_form(models, 2, kw.get('H', 5))) < 0
        assert _call(entry, models=models, env=env, **kw) == UNSUPPORTED, (env, kw)
    # the same models with a form at another horizon are not refused by the plan (a bad pointer keeps the call from launching)
    assert int(lib.sx_cem_rollout_starts_multi_form(cases[3][0], 2, 40)) == SX_FORM_STREAM


def test_the_form_query_is_the_fold_of_the_single_model_query():
    lib = _lib.lib()
    form = lambda ms, H: int(lib.sx_cem_rollout_starts_multi_form(_models(*ms), len(ms), H))
    compiled = _shift0_shapes()
    assert compiled == [(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2)]
    seen = set()
    for n_s, n_u in compiled:
        for H in (3, 15, 40):
            single = [int(lib.sx_cem_rollout_starts_form(ctypes.byref(_plan_model(n_s, n_u, N)), H)) for N in range(1, 1100)]
            edges = [N + 1 for N in range(1, 1099) if single[N] != single[N - 1]]          # single[N - 1] is the form of N
            sizes = sorted({7, 200, 1000} | {N for edge in edges for N in (edge - 1, edge)})
            for N in sizes:
                for other in (7, N):
                    # (a scenario with restarts: its model stands several times in the list)
                    ms = [_plan_model(n_s, n_u, other)] * 2 + [_plan_model(n_s, n_u, N)] * 2
                    alone = [single[other - 1], single[N - 1]]
                    want = -1 if min(alone) < 0 else SX_FORM_BYOUT if SX_FORM_BYOUT in alone else SX_FORM_STREAM
                    got = form(ms, H)
                    assert got == want == int(lib.sx_cem_rollout_multi_form(_models(*ms), len(ms), H)), (n_s, n_u, H, other, N)
                    seen.add(got)
    assert seen == {SX_FORM_STREAM, SX_FORM_BYOUT, -1}
    small, mid, big = _plan_model(4, 1, 33), _plan_model(4, 1, 200), _plan_model(4, 1, 590)
    assert form([small, mid], 3) == SX_FORM_STREAM and form([big, mid, small], 3) == form([small, big], 15) == SX_FORM_BYOUT
    for ms, E, H in ((None, 2, 5), (_models(small, mid), 0, 5), (_models(small, _plan_model(2, 1, 20)), 2, 5),
                     (_models(small, _plan_model(4, 1, 0)), 2, 5), (_models(small, mid), 2, 0),
                     (_models(_plan_model(3, 2, 20)), 1, 5)):
        assert int(lib.sx_cem_rollout_starts_multi_form(ms, E, H)) < 0


# ---- 3: check_solvers ---------------------------------------------------------------------------------------------------------------
def _solver(n_train=20, ssm=None, env=None, R=2, P=32, H=4, k=4, iters=3, device='cpu', **kw):
    kw.setdefault('start_mean', [0.5, -0.5])
    kw.setdefault('start_std', [0.25, 0.125])
    return StaticCemMpc(ssm or _Ssm(n_train), env or _env(), H, P, k, iters, n_restarts=R, init_std=0.2, device=device, **kw)


class _Ssm41(_Ssm):
    num_states, num_actions = 4, 1


def test_check_solvers_names_every_mismatch():
    ok = [_solver(20), _solver(70, start_mean=[0.1, 0.2], start_std=[0.3, 0.3], seed=5)]
    MultiModelStaticCemMpc.check_solvers(ok)                  # start distributions and seeds may differ per scenario
    MultiModelStaticCemMpc.from_solvers(ok)
    for kw, name in ((dict(H=5), 'time_horizon'), (dict(P=64), 'num_rollouts'), (dict(k=8), 'num_elites'),
                     (dict(iters=4), 'num_iterations'), (dict(R=3), 'n_restarts'), (dict(device='meta'), 'device')):
        with pytest.raises(ValueError, match='must share ' + name + '.*solver 1'):
            MultiModelStaticCemMpc.check_solvers([_solver(20), _solver(70, **kw)])
        with pytest.raises(ValueError, match=name):
            MultiModelStaticCemMpc.from_solvers([_solver(20), _solver(70, **kw)])
    other = _solver(70, ssm=_Ssm41(70), env=_env(4, 1), start_mean=[0.0] * 4, start_std=[0.1] * 4)
    with pytest.raises(ValueError, match=r'\(n_s, n_u\).*\(2, 1\).*\(4, 1\)'):
        MultiModelStaticCemMpc.check_solvers([_solver(20), other])
    moved = _env()
    moved.beta = 7.0
    with pytest.raises(ValueError, match='environment constants.*solver 1'):
        MultiModelStaticCemMpc.check_solvers([_solver(20), _solver(70, env=moved)])
    # the sets: byte-equal on all solvers, or on none
    MultiModelStaticCemMpc.check_solvers([_solver(20, con_set=_set()), _solver(70, con_set=_set())])
    for differing in (_set(ctrl=False), _set(m_obs=1)):
        with pytest.raises(ValueError, match='constraint set.*solver 1'):
            MultiModelStaticCemMpc.check_solvers([_solver(20, con_set=_set()), _solver(70, con_set=differing)])
    for some in ([_solver(20, con_set=_set()), _solver(70)], [_solver(20), _solver(70, con_set=_set())]):
        with pytest.raises(NotImplementedError, match='con_set.*1 of 2'):
            MultiModelStaticCemMpc.check_solvers(some)
    # a model that is not an exact RBF GP (the single-model solver refuses it at construction; here it changed afterwards)
    for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
        bad = _solver(70)
        bad._ssm.kernel_family = family
        with pytest.raises(NotImplementedError, match='exact RBF GPs: solver 1.*' + family):
            MultiModelStaticCemMpc.check_solvers([_solver(20), bad])
    with pytest.raises(ValueError, match='at least one'):
        MultiModelStaticCemMpc.from_solvers([])


# ---- 4: the plumbing over a counting fake library -----------------------------------------------------------------------------------
def _host_hand_off(monkeypatch):
    """`_hand_off` without a device: the arguments as they are."""
    def hand_off(owner, best, best_ok, status, q_block):
        return status.to(torch.int64).clone(), best_ok != 0, False, best.clone()
    monkeypatch.setattr(cem_mpc, '_hand_off', hand_off)


@pytest.mark.parametrize('with_set', [False, True])
def test_a_fused_find_is_one_launch_of_the_new_entry_per_iteration(monkeypatch, with_set):
    fake = _fake(monkeypatch)
    _host_hand_off(monkeypatch)
    S, R, P, H, iters = 3, 2, 32, 4, 3
    kw = dict(con_set=_set()) if with_set else {}
    solvers = [_solver(n, R=R, P=P, H=H, iters=iters, seed=10 * s, start_mean=[0.1 * s, -0.5], **kw)
               for s, n in enumerate((7, 200, 590))]
    mpc = MultiModelStaticCemMpc.from_solvers(solvers)
    assert mpc.fused_applies() and mpc.form() == SX_FORM_BYOUT           # (590 points: output by output for all)
    fake.calls.clear()
    drawn = []
    for s in solvers:
        s.sample_noise = lambda s=s, own=s.sample_noise: drawn.append(s) or own()
    answers = mpc.find()
    entry = CONS if with_set else PLAIN
    assert _rollout_entries(fake) == {entry: iters}                      # and no single-model rollout entry
    assert fake.calls['sx_gp_model_table'] == 1 and fake.calls['sx_cem_pack_result'] == 0
    assert drawn == solvers                                              # every solver's own draws, once
    for args in fake.args[entry]:
        assert len(args) == (17 if with_set else 16)
        assert args[4 if with_set else 3:][:3] == (S * R, P, H)
        assert [args[0][e].n_train for e in range(S * R)] == [7, 7, 200, 200, 590, 590]      # problem e = s R + r
        if with_set:
            assert bytes(ctypes.cast(args[3], ctypes.POINTER(_lib.SxConSet)).contents) == bytes(_set())
        assert ctypes.cast(args[2], ctypes.POINTER(_lib.SxEnv)).contents.obj_mode == _lib.SX_OBJ_NEG_VARIANCE
    assert len(answers) == S and all(a is not None and a[0].shape == (2,) and a[1].shape == (H, 1) for a in answers)
    for s in solvers:
        assert tuple(s.last_rows.shape) == (R, 2 + H) and tuple(s.last_costs.shape) == (R, 2)
        assert s.last_choice == 0 and s.last_status == 0
    assert mpc.last_status == [0] * S and mpc.per_model_solves == 0 and mpc.stepwise_fallbacks == 0
    # the table is kept while the models stay
    mpc.find()
    assert fake.calls['sx_gp_model_table'] == 1 and fake.calls[entry] == 2 * iters
    # the wrapper alone
    fake.calls.clear()
    rows = torch.zeros((2, 4, 2 + H), dtype=torch.float64)
    out = cem_mpc.cem_rollout_starts_multi([_Ssm(7), _Ssm(200)], _env(), H, rows=rows, **kw)
    assert _rollout_entries(fake) == {entry: 1} and tuple(out['status'].shape) == (2,)
    with pytest.raises(ValueError, match='3 models for 2 problems'):
        cem_mpc.cem_rollout_starts_multi([_Ssm()] * 3, _env(), H, rows=rows)
    with pytest.raises(ValueError, match='one word per problem'):
        cem_mpc.cem_rollout_starts_multi([_Ssm()] * 2, _env(), H, rows=rows, status=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match='exact RBF GPs'):
        cem_mpc.cem_rollout_starts_multi([_Ssm(), _Ssm(family='feature')], _env(), H, rows=rows)


def test_without_a_form_every_scenario_solves_alone_with_the_same_noise(monkeypatch):
    fake = _fake(monkeypatch)
    _host_hand_off(monkeypatch)
    S, R, P, H, iters = 3, 2, 32, 4, 3
    solvers = [_solver(n, R=R, P=P, H=H, iters=iters) for n in (20, 1100, 70)]          # 1100: no streaming form
    mpc = MultiModelStaticCemMpc.from_solvers(solvers)
    assert not mpc.fused_applies()
    noise = torch.randn((iters, S * R, P, 2 + H), dtype=torch.float64)
    fake.calls.clear()
    answers = mpc.find(noise)
    assert _rollout_entries(fake) == {'sx_cem_rollout_starts': S * iters}
    assert mpc.per_model_solves == 1 and len(answers) == S
    for s, m in enumerate(solvers):
        assert torch.equal(m._last_noise, noise[:, s * R:(s + 1) * R])
    # `solve` itself does not fall back: what the library answers for such models raises
    monkeypatch.setattr(fake, PLAIN, lambda *a: UNSUPPORTED, raising=False)
    with pytest.raises(cem_mpc.FusedMultiUnsupported):
        mpc.solve(noise)


def test_status_is_handled_per_scenario(monkeypatch):
    """Scenario 1's words carry NAN | ZERO_FIX: it alone repeats through its own step-by-step solve; a NaN that stays raises
    with the scenario's number."""
    _fake(monkeypatch)
    S, R, P, H, iters = 3, 2, 32, 4, 2
    both = _lib.SX_STATUS_NAN | _lib.SX_STATUS_ZERO_FIX

    def hand_off(owner, best, best_ok, status, q_block):
        words = status.to(torch.int64).clone()
        if isinstance(owner, MultiModelStaticCemMpc):
            words[3] = both                                           # problem 3 = scenario 1, restart 1
        return words, best_ok != 0, False, best.clone()
    monkeypatch.setattr(cem_mpc, '_hand_off', hand_off)
    solvers = [_solver(n, R=R, P=P, H=H, iters=iters) for n in (20, 70, 100)]
    repeats = []
    for s, m in enumerate(solvers):
        def solve(noise=None, stepwise=False, s=s, m=m):
            repeats.append((s, stepwise, tuple(noise.shape)))
            L = 2 + H
            return (torch.full((R, L), 5.0, dtype=torch.float64), torch.zeros((R, 2), dtype=torch.float64),
                    torch.ones(R, dtype=torch.int32), [], torch.full((1,), m.repeat_status, dtype=torch.int32))
        m.solve, m.repeat_status = solve, 0
    mpc = MultiModelStaticCemMpc.from_solvers(solvers)
    answers = mpc.find()
    assert repeats == [(1, True, (iters, R, P, 2 + H))]
    assert mpc.stepwise_fallbacks == 1 and [m.stepwise_fallbacks for m in solvers] == [0, 1, 0]
    assert float(answers[1][0][0]) == 5.0 and float(answers[0][0][0]) == 0.0 and mpc.last_status == [0, 0, 0]
    solvers[1].repeat_status = _lib.SX_STATUS_NAN
    monkeypatch.setattr(cem_mpc, 'save_failure_state', lambda *a: 'nowhere')
    with pytest.raises(Exception, match=r'scenario 1'):
        mpc.find()
    assert mpc.last_status == [0, _lib.SX_STATUS_NAN, 0]


# ---- 5: the public surface -----------------------------------------------------------------------------------------------------------
def test_find_max_variance_static_multi_takes_static_explorations_only():
    from safe_exploration_amd import safempc_exploration as se
    dynamic = object.__new__(se.DynamicSafeMPCExploration)
    static = object.__new__(se.StaticSafeMPCExploration)
    for bad in ([dynamic], [static, dynamic], [static, object()]):
        with pytest.raises(TypeError, match='StaticSafeMPCExploration'):
            se.find_max_variance_static_multi(bad)
    with pytest.raises(ValueError, match='at least one'):
        se.find_max_variance_static_multi([])


def test_find_max_variance_static_multi_keeps_its_solver_between_calls(monkeypatch):
    from safe_exploration_amd import safempc_exploration as se
    _fake(monkeypatch)
    _host_hand_off(monkeypatch)

    def exploration(n):
        x = object.__new__(se.StaticSafeMPCExploration)
        x._solver, x.n_s, x.n_u, x.verbosity = _solver(n), 2, 1, 0
        return x
    xs = [exploration(n) for n in (20, 70, 100)]
    out = se.find_max_variance_static_multi(xs)
    assert len(out) == 3 and all(x.shape == (2, 1) and u.shape == (1, 1) for x, u in out)
    multi = xs[0]._static_multi
    assert isinstance(multi, MultiModelStaticCemMpc) and multi.solvers == [x._solver for x in xs]
    se.find_max_variance_static_multi(xs)
    assert xs[0]._static_multi is multi                                    # kept
    xs[2]._solver = _solver(100)
    se.find_max_variance_static_multi(xs)
    assert xs[0]._static_multi is not multi                                # rebuilt when the list of solvers changes
    # no feasible restart: (None, None), as find_max_variance
    monkeypatch.setattr(MultiModelStaticCemMpc, 'find', lambda self, noise=None: [None] * 3)
    assert se.find_max_variance_static_multi(xs) == [(None, None)] * 3
