"""CPU: the SafeMPC constraint set of the CEM rollout (sx_con_set), host side -- the struct has the
C layout; sx_conset_eval, sx_cem_rollout_cons and sx_cem_rollout_elites_cons answer every argument error before any device
access and SX_ERR_UNSUPPORTED exactly where sx_cem_rollout_sat does; the form query is plan_stream's; the compiled shapes are
the shift-0 shapes of SX_ROLLOUT_SHAPES; over a fake library a FusedCemMpc(con_set=...) solve reaches the _cons entries and
nothing else, the step-by-step path charges every step through sx_conset_eval, and without a set both call what they called
before; the refusals at construction name their setting; and the inputs of the GPU tests (tests/test_gpu_conset.py) are
decided on the numpy oracle (tests/conset_oracle.py): no distance within 1e-6 of the boundary, every signal mixed."""
import ctypes
import os
import re
import subprocess
from unittest import mock

import numpy as np
import pytest
import torch

import conset_oracle as co
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc
from safe_exploration_amd.gp_reachability_pytorch import make_con_set
from safe_exploration_amd.safempc_cem import CemSafeMPC, get_actions_multi
from test_perf_multi_host import FakeLib, _env, _model, _safempc, _Ssm, conf
from test_sat_cost_host import COST2, _bad_costs, _cost, _hook, p
from test_static_explore_host import form_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
ENTRIES = {'sx_cem_rollout_cons': 'sx_cem_rollout', 'sx_cem_rollout_elites_cons': 'sx_cem_rollout_elites'}


def _set(n_s=2, m_obs=2, ctrl=True):
    rows = np.arange(1, m_obs * n_s + 1, dtype=np.float64).reshape(m_obs, n_s) if m_obs else None
    return make_con_set(n_s, h_mat_obs=rows, h_obs=None if rows is None else np.ones(m_obs), ctrl_ellipsoid=ctrl)


def _bad_sets():
    out = []
    for what, field, value in (('m_obs = -1', 'm_obs', -1), ('m_obs = SX_MAX_M + 1', 'm_obs', _lib.SX_MAX_M + 1),
                               ('ctrl_ellipsoid = 2', 'ctrl_ellipsoid', 2), ('ctrl_ellipsoid = -1', 'ctrl_ellipsoid', -1)):
        c = _set()
        setattr(c, field, value)
        out.append((what, c))
    for what, field, at, value in (('a NaN row entry', 'h_mat_obs', 3, float('nan')), ('an infinite bound', 'h_obs', 1, float('inf'))):
        c = _set()
        getattr(c, field)[at] = value
        out.append((what, c))
    return out


# ---- declarations and layout -----------------------------------------------------------------------------------------------------
def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sx_amd.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(sx_con_set), offsetof(sx_con_set, m_obs),'
                   'offsetof(sx_con_set, ctrl_ellipsoid), offsetof(sx_con_set, h_mat_obs), offsetof(sx_con_set, h_obs));'
                   'return 0;}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    C = _lib.SxConSet
    assert got == [ctypes.sizeof(C), C.m_obs.offset, C.ctrl_ellipsoid.offset, C.h_mat_obs.offset, C.h_obs.offset]
    assert ctypes.sizeof(C) == 8 + 8 * _lib.SX_MAX_M * (_lib.SX_MAX_NS + 1)


def test_entries_are_declared_with_the_parents_arguments_plus_the_set_and_the_cost():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name, parent in ENTRIES.items():
        assert re.search(r'\bint ' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        ours, theirs = _lib.SIGNATURES[name][1], _lib.SIGNATURES[parent][1]
        # (sx_cem_rollout_cons takes no workspace: two arguments fewer)
        assert len(ours) == len(theirs) + 2 - (2 if name == 'sx_cem_rollout_cons' else 0)
        assert ours[:2] == theirs[:2] and ours[2] == ctypes.POINTER(_lib.SxConSet) and ours[3] == ctypes.POINTER(_lib.SxSatCost)
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        assert len(decl.split(',')) == len(ours)
    for name in ('sx_cem_rollout_cons_form', 'sx_conset_eval'):
        assert re.search(r'\bint ' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    decl = re.search(r'\bint sx_conset_eval\((.*?)\);', header, re.S).group(1)
    assert len(decl.split(',')) == len(_lib.SIGNATURES['sx_conset_eval'][1])


def test_make_con_set():
    c = make_con_set(3, h_mat_obs=[[1, 2, 3], [4, 5, 6]], h_obs=[7, 8], ctrl_ellipsoid=True)
    assert (c.m_obs, c.ctrl_ellipsoid) == (2, 1)
    assert list(c.h_mat_obs)[:7] == [1, 2, 3, 4, 5, 6, 0] and list(c.h_obs)[:3] == [7, 8, 0]      # rows n_s apart
    c = make_con_set(2)
    assert (c.m_obs, c.ctrl_ellipsoid) == (0, 0)
    for kw in (dict(h_mat_obs=[[1, 2]]), dict(h_obs=[1]), dict(h_mat_obs=np.ones((17, 2)), h_obs=np.ones(17)),
               dict(h_mat_obs=[[np.nan, 1]], h_obs=[1]), dict(h_mat_obs=[[1, 1]], h_obs=[np.inf])):
        with pytest.raises(ValueError):
            make_con_set(2, **kw)
    with pytest.raises(ValueError):
        make_con_set(5)
    # the oracle's set gives the struct the device reads
    spec = co.pendulum_spec()
    s = co.pendulum_set(spec).struct(2)
    assert (s.m_obs, s.ctrl_ellipsoid) == (2, 1) and list(s.h_obs)[:2] == list(co.OBSTACLE_SCALE * spec.h_vec[:2, 0])


# ---- argument errors, before any device access -----------------------------------------------------------------------------------
def _call(cons, cost=None, *, elites=False, model=None, env=None, E=2, P=4, H=5, x0=16, mean=16, std=16, noise=16, actions=16,
          obj=16, con=16, status=16, rows=16, k=3, mean_out=None, std_out=None):
    env = env if env is not None else _env()
    head = (None if model == 'null' else ctypes.byref(model or _model()), ctypes.byref(env),
            None if cons is None else ctypes.byref(cons), None if cost is None else ctypes.byref(cost))
    entry = 'sx_cem_rollout' + ('_elites' if elites else '') + '_cons'
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
    # the set: null or invalid
    assert call(None) == ARG
    for what, bad in _bad_sets():
        assert call(bad) == ARG, what
    # garbage in the rows NOT in use is not read
    unused = _set(m_obs=1)
    unused.h_mat_obs[2], unused.h_obs[1] = float('nan'), float('inf')
    assert call(unused, x0=None) == ARG and call(unused, model=_model(n_train=1100)) == UNSUPPORTED
    # a bad cost
    for what, bad in _bad_costs():
        assert call(cost=bad) == ARG, what
    # what the parents answer SX_ERR_ARG for
    for kw in (dict(x0=None), dict(actions=None), dict(obj=None), dict(con=None), dict(status=None), dict(E=0), dict(P=0),
               dict(H=0), dict(model=_model(2, 2)), dict(model='null')):
        assert call(**kw) == ARG, kw
    if elites:
        for kw in (dict(rows=None), dict(noise=None), dict(k=0), dict(mean_out=16), dict(std_out=16)):
            assert call(**kw) == ARG, kw
    else:
        assert call(mean=None) == ARG and call(std=None) == ARG
    # SX_ERR_UNSUPPORTED exactly where sx_cem_rollout_sat answers it, before any launch: m beyond SX_MAX_M, a shape without
    # a kernel, the workspace path, neither streaming form, the elite-row limit
    many = _env()
    many.m = _lib.SX_MAX_M + 1
    assert call(env=many) == UNSUPPORTED
    cost3 = _cost(3, 0, 1) if with_cost else None
    assert call(_set(3), cost3, model=_model(3, 2), env=_env(3, 2)) == UNSUPPORTED
    assert call(model=_model(n_train=1100)) == UNSUPPORTED
    cost1 = _cost(1, 0, 1) if with_cost else None
    assert call(_set(1), cost1, model=_model(1, 1, n_train=1000), env=_env(1, 1), H=600) == UNSUPPORTED
    if elites:
        assert call(H=385) == UNSUPPORTED
    # a bad set (or cost) on a model without a form is the argument's error: it is checked before the plan
    assert call(_bad_sets()[0][1], model=_model(n_train=1100)) == ARG
    if with_cost:
        assert call(cost=_cost(rank=0), model=_model(n_train=1100)) == ARG


def _eval(cons, *, env=None, P=4, u=16, q_start=16, p_next=16, q_next=16, check=1, out=16):
    env = env if env is not None else _env()
    return _lib.lib().sx_conset_eval(None if env == 'null' else ctypes.byref(env), None if cons is None else ctypes.byref(cons),
                                     P, p(u), p(q_start), p(p_next), p(q_next), check, p(out), None)


def test_eval_argument_errors_without_a_gpu():
    ok = _set()
    assert _eval(None) == ARG and _eval(ok, env='null') == ARG
    for what, bad in _bad_sets():
        assert _eval(bad) == ARG, what
    for kw in (dict(u=None), dict(out=None), dict(P=0), dict(p_next=None), dict(q_next=None), dict(env=_env(5, 1)),
               dict(env=_env(0, 1)), dict(env=_env(2, 3)), dict(env=_env(2, 0))):
        assert _eval(ok, **kw) == ARG, kw


# ---- the form query and the compiled shapes ----------------------------------------------------------------------------------------
def _shift0_shapes():
    text = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'sx_stream_launch.hpp')).read()
    body = re.search(r'#define SX_ROLLOUT_SHAPES\(X, \.\.\.\)(.*?)\n\n', text, re.S).group(1)
    shapes = [tuple(int(v) for v in m) for m in re.findall(r'X\((\d), (\d), (\d), __VA_ARGS__\)', body)]
    assert len(shapes) == 13
    return sorted((n_s, n_u) for n_s, n_u, sh in shapes if sh == 0)


def _plan_model(n_s, n_u, n_train):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.n_pad = (n_train + 1 + n_s + n_u + 15) // 16 * 16   # sx_gp.hpp: gp_n_pad
    m.x_train = m.a_pack = m.stage_tab = 0x1000             # never dereferenced
    return m


def test_the_form_query_is_the_streaming_plan_on_the_compiled_shapes():
    """(stream_form does not read the SX_ROLLOUT override: these entries have the streaming kernel only.)"""
    lib = _lib.lib()
    compiled = _shift0_shapes()
    assert compiled == [(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2)]
    seen = set()
    for n_s in range(1, _lib.SX_MAX_NS + 1):
        for n_u in range(1, _lib.SX_MAX_NU + 1):
            for steps in (2, 3, 15, 40, 400):
                for N in list(range(1, 1200, 13)) + [2000]:
                    m = _plan_model(n_s, n_u, N)
                    got = int(lib.sx_cem_rollout_cons_form(ctypes.byref(m), steps))
                    want = form_rule(n_s, n_u, m.n_pad, steps) if (n_s, n_u) in compiled else -1
                    assert got == want == int(lib.sx_cem_rollout_sat_form(ctypes.byref(m), steps)), (n_s, n_u, N, steps)
                    seen.add(got)
    assert seen == {SX_FORM_STREAM, SX_FORM_BYOUT, -1}
    assert int(lib.sx_cem_rollout_cons_form(None, 5)) < 0 and int(lib.sx_cem_rollout_cons_form(ctypes.byref(_model()), 0)) < 0
    # the entries answer SX_ERR_UNSUPPORTED for exactly the other shapes (the model's form aside)
    for n_s in range(1, _lib.SX_MAX_NS + 1):
        for n_u in range(1, _lib.SX_MAX_NU + 1):
            code = _call(_set(n_s), model=_model(n_s, n_u), env=_env(n_s, n_u), x0=None)
            assert code == ARG      # (the arguments come first)
            if (n_s, n_u) not in compiled:
                assert _call(_set(n_s), model=_model(n_s, n_u), env=_env(n_s, n_u)) == UNSUPPORTED


def test_both_translation_units_are_built():
    text = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'build.sh')).read()
    for src in ('sx_conset.hip', 'sx_stream_cons.hip', 'sx_stream_cons_sat.hip'):
        assert src in text and os.path.exists(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', src))


# ---- the plumbing over a fake library ----------------------------------------------------------------------------------------------
class _Lib(FakeLib):
    HOST_ONLY = FakeLib.HOST_ONLY + ('sx_cem_rank_counts',)


def _fake(monkeypatch):
    fake = _Lib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: fake)
    monkeypatch.setattr(_lib, 'require_gpu', lambda *a: None)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda dev: None)

    def rank(con, obj, actions, kk, want_rows=False, want_refit=True):
        E, L = con.size(0), actions[0, 0].numel()
        full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64)
        return dict(elite_rows=full(0, E, kk, 2 + L) if want_rows else None, mean=full(1, E, L) if want_refit else None,
                    std=full(2, E, L) if want_refit else None, best=torch.zeros((E, L), dtype=torch.float64),
                    best_ok=torch.ones(E, dtype=torch.int32))

    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)
    return fake


def _rollout_entries(fake):
    return {name: n for name, n in fake.calls.items() if name.startswith('sx_cem_rollout') and n
            and not name.endswith(('_form', '_bytes'))}


@pytest.mark.parametrize('with_cost', [False, True])
def test_a_solve_with_a_set_reaches_the_cons_entries_only(monkeypatch, with_cost):
    fake = _fake(monkeypatch)
    iters, P, H = 3, 4096, 4       # (4096 candidates: the counting ranking, whose refit moves into the rollout's prologue)
    ssm = _Ssm(200)
    ssm.workspace = lambda nbytes: None
    cons = _set()
    mpc = FusedCemMpc(ssm, _env(), H, P, 8, iters, device='cpu', init_std=0.2, con_set=cons, cost_on_safety=with_cost)
    if with_cost:
        mpc.set_env(_env(), objective_hook=_hook)
        mpc.set_cost(COST2)
    assert mpc._refit_in_prologue(1)
    mpc.solve(torch.zeros((1, 2), dtype=torch.float64))
    assert _rollout_entries(fake) == {'sx_cem_rollout_cons': 1, 'sx_cem_rollout_elites_cons': iters - 1}
    first = fake.args['sx_cem_rollout_cons'][0]
    assert len(first) == 19 and first[4:7] == (1, P, H)
    assert ctypes.cast(first[2], ctypes.POINTER(_lib.SxConSet)).contents.m_obs == 2
    if with_cost:
        assert ctypes.cast(first[3], ctypes.POINTER(_lib.SxSatCost)).contents.rank == COST2.rank
    else:
        assert first[3] is None
    for args in fake.args['sx_cem_rollout_elites_cons']:
        assert len(args) == 21 and args[4:7] == (1, P, H) and args[10] == 8
    # set_env keeps the set
    fake.calls.clear()
    mpc.set_env(_env(), objective_hook=_hook if with_cost else None)
    mpc.solve(torch.zeros((2, 2), dtype=torch.float64))
    assert set(_rollout_entries(fake)) <= set(ENTRIES) and sum(_rollout_entries(fake).values()) == iters
    # without a set the same solver calls what it called before
    fake.calls.clear()
    plain = FusedCemMpc(ssm, _env(), H, P, 8, iters, device='cpu', init_std=0.2, cost_on_safety=with_cost)
    if with_cost:
        plain.set_cost(COST2)
    plain.solve(torch.zeros((1, 2), dtype=torch.float64))
    sfx = '_sat' if with_cost else ''
    assert _rollout_entries(fake) == {'sx_cem_rollout' + sfx: 1, 'sx_cem_rollout_elites' + sfx: iters - 1}
    assert 'sx_conset_eval' not in fake.calls


def test_the_stepwise_path_charges_every_step_through_the_eval(monkeypatch):
    """solve(stepwise=True), what the NAN | ZERO_FIX repeat runs: one sx_conset_eval per step, the obstacle rows on every
    step but the last, q_start NULL at the first step only; no rollout entry."""
    fake = _fake(monkeypatch)
    iters, P, H = 2, 32, 4
    ssm = _Ssm(20)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    ssm.predict_without_jacobians = lambda x, u: (zeros(x.size(0), 2), zeros(x.size(0), 2))
    ssm.predict_with_jacobians = lambda x, u: (zeros(x.size(0), 2), zeros(x.size(0), 2), zeros(x.size(0), 2, 3))
    mpc = FusedCemMpc(ssm, _env(), H, P, 8, iters, device='cpu', init_std=0.2, con_set=_set())
    mpc.solve(torch.zeros((1, 2), dtype=torch.float64), stepwise=True)
    assert _rollout_entries(fake) == {} and fake.calls['sx_conset_eval'] == fake.calls['sx_onestep_reach'] == iters * H
    calls = fake.args['sx_conset_eval']
    assert [c[7] for c in calls] == [1, 1, 1, 0] * iters
    assert [c[4] is None for c in calls] == [True, False, False, False] * iters
    assert all(c[2] == P for c in calls)
    # without a set: the box test in torch, as before
    fake.calls.clear()
    FusedCemMpc(ssm, _env(), H, P, 8, iters, device='cpu', init_std=0.2).solve(zeros(1, 2), stepwise=True)
    assert 'sx_conset_eval' not in fake.calls and fake.calls['sx_onestep_reach'] == iters * H
    with pytest.raises(TypeError, match='SxConSet'):
        cem_mpc.cem_rollout_stepwise(ssm, _env(), zeros(2), zeros(P, H, 1), status=torch.zeros(1, dtype=torch.int32),
                                     con_set='set')


# ---- the refusals at construction ------------------------------------------------------------------------------------------------
def test_the_fused_solver_refuses_what_is_not_built(monkeypatch):
    _fake(monkeypatch)
    mk = lambda ssm=None, **kw: FusedCemMpc(ssm or _Ssm(), _env(), 4, 32, 8, 2, device='cpu', con_set=_set(), **kw)
    for family in ('feature', 'mlp', 'rbf_junk', 'feature_junk', 'stepwise'):
        with pytest.raises(NotImplementedError, match='con_set.*exact RBF GPs'):
            mk(_Ssm(family=family))
    for kw in (dict(n_perf=6), dict(n_perf=6, perf_type='taylor'), dict(n_perf=6, perf_variance=True)):
        with pytest.raises(NotImplementedError, match='con_set.*n_perf'):
            mk(**kw)
    with pytest.raises(NotImplementedError, match='con_set.*process group'):
        mk(process_group=mock.Mock())
    with pytest.raises(TypeError, match='SxConSet'):
        FusedCemMpc(_Ssm(), _env(), 4, 32, 8, 2, device='cpu', con_set=dict(m_obs=0))
    solvers = [mk(), mk()]
    with pytest.raises(NotImplementedError, match='con_set'):
        MultiModelCemMpc.check_solvers(solvers)
    with pytest.raises(NotImplementedError, match='con_set'):
        MultiModelCemMpc.check_solvers([mk(), FusedCemMpc(_Ssm(), _env(), 4, 32, 8, 2, device='cpu')])
    # the wrapper itself
    x0, noise = torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1, 4, 3, 1), dtype=torch.float64)
    mean = torch.zeros((1, 3, 1), dtype=torch.float64)
    for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
        with pytest.raises(NotImplementedError, match='exact RBF GPs'):
            cem_mpc.cem_rollout(_Ssm(family=family), _env(), x0, 3, mean=mean, std=mean, noise=noise, con_set=_set())
    with pytest.raises(TypeError, match='SxConSet'):
        cem_mpc.cem_rollout(_Ssm(), _env(), x0, 3, mean=mean, std=mean, noise=noise, con_set='set')


def _safempc_with(c, opt_env_extra=None, family='rbf', mpc=None):
    spec = problems.pendulum(n_train=8, obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=-0.1)
    ssm = mock.Mock()
    ssm.kernel_family = family
    return CemSafeMPC(ssm, [], env, c, dict({'lin_model': (spec.a, spec.b)}, **(opt_env_extra or {})), wx_feedback_cost=None,
                      wu_feedback_cost=None, lqr=mock.Mock(), mpc=mpc, beta_safety=2.0, safe_policy=lambda x: spec.k_fb @ x)


def test_the_conf_settings_of_cemsafempc(monkeypatch):
    obs = {'h_mat_obs': np.array([[1.0, 0.0], [-1.0, 0.0]]), 'h_obs': np.array([[0.7], [0.7]])}
    # off by default: no set at all
    assert _safempc(conf())._con_set is None and _safempc_with(conf(), obs)._con_set is None
    s = _safempc_with(conf(cem_ctrl_ellipsoid_constraint=True), obs)
    assert (s._con_set.m_obs, s._con_set.ctrl_ellipsoid) == (0, 1)           # the obstacle rows need their own setting
    s = _safempc_with(conf(cem_obstacle_constraint=True), obs)
    assert (s._con_set.m_obs, s._con_set.ctrl_ellipsoid) == (2, 0) and list(s._con_set.h_obs)[:2] == [0.7, 0.7]
    s = _safempc_with(conf(cem_obstacle_constraint=True, cem_ctrl_ellipsoid_constraint=True), obs)
    assert (s._con_set.m_obs, s._con_set.ctrl_ellipsoid) == (2, 1)
    # None means no rows, as in CautiousCemMPC
    for extra in (None, {'h_mat_obs': None, 'h_obs': None}):
        s = _safempc_with(conf(cem_obstacle_constraint=True), extra)
        assert (s._con_set.m_obs, s._con_set.ctrl_ellipsoid) == (0, 0)
    # the refusals name the setting
    for kw, name in ((dict(cem_ctrl_ellipsoid_constraint=True), 'cem_ctrl_ellipsoid_constraint'),
                     (dict(cem_obstacle_constraint=True), 'cem_obstacle_constraint')):
        with pytest.raises(NotImplementedError, match=name + '.*cem_n_perf'):
            _safempc_with(conf(cem_n_perf=6, **kw), obs)
        for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
            with pytest.raises(NotImplementedError, match=name + '.*exact RBF GP'):
                _safempc_with(conf(**kw), obs, family=family)
        with pytest.raises(NotImplementedError, match='static exploration.*' + name):
            _safempc_with(conf(**kw), obs).static_solver(2, np.zeros(2), np.ones(2))
        with pytest.raises(NotImplementedError, match='get_actions_multi.*' + name):
            get_actions_multi([_safempc_with(conf(**kw), obs), _safempc(conf())], np.zeros((2, 2)))
    # the optimiser it builds carries the set; without the settings it is built as before
    built = {}

    class Spy(FusedCemMpc):
        def __init__(self, *a, **kw):
            built.update(kw)
            self._cost_on_safety, self._cost, self._n_perf = False, None, 0

        def set_env(self, env, objective_hook=None):
            pass

    import safe_exploration_amd.safempc_cem as sc
    monkeypatch.setattr(sc, 'FusedCemMpc', Spy)
    monkeypatch.setattr(CemSafeMPC, '_build_env', lambda self: (_env(), False))
    on = _safempc_with(conf(cem_obstacle_constraint=True, cem_ctrl_ellipsoid_constraint=True), obs)
    on._solver()
    assert built.get('con_set') is on._con_set
    built.clear()
    _safempc_with(conf(), obs)._solver()
    assert 'con_set' not in built


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------------
def test_the_main_case_is_decided_and_mixed():
    """Pendulum, x0 = (0.02, -0.03), H = 5, 256 rows of std 0.5: control-violating rows per step 0 / 14 / 22 / 54 / 97, of
    those with the box satisfied 0 / 2 / 8 / 43 / 86, obstacle-violating rows per step 118 / 171 / 190 / 221 / 0, smallest |d|
    1.1e-3.  No particle is left out."""
    spec, con, x0, rows, r, s = co.main_case()
    ell_only = s.ell & ~s.box
    print('ellipsoid-violated rows per step', s.ell.sum(axis=0), 'with the box satisfied', ell_only.sum(axis=0),
          'box-violated', s.box.sum(axis=0), 'obstacle-violated', s.obs.sum(axis=0), 'smallest |d|', s.min_abs_d)
    assert s.min_abs_d >= co.MARGIN
    assert list(s.ell.sum(axis=0)) == [0, 14, 22, 54, 97] and list(ell_only.sum(axis=0)) == [0, 2, 8, 43, 86]
    for name, fires in (('box', s.box.any(axis=1)), ('ellipsoid with the box satisfied', ell_only.any(axis=1)),
                        ('obstacle', s.obs.any(axis=1))):
        assert fires.any() and not fires.all(), name
    assert not s.obs[:, -1].any() and not s.ell[:, 0].any()      # the terminal ellipsoid, and the step from a point
    assert np.array_equal(co.extra_cost(problems.oracle_problem(spec, ocem), con, r, rows), s.extra)
    assert (s.extra > 0).any() and (s.extra == 0).any()
    # the empty set adds nothing
    e = co.signals(problems.oracle_problem(spec, ocem), co.empty(2), r.traj_p, r.traj_q, rows)
    assert not e.extra.any() and e.min_abs_d == np.inf
    # cart-pole, H = 3: ellipsoid-only violations at the last step too
    cart = problems.cartpole(n_train=200)
    prob = problems.oracle_problem(cart, ocem)
    crows = 2.0 * np.random.default_rng(co.SEED).normal(size=(64, 3, 1))      # (the box is +-4)
    cr = ocem.rollout(prob, co.gp_of(cart), np.array([0.3, 0.0, 0.05, 0.0]), crows)
    cs = co.signals(prob, co.ConSet(np.zeros((0, 4)), np.zeros(0), True), cr.traj_p, cr.traj_q, crows)
    print('cart-pole: ellipsoid-violated with the box satisfied per step', (cs.ell & ~cs.box).sum(axis=0), 'smallest |d|',
          cs.min_abs_d)
    assert (cs.ell & ~cs.box)[:, -1].any() and cs.min_abs_d >= co.MARGIN


def test_the_step_cost_of_the_oracle_is_the_rollouts():
    """conset_oracle.step_cost summed over the steps is the parent's action cost plus the set's extra cost."""
    spec, con, x0, rows, r, s = co.main_case()
    prob = problems.oracle_problem(spec, ocem)
    total = np.zeros(len(rows))
    for t in range(co.H):
        q_start = None if t == 0 else r.traj_q[:, t - 1]
        total += co.step_cost(prob, con, rows[:, t], q_start, r.traj_p[:, t], r.traj_q[:, t], t + 1 < co.H)
    assert np.array_equal(total, ocem.ACTION_VIOLATION_COST * s.box.sum(axis=1) + s.extra)


def test_the_gpu_solve_inputs_are_decided():
    """In every iteration the last elite and the first non-elite differ by more than 1e-6 (or in their constraint cost,
    which is exact), as do the best two rows of the last iteration; no distance sits within 1e-6 of the boundary; the last
    iteration ends feasible; and the same solve without the set picks another elite set in every iteration.  (Elite gaps
    7.1e-3, 9.4e-4, 3.9e-4, 6.7e-5; smallest |d| 6.0e-5; 250 -> 127 of 256 rows violate.)"""
    spec, con, H, x0, init_std, noise, best, trace, plain_best, plain_trace = co.solve()
    gaps = co.elite_gaps(trace, co.K)
    cost, obj, idx, _ = trace[-1]
    order = ocem.rank(cost, obj, 2)
    best_two = abs(obj[order[0]] - obj[order[1]])
    print('elite gaps per iteration:', gaps, 'best two:', best_two, 'smallest |d|:', [t[3] for t in trace],
          'rows with a violation:', [int((t[0] > 0).sum()) for t in trace])
    assert all(g > co.GAP for g in gaps) and all(g > co.GAP for g in co.elite_gaps(plain_trace, co.K))
    assert cost[order[0]] != cost[order[1]] or best_two > co.GAP
    assert all(t[3] >= co.MARGIN for t in trace)
    assert best is not None and cost[order[0]] == 0
    differ = [set(a[2]) != set(b[2]) for a, b in zip(trace, plain_trace)]
    assert any(differ), 'the set never changes an elite set: the solve test would pass without the feature'
    assert any((t[0] > 0).any() for t in trace)
