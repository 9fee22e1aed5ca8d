"""CPU: the SafeMPC constraint set in static exploration, host side ("the constraint set") -- the inputs
of tests/test_gpu_static_conset.py are sound on the oracle's numbers alone (tests/static_conset_oracle.py: every distance at
least 1e-6 from the boundary, every elite set decided by a gap above 1e-6, every signal present, another answer with the set
than without); sx_cem_rollout_starts_cons is declared, exported and bound and checks its arguments before any device access;
StaticCemMpc(con_set=...) reaches the new entry from its fused solve and charges every step and the start through
sx_conset_eval from its step-by-step solve (a fake library in place of the launches); and CemSafeMPC builds the set of
static_solver from its two settings, which are off by default and independent of the dynamic solver's."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import static_conset_oracle as sco
import static_explore_oracle as seo
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cem_mpc import StaticCemMpc
from test_conset_host import _bad_sets, _fake, _rollout_entries, _safempc_with, _set
from test_perf_multi_host import _Ssm, conf
from test_static_explore_host import _env, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
ENTRY = 'sx_cem_rollout_starts_cons'


# ---- 1: the inputs of the GPU tests -----------------------------------------------------------------------------------------------
def test_the_main_case_is_decided_and_holds_every_signal():
    """Pendulum, 256 rows [x0 | 4 actions] from the solve's first distribution, the feedback bounds and the obstacle slab
    -0.6 <= d_theta <= 0.55: 13 starts violate the obstacle inside the safe polytope (1 outside both), 26 rows have a step that
    is ellipsoid-violated with the box satisfied, 231 an obstacle-violated ellipsoid, 13 are feasible; smallest |d| 8.4e-4."""
    spec, con, rows, res = sco.main_case()
    prob = problems.oracle_problem(spec, ocem)
    plain = seo.rollout(prob, sco.gp_of(spec), rows)
    s = res.signals
    inside = plain.start_cost == 0
    ell_only = (s.ell & ~s.box).any(axis=1)
    margin = sco.polytope_margin(prob, rows, res)
    print(f'starts obstacle-violated inside the safe polytope {int((res.start_obs & inside).sum())}, outside both '
          f'{int((res.start_obs & ~inside).sum())}; rows ellipsoid-violated with the box satisfied {int(ell_only.sum())}, '
          f'obstacle-violated {int(s.obs.any(axis=1).sum())}, feasible {int((res.con_cost == 0).sum())} of {len(rows)}; '
          f'smallest |d| {res.min_abs_d:.2e}, to the safe polytope {margin:.2e}')
    assert res.min_abs_d >= sco.MARGIN and margin >= sco.MARGIN
    assert (res.start_obs & inside).any() and (res.start_obs & ~inside).any() and not res.start_obs.all()
    assert ell_only.any() and not ell_only.all()
    assert s.obs.any(axis=1).any() and not s.obs.any(axis=1).all()
    assert (res.con_cost == 0).any()
    assert not s.obs[:, -1].any() and not s.ell[:, 0].any()        # the terminal ellipsoid, and the step from a point
    # the composition: the plain static rollout, the steps' signals, 10 per violating start -- 20 for a start outside both
    np.testing.assert_array_equal(res.con_cost, plain.con_cost + s.extra + ocem.STATE_VIOLATION_COST * res.start_obs)
    both = res.start_obs & ~inside
    assert np.all((plain.start_cost + ocem.STATE_VIOLATION_COST * res.start_obs)[both] == 20.0)
    extra, smallest, _, start_obs = sco.extra_of(prob, con, res.traj_p, res.traj_q, rows)
    np.testing.assert_array_equal(extra, res.extra)
    assert smallest == res.min_abs_d and np.array_equal(start_obs, res.start_obs)
    # the start test is the point's distance to the rows, NaN never a violation, and it is all that H = 1 sees of the rows
    d0 = sco.start_obstacle_distances(con, rows[:, :2])
    np.testing.assert_array_equal(d0, np.stack((rows[:, 0] - sco.OBSTACLE[0], -rows[:, 0] - sco.OBSTACLE[1]), axis=1))
    one = sco.rollout(prob, con, sco.gp_of(spec), rows[:, :3])
    np.testing.assert_array_equal(one.extra, ocem.STATE_VIOLATION_COST * res.start_obs)
    with np.errstate(invalid='ignore'):
        assert not (sco.start_obstacle_distances(con, np.full((1, 2), np.nan)) >= 0).any()
    # without the set it is the plain static oracle
    np.testing.assert_array_equal(sco.rollout(prob, None, sco.gp_of(spec), rows).con_cost, plain.con_cost)


def test_the_solve_is_decided_and_the_set_changes_its_answer():
    """3 restarts of 64 rows, 8 elites, 4 iterations: the first seed whose rankings, with and without the set, are all decided
    by a relative gap above 1e-6 (elite k against k + 1, and the first two rows), whose distances all keep 1e-6 from the
    boundary, and whose answer the set changes."""
    d = sco.solve()
    gap, margin, feasible, differ = sco.solve_conditions(d['per'], d['plain_per'], d['chosen'], d['plain_chosen'])
    moved = float(np.abs(d['per'][d['chosen']][0] - d['plain_per'][d['plain_chosen']][0]).max())
    print(f'seed {d["seed"]}: smallest elite gap {gap:.2e}, smallest |d| {margin:.2e}; with the set restart {d["chosen"]} '
          f'(feasible {[bool(p[2]) for p in d["per"]]}), without restart {d["plain_chosen"]}; best rows differ by {moved:.3f}')
    assert gap > sco.GAP and margin >= sco.MARGIN and feasible and differ
    assert any(p[2] for p in d['per']) and d['answer'] is not None
    # the plain half is static_explore_oracle's own solve
    answer, chosen, per = seo.find(problems.oracle_problem(d['spec'], ocem), sco.gp_of(d['spec']), d['noise'], sco.K,
                                   sco.START_MEAN, sco.START_STD, sco.INIT_STD)
    assert chosen == d['plain_chosen']
    for a, b in zip(per, d['plain_per']):
        np.testing.assert_array_equal(a[0], b[0])
    # the set's penalties reach the ranking: some iteration's costs differ from the plain solve's on the same rows
    assert any(set(t[0].tolist()) - {0.0, 3.0, 6.0, 9.0, 10.0, 12.0} for p in d['per'] for t in p[3])


# ---- 2: the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    assert re.search(r'\bint ' + ENTRY + r'\(', header) and ENTRY in _lib.SIGNATURES
    fn = getattr(_lib.lib(), ENTRY)
    ours, parent = _lib.SIGNATURES[ENTRY][1], _lib.SIGNATURES['sx_cem_rollout_starts'][1]
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == ours
    assert ours == parent[:2] + [ctypes.POINTER(_lib.SxConSet)] + parent[2:]
    decl = re.search(r'\bint ' + ENTRY + r'\((.*?)\);', header, re.S).group(1)
    assert len(decl.split(',')) == len(ours) == 16
    # one plan, one query: no form entry of its own
    assert 'sx_cem_rollout_starts_cons_form' not in header and 'sx_cem_rollout_starts_cons_form' not in _lib.SIGNATURES
    build = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'build.sh')).read()
    assert 'sx_stream_starts_cons.hip' in build
    assert os.path.exists(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'sx_stream_starts_cons.hip'))


def _call(cons='ok', *, model=(), env=(), no_model=False, no_env=False, E=2, P=4, H=5, mean=16, std=16, noise=16, rows=16, obj=16,
          con=16, status=16, entry=ENTRY):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    m, e = _model(*model), _env(*env)
    cons = _set(e.n_s) if isinstance(cons, str) else cons
    head = (None if no_model else ctypes.byref(m), None if no_env else ctypes.byref(e))
    if entry == ENTRY:
        head += (None if cons is None else ctypes.byref(cons),)
    return getattr(_lib.lib(), entry)(*head, E, P, H, p(mean), p(std), p(noise), p(rows), None, None, p(obj), p(con), p(status),
                                      None)


PARENT_CASES = [dict(no_model=True), dict(no_env=True), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None),
                dict(E=0), dict(P=0), dict(H=0), dict(P=-3), dict(mean=None), dict(std=None), dict(model=(2, 2)),
                dict(env=(4, 1)), dict(model=(2, 1, 0)), dict(model=(3, 2), env=(3, 2), rows=None),
                dict(model=(3, 2), env=(3, 2)), dict(env=(2, 1, 17)), dict(env=(2, 1, 0)), dict(model=(2, 1, 2000)),
                dict(model=(1, 1, 1000), env=(1, 1), H=600)]


def test_argument_errors_without_a_gpu():
    # the set: null, m_obs out of range, ctrl_ellipsoid out of range, a non-finite constant in a row in use
    assert _call(None) == ARG
    for what, bad in _bad_sets():
        assert _call(bad) == ARG, what
    # noise without mean / std, as the parent
    assert _call(mean=None) == ARG and _call(std=None) == ARG
    # garbage in the rows NOT in use is not read
    unused = _set(m_obs=1)
    unused.h_mat_obs[2], unused.h_obs[1] = float('nan'), float('inf')
    assert _call(unused, rows=None) == ARG and _call(unused, model=(2, 1, 2000)) == UNSUPPORTED
    # the parent's own checks come first and its answers are this entry's, SX_ERR_UNSUPPORTED included: before any launch
    for kw in PARENT_CASES:
        want = _call(entry='sx_cem_rollout_starts', **kw)
        assert want in (ARG, UNSUPPORTED) and _call(**kw) == want, kw
    # a bad set on a model without a form is the argument's error: it is checked before the plan
    assert _call(_bad_sets()[0][1], model=(2, 1, 2000)) == ARG and _call(None, model=(3, 2), env=(3, 2)) == ARG
    # one plan for both entries: wherever the form query has no form, both entries answer SX_ERR_UNSUPPORTED
    for n_train in (20, 500, 900, 1100, 2000):
        m = _model(2, 1, n_train)
        has_form = int(_lib.lib().sx_cem_rollout_starts_form(ctypes.byref(m), 5)) >= 0
        if not has_form:
            assert _call(model=(2, 1, n_train)) == UNSUPPORTED == _call(model=(2, 1, n_train), entry='sx_cem_rollout_starts')


# ---- 3: StaticCemMpc(con_set=...) over the fake library -----------------------------------------------------------------------------
def _solver(ssm=None, E=2, P=32, H=4, k=4, iters=3, **kw):
    return StaticCemMpc(ssm or _Ssm(), _env(), H, P, k, iters, start_mean=[0.5, -0.5], start_std=[0.25, 0.125], n_restarts=E,
                        init_std=0.2, device='cpu', **kw)


def test_the_fused_solve_reaches_the_new_entry_only(monkeypatch):
    fake = _fake(monkeypatch)
    E, P, H, iters = 2, 32, 4, 3
    cons = _set()
    mpc = _solver(con_set=cons, E=E, P=P, H=H, iters=iters)
    mpc.solve()
    assert _rollout_entries(fake) == {ENTRY: iters}
    for args in fake.args[ENTRY]:
        assert len(args) == 16 and args[3:6] == (E, P, H)
        got = ctypes.cast(args[2], ctypes.POINTER(_lib.SxConSet)).contents
        assert (got.m_obs, got.ctrl_ellipsoid) == (2, 1) and bytes(got) == bytes(cons)
    assert 'sx_conset_eval' not in fake.calls and 'sx_onestep_reach' not in fake.calls
    # the solver's copy of env has the variance objective, as without the set
    assert ctypes.cast(fake.args[ENTRY][0][1], ctypes.POINTER(_lib.SxEnv)).contents.obj_mode == _lib.SX_OBJ_NEG_VARIANCE
    # without a set the same solver calls what it called before
    fake.calls.clear()
    _solver(E=E, P=P, H=H, iters=iters).solve()
    assert _rollout_entries(fake) == {'sx_cem_rollout_starts': iters}
    # the wrapper alone
    rows = torch.zeros((1, 4, 2 + H), dtype=torch.float64)
    fake.calls.clear()
    cem_mpc.cem_rollout_starts(_Ssm(), _env(), H, rows=rows, con_set=cons)
    cem_mpc.cem_rollout_starts(_Ssm(), _env(), H, rows=rows)
    assert _rollout_entries(fake) == {ENTRY: 1, 'sx_cem_rollout_starts': 1}


def test_the_stepwise_solve_charges_every_step_and_the_start_through_the_eval(monkeypatch):
    """Per iteration and restart: H sx_conset_eval calls for the steps (the obstacle rows on every step but the last, q_start
    NULL at the first step only), then one for the starts (points: q_start NULL, the obstacle rows checked); no rollout entry."""
    fake = _fake(monkeypatch)
    E, P, H, iters = 2, 32, 4, 2
    ssm = _Ssm(20)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    ssm.predict_without_jacobians = lambda x, u: (zeros(x.size(0), 2), zeros(x.size(0), 2))
    ssm.predict_with_jacobians = lambda x, u: (zeros(x.size(0), 2), zeros(x.size(0), 2), zeros(x.size(0), 2, 3))
    mpc = _solver(ssm, con_set=_set(), E=E, P=P, H=H, iters=iters)
    mpc.solve(stepwise=True)
    assert _rollout_entries(fake) == {}
    assert fake.calls['sx_onestep_reach'] == iters * E * H and fake.calls['sx_conset_eval'] == iters * E * (H + 1)
    calls = fake.args['sx_conset_eval']
    assert [c[7] for c in calls] == ([1] * (H - 1) + [0] + [1]) * (iters * E)
    assert [c[4] is None for c in calls] == ([True] + [False] * (H - 1) + [True]) * (iters * E)
    assert all(c[2] == P for c in calls)
    # the start charge sits beside the safe-polytope charge of the start: one more sx_polytope_distance per restart
    terminal_only = _env().con_mode != _lib.SX_CON_ALL_STATES
    assert fake.calls['sx_polytope_distance'] == iters * E * ((1 if terminal_only else H) + 1)
    # without a set: the box test in torch and no eval, as before
    fake.calls.clear()
    _solver(ssm, E=E, P=P, H=H, iters=iters).solve(stepwise=True)
    assert 'sx_conset_eval' not in fake.calls and fake.calls['sx_onestep_reach'] == iters * E * H


def test_the_solver_and_the_wrapper_refuse_what_is_not_built(monkeypatch):
    _fake(monkeypatch)
    with pytest.raises(TypeError, match='SxConSet'):
        _solver(con_set=dict(m_obs=0))
    for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
        with pytest.raises(NotImplementedError, match='con_set.*exact RBF GPs'):
            _solver(_Ssm(family=family), con_set=_set())
    rows = torch.zeros((1, 4, 6), dtype=torch.float64)
    with pytest.raises(TypeError, match='SxConSet'):
        cem_mpc.cem_rollout_starts(_Ssm(), _env(), 4, rows=rows, con_set='set')
    with pytest.raises(NotImplementedError, match='exact RBF GPs'):
        cem_mpc.cem_rollout_starts(_Ssm(family='feature'), _env(), 4, rows=rows, con_set=_set())


# ---- 4: CemSafeMPC ------------------------------------------------------------------------------------------------------------------
OBS = {'h_mat_obs': np.array([[1.0, 0.0], [-1.0, 0.0]]), 'h_obs': np.array([[0.7], [0.6]])}


def _spy(monkeypatch):
    import safe_exploration_amd.safempc_cem as sc
    built = []

    class Spy:
        def __init__(self, *a, **kw):
            built.append((a, kw))

    monkeypatch.setattr(sc, 'StaticCemMpc', Spy)
    monkeypatch.setattr(sc.CemSafeMPC, '_build_env', lambda self: (_env(), False))
    return built


def test_the_static_settings_build_the_set_of_static_solver(monkeypatch):
    built = _spy(monkeypatch)
    for kw, want in ((dict(cem_static_ctrl_ellipsoid_constraint=True), (0, 1)),
                     (dict(cem_static_obstacle_constraint=True), (2, 0)),
                     (dict(cem_static_ctrl_ellipsoid_constraint=True, cem_static_obstacle_constraint=True), (2, 1))):
        s = _safempc_with(conf(**kw), OBS)
        assert s._con_set is None                        # the dynamic solver's set is not theirs
        s.static_solver(3, np.zeros(2), np.ones(2))
        con = built[-1][1]['con_set']
        assert isinstance(con, _lib.SxConSet) and (con.m_obs, con.ctrl_ellipsoid) == want
        if want[0]:
            assert list(con.h_mat_obs)[:4] == [1.0, 0.0, -1.0, 0.0] and list(con.h_obs)[:2] == [0.7, 0.6]
    # None means no rows, as for the dynamic settings
    for extra in (None, {'h_mat_obs': None, 'h_obs': None}):
        _safempc_with(conf(cem_static_obstacle_constraint=True), extra).static_solver(3, np.zeros(2), np.ones(2))
        con = built[-1][1]['con_set']
        assert (con.m_obs, con.ctrl_ellipsoid) == (0, 0)
    # independent of the dynamic settings: both on gives each solver its own set
    s = _safempc_with(conf(cem_ctrl_ellipsoid_constraint=True, cem_static_obstacle_constraint=True), OBS)
    s.static_solver(3, np.zeros(2), np.ones(2))
    assert (s._con_set.m_obs, s._con_set.ctrl_ellipsoid) == (0, 1)
    assert (built[-1][1]['con_set'].m_obs, built[-1][1]['con_set'].ctrl_ellipsoid) == (2, 0)


def test_static_solver_is_built_as_before_without_the_settings(monkeypatch):
    built = _spy(monkeypatch)
    s = _safempc_with(conf(cem_seed=4, cem_init_std=0.3), OBS)
    s.static_solver(3, np.zeros(2), np.ones(2))
    (a, kw), = built
    assert a[2:] == (5, 64, 8, 3) and a[0] is s._ssm
    assert sorted(kw) == ['device', 'init_std', 'n_restarts', 'record_rollouts', 'seed', 'start_mean', 'start_std']
    assert kw['n_restarts'] == 3 and kw['seed'] == 4 and kw['init_std'] == 0.3 and kw['record_rollouts'] is False


def test_the_refusals_of_static_solver(monkeypatch):
    _spy(monkeypatch)
    # the dynamic set without a static setting still refuses, with the message it had
    for kw, name in ((dict(cem_ctrl_ellipsoid_constraint=True), 'cem_ctrl_ellipsoid_constraint'),
                     (dict(cem_obstacle_constraint=True), 'cem_obstacle_constraint')):
        with pytest.raises(NotImplementedError, match='static exploration is not built for ' + name):
            _safempc_with(conf(**kw), OBS).static_solver(2, np.zeros(2), np.ones(2))
    # a model the set is not built for refuses at static_solver, naming the setting; construction itself succeeds
    for kw, name in ((dict(cem_static_ctrl_ellipsoid_constraint=True), 'cem_static_ctrl_ellipsoid_constraint'),
                     (dict(cem_static_obstacle_constraint=True), 'cem_static_obstacle_constraint')):
        for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
            s = _safempc_with(conf(**kw), OBS, family=family)
            with pytest.raises(NotImplementedError, match=name + '.*exact RBF GP'):
                s.static_solver(2, np.zeros(2), np.ones(2))
