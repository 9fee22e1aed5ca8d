"""CPU: the saturating cost on the safety trajectory, host side -- the five entries are declared with the parents' argument
lists plus the cost, answer every argument error before any device access and report their form without one; over a fake
library a FusedCemMpc(cost_on_safety=True) solve reaches sx_cem_rollout_sat / sx_cem_rollout_elites_sat and nothing else,
never evaluates a hook and records no trajectory; the flag and equal-cost rules of FusedCemMpc, MultiModelCemMpc and
CemSafeMPC; and the inputs of the GPU solve tests (tests/test_gpu_safety_sat.py) are decided: in the numpy oracle's solves
(tests/safety_sat_oracle.py) every elite set and the best row hold by more than 1e-6."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import safety_sat_oracle as sso
import sat_cost_oracle as so
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc, MultiModelPerfCemMpc
from safe_exploration_amd.costs import SaturatingCost
from safe_exploration_amd.safempc_cem import CemSafeMPC, multi_solve_applies
from test_perf_multi_host import ABS, FakeLib, _env, _model, _models, _safempc, _Ssm, conf
from test_sat_cost_host import COST2, _bad_costs, _cost, _hook, p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
ENTRIES = {'sx_cem_rollout_sat': 'sx_cem_rollout', 'sx_cem_rollout_elites_sat': 'sx_cem_rollout_elites',
           'sx_cem_rollout_sat_multi': 'sx_cem_rollout_multi', 'sx_cem_rollout_elites_sat_multi': 'sx_cem_rollout_elites_multi'}


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_with_the_parents_arguments_plus_the_cost():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name, parent in ENTRIES.items():
        assert re.search(r'\bint ' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        ours, theirs = _lib.SIGNATURES[name][1], _lib.SIGNATURES[parent][1]
        # (sx_cem_rollout_sat takes no workspace: two arguments fewer)
        assert len(ours) == len(theirs) + 1 - (2 if name == 'sx_cem_rollout_sat' else 0)
        at = 3 if name.endswith('_multi') else 2
        assert ours[at] == ctypes.POINTER(_lib.SxSatCost) and ours[:at] == theirs[:at]
        # the header's argument count is the mirror's
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        assert len(decl.split(',')) == len(ours)
    assert re.search(r'\bint sx_cem_rollout_sat_form\(', header) and 'sx_cem_rollout_sat_form' in _lib.SIGNATURES
    assert hasattr(_lib.lib(), 'sx_cem_rollout_sat_form')


# ---- argument errors, before any device access ---------------------------------------------------------------------------------
def _call(cost, *, multi=False, elites=False, model=None, models=None, env=None, table=16, E=2, P=4, H=5, x0=16, mean=16,
          std=16, noise=16, actions=16, obj=16, con=16, status=16, rows=16, k=3, mean_out=None, std_out=None):
    env = env if env is not None else _env()
    if multi:
        ms = models if models is not None else [model or _model(), model or _model(n_train=70)]
        head = (None if ms == 'null' else _models(*ms), p(table), ctypes.byref(env))
    else:
        head = (None if model == 'null' else ctypes.byref(model or _model()), ctypes.byref(env))
    head += (None if cost is None else ctypes.byref(cost),)
    entry = 'sx_cem_rollout' + ('_elites' if elites else '') + '_sat' + ('_multi' if multi else '')
    dist = (p(rows), k) if elites else (p(mean), p(std))
    tail = (p(mean_out), p(std_out)) if elites else ()
    return getattr(_lib.lib(), entry)(*head, E, P, H, p(x0), None, *dist, p(noise), p(actions), None, None, p(obj), p(con),
                                      p(status), *tail, None)


@pytest.mark.parametrize('elites', [False, True])
@pytest.mark.parametrize('multi', [False, True])
def test_argument_errors_without_a_gpu(multi, elites):
    ok = _cost()
    call = lambda cost=ok, **kw: _call(cost, multi=multi, elites=elites, **kw)
    # the cost: null or invalid
    assert call(None) == ARG
    for what, bad in _bad_costs():
        assert call(bad) == ARG, what
    # what the parents answer SX_ERR_ARG for
    for kw in (dict(x0=None), dict(actions=None), dict(obj=None), dict(con=None), dict(status=None), dict(E=0), dict(P=0),
               dict(H=0), dict(model=_model(2, 2))):
        assert call(**kw) == ARG, kw
    if elites:
        for kw in (dict(rows=None), dict(noise=None), dict(k=0), dict(mean_out=16), dict(std_out=16)):
            assert call(**kw) == ARG, kw
    else:
        assert call(mean=None) == ARG and call(std=None) == ARG
    if multi:
        assert call(table=None) == ARG and call(models='null') == ARG
        assert call(models=[_model(), _model(2, 2)]) == ARG and call(models=[_model(), _model(n_train=0)]) == ARG
    else:
        assert call(model='null') == ARG
    # SX_ERR_UNSUPPORTED, before any launch: m beyond SX_MAX_M, a shape without a kernel, the workspace path / neither form
    many = _env()
    many.m = _lib.SX_MAX_M + 1
    assert call(env=many) == UNSUPPORTED
    assert call(_cost(3, 0, 1), model=_model(3, 2), env=_env(3, 2)) == UNSUPPORTED
    assert call(model=_model(n_train=1100)) == UNSUPPORTED
    assert call(_cost(1, 0, 1), model=_model(1, 1, n_train=1000), env=_env(1, 1), H=600) == UNSUPPORTED
    if elites:
        # beyond the parents' 2 H n_u <= 256 (1 + n_s)
        assert call(H=385) == UNSUPPORTED
    # a bad cost on a model without a form is the cost's error: it is checked before the plan
    assert call(_cost(rank=0), model=_model(n_train=1100)) == ARG
    # env->obj_mode is not read, not even to reject an odd value
    odd = _env()
    odd.obj_mode = 7
    assert call(env=odd, model=_model(n_train=1100)) == UNSUPPORTED and call(env=odd, x0=None) == ARG


def test_the_form_query():
    lib = _lib.lib()
    form = lambda m, H=5: int(lib.sx_cem_rollout_sat_form(None if m is None else ctypes.byref(m), H))
    assert form(_model(n_train=7)) == form(_model(n_train=200)) == SX_FORM_STREAM and form(_model(n_train=590)) == SX_FORM_BYOUT
    assert form(None) < 0 and form(_model(), 0) < 0
    assert form(_model(n_train=1100)) < 0                                  # the workspace path is not served
    assert form(_model(3, 2)) < 0                                          # a shape without a kernel
    assert form(_model(1, 1, n_train=1000), 600) < 0                       # fits neither form
    # the streaming kernel only, as sx_cem_rollout_starts_form: a model whose parent takes a resident form reports STREAM
    for m in (_model(n_train=7), _model(n_train=200), _model(4, 1, n_train=200), _model(n_train=590)):
        assert form(m) == int(lib.sx_cem_rollout_starts_form(ctypes.byref(m), 5))


# ---- the plumbing over a fake library --------------------------------------------------------------------------------------------
class _Lib(FakeLib):
    """FakeLib whose ranking query also answers for real (so that the prologue refit applies as on the device)."""
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


def test_a_cost_on_safety_solve_reaches_the_sat_entries_only(monkeypatch):
    fake = _fake(monkeypatch)
    iters, P, H = 3, 4096, 4       # (4096 candidates: the counting ranking, whose refit moves into the rollout's prologue)
    ssm = _Ssm(200)
    ssm.workspace = lambda nbytes: None        # (what the parent entry's wrapper asks the model for; the _sat entry has none)
    mpc = FusedCemMpc(ssm, _env(), H, P, 8, iters, device='cpu', init_std=0.2, cost_on_safety=True)
    assert mpc._refit_in_prologue(1)
    mpc.set_env(_env(), objective_hook=_hook)                  # a raising hook: never evaluated
    mpc.set_cost(COST2)
    mpc.solve(torch.zeros((1, 2), dtype=torch.float64))
    assert _rollout_entries(fake) == {'sx_cem_rollout_sat': 1, 'sx_cem_rollout_elites_sat': iters - 1}
    first = fake.args['sx_cem_rollout_sat'][0]
    assert len(first) == 18 and first[3:6] == (1, P, H)
    assert ctypes.cast(first[2], ctypes.POINTER(_lib.SxSatCost)).contents.rank == COST2.rank
    assert first[12] is None and first[13] is None             # no traj, no sigma
    for args in fake.args['sx_cem_rollout_elites_sat']:
        assert len(args) == 20 and args[3:6] == (1, P, H) and args[9] == 8 and args[12] is None
    # where the prologue does not apply (the ranking launch refits): the plain sat entry every iteration
    fake.calls.clear()
    with monkeypatch.context() as m:
        m.setattr(cem_mpc, 'fused_refit_applies', lambda *a, **kw: False)
        mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    assert _rollout_entries(fake) == {'sx_cem_rollout_sat': iters}
    # without a cost the same solver is the parent's: the parent entries, and the hook on the recorded trajectory
    fake.calls.clear()
    mpc.set_cost(None)
    with pytest.raises(AssertionError, match='hook was evaluated'):
        mpc.solve(torch.zeros((1, 2), dtype=torch.float64))
    assert _rollout_entries(fake) == {'sx_cem_rollout': 1} and fake.args['sx_cem_rollout'][-1][11] is not None


def test_the_stepwise_path_prices_every_step_with_the_cost(monkeypatch):
    """solve(stepwise=True), what the NAN | ZERO_FIX repeat runs: one sx_sat_cost_eval per step, no hook, no rollout entry."""
    fake = _fake(monkeypatch)
    iters, P, H = 2, 32, 4
    ssm = _Ssm(20)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    ssm.predict_without_jacobians = lambda x, u: (zeros(x.size(0), 2), zeros(x.size(0), 2))
    ssm.predict_with_jacobians = lambda x, u: (zeros(x.size(0), 2), zeros(x.size(0), 2), zeros(x.size(0), 2, 3))
    mpc = FusedCemMpc(ssm, _env(), H, P, 8, iters, device='cpu', init_std=0.2, cost_on_safety=True)
    mpc.set_env(_env(), objective_hook=_hook)
    mpc.set_cost(COST2)
    mpc.solve(torch.zeros((1, 2), dtype=torch.float64), stepwise=True)
    assert _rollout_entries(fake) == {} and fake.calls['sx_sat_cost_eval'] == iters * H
    assert fake.calls['sx_onestep_reach'] == iters * H
    with pytest.raises(TypeError, match='SaturatingCost'):
        cem_mpc.cem_rollout_stepwise(ssm, _env(), zeros(2), zeros(P, H, 1), status=torch.zeros(1, dtype=torch.int32),
                                     cost=lambda m, v: 0.0)


def test_the_wrappers_take_exact_gps_only(monkeypatch):
    _fake(monkeypatch)
    x0, noise = torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1, 4, 3, 1), dtype=torch.float64)
    mean = torch.zeros((1, 3, 1), dtype=torch.float64)
    for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
        with pytest.raises(NotImplementedError, match='exact RBF GPs'):
            cem_mpc.cem_rollout(_Ssm(family=family), _env(), x0, 3, mean=mean, std=mean, noise=noise, cost=COST2)
        with pytest.raises(NotImplementedError, match='exact RBF GPs'):
            cem_mpc.cem_rollout_multi([_Ssm(family=family)], _env(), x0, 3, mean=mean, std=mean, noise=noise, cost=COST2)
        with pytest.raises(NotImplementedError, match='exact RBF GPs'):
            FusedCemMpc(_Ssm(family=family), _env(), 3, 32, 8, 2, device='cpu', cost_on_safety=True).set_cost(COST2)
    with pytest.raises(TypeError, match='SaturatingCost'):
        cem_mpc.cem_rollout(_Ssm(), _env(), x0, 3, mean=mean, std=mean, noise=noise, cost='cost')
    with pytest.raises(ValueError, match='n_s = 4'):
        cem_mpc.cem_rollout(_Ssm(), _env(), x0, 3, mean=mean, std=mean, noise=noise,
                            cost=SaturatingCost(so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, 2))


# ---- the flag and cost rules -------------------------------------------------------------------------------------------------------
def test_the_flag_rules_of_the_fused_solver():
    mk = lambda **kw: FusedCemMpc(_Ssm(), _env(), 4, 32, 8, 2, device='cpu', **kw)
    # without the flag today's refusal stands
    for kw in (dict(), dict(n_perf=6), dict(n_perf=6, perf_variance=True)):
        with pytest.raises(ValueError, match="cem_perf_type='taylor'"):
            mk(**kw).set_cost(COST2)
    # with the flag the cost belongs to the safety trajectory: no performance trajectory beside it
    for kw in (dict(n_perf=6), dict(n_perf=6, perf_type='taylor')):
        with pytest.raises(ValueError, match='cost_on_safety'):
            mk(cost_on_safety=True, **kw)
    mpc = mk(cost_on_safety=True)
    assert mpc._safety_cost is None
    mpc.set_cost(COST2)
    assert mpc._cost is COST2 and mpc._safety_cost is COST2
    with pytest.raises(TypeError, match='SaturatingCost'):
        mpc.set_cost(lambda m, v: 0.0)
    with pytest.raises(ValueError, match='n_s = 4'):
        mpc.set_cost(SaturatingCost(so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, 2))
    mpc.set_cost(None)
    assert mpc._safety_cost is None
    # a Taylor solver's cost is not a safety cost
    taylor = mk(n_perf=6, perf_type='taylor')
    taylor.set_cost(COST2)
    assert taylor._safety_cost is None


def test_multi_model_solve_needs_equal_costs(monkeypatch):
    fake = _fake(monkeypatch)
    iters, P, H = 2, 32, 4
    mk = lambda e, **kw: FusedCemMpc(_Ssm(20 + 10 * e), _env(), H, P, 8, iters, device='cpu', init_std=0.2, seed=e, **kw)
    solvers = [mk(e, cost_on_safety=True) for e in range(3)]
    for s in solvers:
        s.set_cost(SaturatingCost(COST2.target, COST2.weight, 0))       # equal, not identical
    mpc = MultiModelCemMpc.from_solvers(solvers)
    mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    assert solvers[0]._refit_in_prologue(3)      # (the elite-row form from the second iteration on)
    assert _rollout_entries(fake) == {'sx_cem_rollout_sat_multi': 1, 'sx_cem_rollout_elites_sat_multi': iters - 1}
    assert len(fake.args['sx_cem_rollout_elites_sat_multi'][0]) == 21
    args = fake.args['sx_cem_rollout_sat_multi'][0]
    assert len(args) == 19 and args[4:7] == (3, P, H)
    solvers[1].set_cost(None)
    with pytest.raises(ValueError, match='equal costs'):
        mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match='equal costs'):
        mpc.get_actions_multi(torch.zeros((3, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match='equal costs'):
        MultiModelCemMpc.from_solvers(solvers)
    solvers[1].set_cost(SaturatingCost(COST2.target, 2 * COST2.weight, 0))
    with pytest.raises(ValueError, match='equal costs'):
        mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    fake.calls.clear()
    mpc.set_cost(None)
    mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    assert _rollout_entries(fake) == {'sx_cem_rollout_multi': 1, 'sx_cem_rollout_elites_multi': iters - 1}
    # check_solvers compares the flag
    with pytest.raises(ValueError, match='CEM settings'):
        MultiModelCemMpc.check_solvers([mk(0, cost_on_safety=True), mk(1)])
    MultiModelCemMpc.check_solvers([mk(0, cost_on_safety=True), mk(1, cost_on_safety=True)])
    # the performance solve keeps its rule and its launches: the cost there belongs to the performance trajectory
    assert MultiModelPerfCemMpc.set_cost is MultiModelCemMpc.set_cost
    # solvers with a hook go through the multi-model solve where a safety cost stands in for it
    hooked = [mk(e, cost_on_safety=True) for e in range(2)]
    for s in hooked:
        s.set_env(_env(), objective_hook=_hook)
    assert not multi_solve_applies(hooked)
    for s in hooked:
        s.set_cost(COST2)
    assert multi_solve_applies(hooked)


class _Mpc:
    def __init__(self):
        self.costs = []

    def set_cost(self, cost):
        self.costs.append(cost)


def test_init_solver_with_and_without_cem_cost_on_safety(monkeypatch):
    # objects built by __new__ may lack the setting: it reads as off
    solver = CemSafeMPC.__new__(CemSafeMPC)
    solver._mpc, solver._cost, solver._perf = _Mpc(), None, cem_mpc.PerfSpec(0, type='mean_equivalent')
    with pytest.raises(ValueError, match="cem_perf_type='taylor'"):
        solver.init_solver(COST2)
    solver._cem_cost_on_safety = True
    solver.init_solver(lambda *a: 0.0)                                  # any other value changes nothing
    assert solver._mpc.costs == [] and solver._cost is None
    solver.init_solver(COST2)
    assert solver._mpc.costs == [COST2] and solver._cost is COST2
    # through the constructor: the conf setting, off by default, refused beside a performance trajectory
    assert _safempc(conf())._cem_cost_on_safety is False
    with pytest.raises(ValueError, match="cem_perf_type='taylor'"):
        _safempc(conf()).init_solver(COST2)
    with pytest.raises(ValueError, match='cem_cost_on_safety'):
        _safempc(conf(cem_cost_on_safety=True, cem_n_perf=6))
    on = _safempc(conf(cem_cost_on_safety=True))
    assert on._cem_cost_on_safety is True
    on.init_solver(COST2)
    assert on._cost is COST2
    # ... and the optimiser it builds carries the flag and the cost
    built = {}

    class Spy(FusedCemMpc):
        def __init__(self, *a, **kw):
            built.update(kw)
            self._cost_on_safety, self._cost, self._n_perf = kw.get('cost_on_safety', False), None, 0
            self._ssm, self._objective_hook = _Ssm(), None

        def set_env(self, env, objective_hook=None):
            pass

    import safe_exploration_amd.safempc_cem as sc
    monkeypatch.setattr(sc, 'FusedCemMpc', Spy)
    monkeypatch.setattr(CemSafeMPC, '_build_env', lambda self: (_env(), False))
    mpc = on._solver()
    assert built.get('cost_on_safety') is True and mpc._cost is COST2 and mpc._safety_cost is COST2
    off = _safempc(conf())
    built.clear()
    off._solver()
    assert 'cost_on_safety' not in built


# ---- the inputs of the GPU solve tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(sso.SOLVES))
def test_the_gpu_solve_inputs_are_decided(name):
    """In every iteration the last elite and the first non-elite differ by more than 1e-6 (or in their constraint cost,
    which is exact), as do the best two rows of the last iteration; the last iteration ends feasible and some constraint
    is active.  (cart-pole: smallest elite gap 2.0e-6, best two 9.3e-5, 252 -> 230 of 256 rows violate; pendulum: 2.0e-4,
    4.0e-4, 248 -> 48.)"""
    spec, cost, H, x0, init_std, noise, best, trace = sso.solve(name)
    assert noise.shape == (sso.ITERS, sso.P, H, spec.n_u) and len(trace) == sso.ITERS
    assert best is not None, 'the oracle\'s last iteration does not end feasible'
    gaps = so.elite_gaps(trace, sso.K)
    con, obj, idx = trace[-1]
    order = ocem.rank(con, obj, 2)
    best_two = abs(obj[order[0]] - obj[order[1]])
    print(name, 'elite gaps per iteration:', gaps, 'best two:', best_two, 'rows with a violation:',
          [int((c > 0).sum()) for c, _, _ in trace])
    assert all(g > sso.GAP for g in gaps)
    assert con[order[0]] != con[order[1]] or best_two > sso.GAP
    for con, obj, idx in trace:
        assert np.isfinite(obj).all() and (obj > 0).all() and (obj < H).all()
    assert any((con > 0).any() for con, _, _ in trace), 'no constraint is ever active'


def test_the_oracle_objective_is_the_loss_of_every_safety_ellipsoid():
    """safety_cost sums sat_cost_oracle.loss over (traj_p, traj_q) of oracle.cem.rollout: spelled out for three particles."""
    spec, cost, H, x0, init_std, noise, _, trace = sso.solve('pendulum')
    from safe_exploration_amd import problems
    rows = init_std * noise[0, :3]
    r = ocem.rollout(problems.oracle_problem(spec, ocem), sso.gp_of(spec), x0, rows)
    want = [sum(so.loss(cost, r.traj_p[i, t], r.traj_q[i, t]) for t in range(H)) for i in range(3)]
    assert np.array_equal(sso.safety_cost(cost, r), np.array(want))
    assert np.abs(trace[0][1][:3] - np.array(want)).max() <= 1e-12      # (the GP's products in a batch of 256 against 3)
    assert np.abs(r.traj_q - np.swapaxes(r.traj_q, -1, -2)).max() <= 1e-15 * np.abs(r.traj_q).max()
