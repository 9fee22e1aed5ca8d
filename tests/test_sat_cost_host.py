"""CPU: the saturating cost, host side -- the numpy oracle (tests/sat_cost_oracle.py) against sampling, the symmetric V-form
against the inverse / determinant form, costs.SaturatingCost (refusals, struct contents, __call__ against the oracle), the
layout of sx_sat_cost, the argument checks of the four entries before any device access, the plumbing from init_solver to the
_sat entries over a fake library, and the inputs of the GPU solve tests (tests/test_gpu_sat_cost.py): the oracle's elite sets
are decided by more than 1e-6 in every iteration."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import sat_cost_oracle as so
from oracle import cem as ocem
from oracle.gp import ExactGP
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cem_mpc import CautiousCemMpc, FusedCemMpc, MultiModelPerfCemMpc
from safe_exploration_amd.costs import SaturatingCost
from test_perf_multi_host import ABS, _env, _fake_device, _model, _models, _Ssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
CARTPOLE = so.Cost(so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, so.CARTPOLE_TRIG_IDX)


def random_spd(rng, n, scale):
    root = rng.normal(size=(n, n))
    return scale * (root @ root.T + 0.1 * np.eye(n))


def random_weight(rng, n, rank):
    root = rng.normal(size=(n, rank))
    return root @ root.T


# ---- the oracle against sampling -------------------------------------------------------------------------------------------
SAMPLED = [  # (n_s, trig_idx, target, weight)
    (2, 0, np.array([0.3, 0.2, 0.9]), np.diag([0.5, 1.0, 2.0])),
    (2, 1, np.array([-0.2, 0.1, 0.8]), random_weight(np.random.default_rng(3), 3, 2)),
    (4, 2, so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT),
    (3, None, np.array([0.1, -0.3, 0.2]), random_weight(np.random.default_rng(4), 3, 3)),
]


@pytest.mark.parametrize('n_s,trig_idx,target,weight', SAMPLED, ids=['ns2-i0', 'ns2-i1', 'cartpole', 'no-angle'])
def test_oracle_against_sampling(n_s, trig_idx, target, weight):
    """Fixed seed, 4e5 draws: the augmented mean and covariance and E[1 - exp(-1/2 (x - z)^T W (x - z))] under the augmented
    Gaussian lie within 6 standard errors, computed from the sample itself."""
    rng = np.random.default_rng(100 + n_s + (trig_idx or 0))
    n = 400_000
    mu, cov = rng.normal(0, 0.7, size=n_s), random_spd(rng, n_s, 0.15)
    x = rng.multivariate_normal(mu, cov, size=n)
    if trig_idx is not None:
        keep = [j for j in range(n_s) if j != trig_idx]
        xa = np.concatenate((x[:, keep], np.sin(x[:, trig_idx:trig_idx + 1]), np.cos(x[:, trig_idx:trig_idx + 1])), axis=1)
    else:
        xa = x
    ma, sa = so.augment(mu, cov, trig_idx)
    se_mean = xa.std(axis=0, ddof=1) / np.sqrt(n)
    assert (np.abs(xa.mean(axis=0) - ma) <= 6 * se_mean).all()
    centred = xa - xa.mean(axis=0)
    prod = centred[:, :, None] * centred[:, None, :]
    se_cov = prod.std(axis=0, ddof=1) / np.sqrt(n)
    assert (np.abs(prod.mean(axis=0) * n / (n - 1) - sa) <= 6 * se_cov).all()
    # the loss is the expectation of the saturating cost under the Gaussian with the augmented moments
    g = rng.multivariate_normal(ma, sa, size=n, check_valid='ignore') - target
    val = 1.0 - np.exp(-0.5 * np.einsum('ni,ij,nj->n', g, weight, g))
    got = so.loss(so.Cost(target, weight, trig_idx), mu, cov)
    assert abs(val.mean() - got) <= 6 * val.std(ddof=1) / np.sqrt(n)
    assert 0.01 < got < 0.99


# ---- the V-form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rank', [2, 5])
def test_v_form_equals_the_inverse_determinant_form(rank):
    rng = np.random.default_rng(rank)
    weight = random_weight(rng, 5, rank) * 0.3
    assert np.abs(weight - np.diag(np.diag(weight))).max() > 0.01
    cost = so.Cost(rng.normal(0, 0.5, size=5), weight, 2)
    assert so.factor(weight).shape == (5, rank)
    for _ in range(50):
        mu, cov = rng.normal(0, 1.0, size=4), random_spd(rng, 4, rng.uniform(0.01, 1.0))
        assert abs(so.v_form(cost, mu, cov) - so.loss(cost, mu, cov)) <= 1e-13
    for _ in range(20):
        mu, cov = rng.normal(0, 0.3, size=4), random_spd(rng, 4, 0.05)
        assert abs(so.v_form(CARTPOLE, mu, cov) - so.loss(CARTPOLE, mu, cov)) <= 1e-13


# ---- SaturatingCost ------------------------------------------------------------------------------------------------------------
def test_saturating_cost_refusals():
    z, w = so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT
    asym = w.copy()
    asym[0, 4] = 0.1
    for args, word in (((z, asym, 2), 'symmetric'), ((z, -w, 2), 'positive semi-definite'),
                       ((z, np.diag([1.0, 0, 0, 0, -0.5]), 2), 'positive semi-definite'),
                       ((z, np.zeros((5, 5)), 2), 'positive semi-definite'), ((z[:4], w, 2), 'weight must be'),
                       ((z, w[:4, :4], 2), 'weight must be'), ((z, w, 4), 'trig_idx'), ((z, w, -1), 'trig_idx'),
                       ((z, w, 1.5), 'trig_idx'), ((z, w, None), 'n_s = 5'), ((np.zeros(6), np.eye(6), 0), 'n_s = 5'),
                       ((np.zeros((2, 2)), np.eye(2), None), 'vector'), ((np.array([0.0]), np.eye(1), 0), 'trig_idx'),
                       ((np.array([np.nan, 0]), np.eye(2), None), 'finite'), ((z, np.full((5, 5), np.inf), 2), 'finite')):
        with pytest.raises(ValueError, match=word):
            SaturatingCost(*args)


def test_saturating_cost_struct_contents():
    cost = SaturatingCost(so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, trig_idx=2)
    s = cost.struct
    assert (cost.n_s, cost.n_a, cost.rank, s.trig_idx, s.rank) == (4, 5, 2, 2, 2)
    assert list(s.target)[:5] == list(so.CARTPOLE_TARGET)
    v = np.array(list(s.v)[:10]).reshape(5, 2)
    assert np.abs(v @ v.T - so.CARTPOLE_WEIGHT).max() <= 1e-16 and not np.array(list(s.v)[10:]).any()
    rng = np.random.default_rng(0)
    w = random_weight(rng, 3, 3)
    full = SaturatingCost([0.1, 0.2, 0.3], w)
    assert (full.n_s, full.rank, full.struct.trig_idx) == (3, 3, -1)
    v = np.array(list(full.struct.v)[:9]).reshape(3, 3)
    assert np.abs(v @ v.T - w).max() <= 1e-14 * np.abs(w).max()
    # eigenvalues below 1e-12 of the largest are dropped
    w2 = random_weight(rng, 3, 2) + 1e-14 * np.eye(3)
    assert SaturatingCost([0.1, 0.2, 0.3], w2).rank == 2
    assert cost == SaturatingCost(so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, 2) and cost != full
    assert cost != SaturatingCost(so.CARTPOLE_TARGET, 2 * so.CARTPOLE_WEIGHT, 2)


@pytest.mark.parametrize('n_s,trig_idx,rank', [(2, 0, 1), (2, 1, 3), (2, None, 2), (4, 2, 5), (1, 0, 2), (3, None, 3)])
def test_call_against_the_oracle(n_s, trig_idx, rank):
    rng = np.random.default_rng(7 + n_s + rank)
    n_a = n_s + (trig_idx is not None)
    z, w = rng.normal(0, 0.5, size=n_a), random_weight(rng, n_a, rank) * 0.5
    cost = SaturatingCost(z, w, trig_idx)
    assert cost.rank == rank
    mu = rng.normal(0, 1.0, size=(3, 11, n_s))
    cov = np.stack([random_spd(rng, n_s, 0.2) for _ in range(33)]).reshape(3, 11, n_s, n_s)
    got = cost(torch.tensor(mu), torch.tensor(cov)).numpy()
    want = so.losses(so.Cost(z, w, trig_idx), mu, cov)
    assert got.shape == (3, 11) and np.abs(got - want).max() <= 1e-13
    with pytest.raises(ValueError, match='mu must be'):
        cost(torch.zeros(4, n_s + 1), torch.zeros(4, n_s + 1, n_s + 1))


# ---- the struct's layout -------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sx_amd.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(sx_sat_cost), offsetof(sx_sat_cost, trig_idx),'
                   'offsetof(sx_sat_cost, rank), offsetof(sx_sat_cost, target), offsetof(sx_sat_cost, v), SX_SAT_MAX_DIM);'
                   'return 0;}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    S = _lib.SxSatCost
    assert got == [ctypes.sizeof(S), S.trig_idx.offset, S.rank.offset, S.target.offset, S.v.offset, _lib.SX_SAT_MAX_DIM]
    assert _lib.SX_SAT_MAX_DIM == _lib.SX_MAX_NS + 1


# ---- the entries' argument checks, before any device access --------------------------------------------------------------------
def _cost(n_s=2, trig_idx=0, rank=1):
    n_a = n_s + (trig_idx >= 0)
    c = _lib.SxSatCost()
    c.trig_idx, c.rank = trig_idx, rank
    for i in range(n_a * min(max(rank, 0), n_a)):
        c.v[i] = 0.5
    return c


BAD_COSTS = [('trig_idx = n_s', dict(trig_idx=2)), ('trig_idx = -2', dict(trig_idx=-2)), ('rank = 0', dict(rank=0)),
             ('rank = n_a + 1', dict(rank=4)), ('rank = n_s + 1 without an angle', dict(trig_idx=-1, rank=3))]


def _bad_costs():
    out = [(what, _cost(**kw)) for what, kw in BAD_COSTS]
    for what, field, value in (('target NaN', 'target', float('nan')), ('v inf', 'v', float('inf'))):
        c = _cost()
        getattr(c, field)[0] = value
        out.append((what, c))
    return out


p = lambda v: None if v is None else ctypes.c_void_p(v)


def _eval(cost, n_s=2, P=4, mu=16, cov=16, loss=16, status=16):
    return _lib.lib().sx_sat_cost_eval(None if cost is None else ctypes.byref(cost), n_s, P, p(mu), p(cov), p(loss),
                                       p(status), None)


def _taylor(cost, *, multi=False, model=None, env=None, table=16, E=2, P=4, H=5, n_perf=8, r=1, x0=16, safe=16, mean=16,
            std=16, noise=16, rows=16, obj=16, con=16, status=16, terminal=0):
    ms = [model or _model(), model or _model()]
    env = env if env is not None else _env()
    head = ((_models(*ms), p(table)) if multi else (ctypes.byref(ms[0]),)) + (ctypes.byref(env),)
    entry = 'sx_cem_perf_rollout_taylor_sat' + ('_multi' if multi else '')
    return getattr(_lib.lib(), entry)(*head, None if cost is None else ctypes.byref(cost), E, P, H, n_perf, r, p(x0), p(safe),
                                      p(mean), p(std), p(noise), p(rows), p(obj), p(con), None, None, None, terminal,
                                      p(status), None)


def _cautious(cost, *, model=None, env=None, E=1, P=4, T=8, x0=16, mean=16, std=16, noise=16, rows=16, obj=16, con=16,
              status=16):
    model, env = model or _model(), env if env is not None else _env()
    return _lib.lib().sx_cem_cautious_rollout_sat(ctypes.byref(model), ctypes.byref(env),
                                                  None if cost is None else ctypes.byref(cost), E, P, T, p(x0), p(mean),
                                                  p(std), p(noise), p(rows), p(obj), p(con), None, None, None, None, 1,
                                                  p(status), None)


def test_entries_are_declared():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name in ('sx_sat_cost_eval', 'sx_cem_perf_rollout_taylor_sat', 'sx_cem_perf_rollout_taylor_sat_multi',
                 'sx_cem_cautious_rollout_sat'):
        assert 'int ' + name + '(' in header and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    # the parents' arguments plus the cost
    for parent in ('sx_cem_perf_rollout_taylor', 'sx_cem_cautious_rollout'):
        assert len(_lib.SIGNATURES[parent + '_sat'][1]) == len(_lib.SIGNATURES[parent][1]) + 1
    assert len(_lib.SIGNATURES['sx_cem_perf_rollout_taylor_sat_multi'][1]) == \
        len(_lib.SIGNATURES['sx_cem_perf_rollout_taylor_multi'][1]) + 1


def test_eval_argument_errors():
    ok = _cost()
    for kw in (dict(mu=None), dict(cov=None), dict(loss=None), dict(status=None), dict(P=0), dict(P=-1), dict(n_s=0),
               dict(n_s=5)):
        assert _eval(ok, **kw) == ARG, kw
    assert _eval(None) == ARG
    for what, bad in _bad_costs():
        assert _eval(bad) == ARG, what


@pytest.mark.parametrize('multi', [False, True])
def test_taylor_sat_argument_errors(multi):
    ok = _cost()
    call = lambda cost=ok, **kw: _taylor(cost, multi=multi, **kw)
    assert call(None) == ARG
    for what, bad in _bad_costs():
        assert call(bad) == ARG, what
    # what the parent refuses, with the parent's code
    for kw in (dict(x0=None), dict(safe=None), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None),
               dict(mean=None), dict(std=None), dict(E=0), dict(P=0), dict(H=0), dict(r=0), dict(r=6), dict(n_perf=3, r=3),
               dict(model=_model(n_train=0)), dict(model=_model(2, 2)), dict(terminal=1, n_perf=6)):
        assert call(**kw) == ARG, kw
    if multi:
        assert call(table=None) == ARG
    neg, many = _env(), _env()
    neg.m, many.m = -1, _lib.SX_MAX_M + 1
    assert call(env=neg) == ARG and call(env=many) == UNSUPPORTED
    assert call(model=_model(n_train=1100)) == UNSUPPORTED
    assert call(_cost(3, 0, 1), model=_model(3, 2), env=_env(3, 2)) == UNSUPPORTED      # a shape without a kernel
    # a bad cost on a model without a form is the cost's error: it is checked before the plan
    assert call(_cost(rank=0), model=_model(n_train=1100)) == ARG
    # env->obj_mode is not read
    odd = _env()
    odd.obj_mode = 7
    assert call(env=odd, model=_model(n_train=1100)) == UNSUPPORTED and call(env=odd, x0=None) == ARG


def test_cautious_sat_argument_errors():
    ok = _cost()
    assert _cautious(None) == ARG
    for what, bad in _bad_costs():
        assert _cautious(bad) == ARG, what
    for kw in (dict(x0=None), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None), dict(mean=None),
               dict(std=None), dict(E=0), dict(P=0), dict(T=0), dict(model=_model(n_train=0)), dict(model=_model(2, 2))):
        assert _cautious(ok, **kw) == ARG, kw
    neg, many, odd = _env(), _env(), _env()
    neg.m, many.m, odd.obj_mode = -1, _lib.SX_MAX_M + 1, 7
    assert _cautious(ok, env=neg) == ARG and _cautious(ok, env=many) == UNSUPPORTED
    assert _cautious(ok, model=_model(n_train=1100)) == UNSUPPORTED
    assert _cautious(ok, env=odd, model=_model(n_train=1100)) == UNSUPPORTED                 # obj_mode is not read
    assert _cautious(_cost(rank=4), model=_model(n_train=1100)) == ARG


# ---- the plumbing over a fake library ------------------------------------------------------------------------------------------
COST2 = SaturatingCost([0.1, 0.0, 0.9], np.diag([1.0, 0.0, 0.5]), trig_idx=0)      # n_s = 2: the fakes' models


def _hook(ps):
    raise AssertionError('the objective hook was evaluated beside a kernel-form cost')


def test_cautious_solver_reaches_the_sat_entry_once_per_iteration(monkeypatch):
    fake = _fake_device(monkeypatch, 8, [])
    iters, P, T = 3, 32, 4
    mpc = CautiousCemMpc(_Ssm(), _env(), T, P, 8, iters, device='cpu', init_std=0.2)
    mpc.set_env(_env(), objective_hook=_hook)
    mpc.set_cost(COST2)
    mpc.solve(torch.zeros((2, 2), dtype=torch.float64))
    assert fake.calls['sx_cem_cautious_rollout_sat'] == iters and fake.calls['sx_cem_cautious_rollout'] == 0
    args = fake.args['sx_cem_cautious_rollout_sat'][0]
    assert len(args) == 20 and args[3:6] == (2, P, T) and args[13] is None           # no trajectory is asked for
    # without a cost: the parent entry, and the hook (which needs the means)
    mpc.set_cost(None)
    with pytest.raises(AssertionError, match='hook was evaluated'):
        mpc.solve(torch.zeros((2, 2), dtype=torch.float64))
    assert fake.calls['sx_cem_cautious_rollout'] == 1 and fake.calls['sx_cem_cautious_rollout_sat'] == iters
    with pytest.raises(TypeError, match='SaturatingCost'):
        mpc.set_cost(lambda m, v: 0.0)
    with pytest.raises(ValueError, match='n_s = 4'):
        mpc.set_cost(SaturatingCost(so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, 2))


def test_fused_solver_reaches_the_sat_entry_once_per_iteration(monkeypatch):
    fake = _fake_device(monkeypatch, 8, [])
    iters, P, H, n_perf = 3, 32, 4, 6

    def safety(ssm, env, x0, horizon, *, noise, status=None, **kw):       # (the single-model safety rollout owns a workspace)
        E, P = x0.size(0), noise.size(1)
        return dict(actions=torch.zeros((E, P, horizon, 1), dtype=torch.float64), obj_cost=torch.zeros((E, P)),
                    con_cost=torch.zeros((E, P)), traj=None, sigma=None, status=status)

    monkeypatch.setattr(cem_mpc, 'cem_rollout', safety)
    mk = lambda **kw: FusedCemMpc(_Ssm(), _env(obj_mode=ABS), H, P, 8, iters, device='cpu', init_std=0.2, **kw)
    mpc = mk(n_perf=n_perf, perf_type='taylor')
    mpc.set_env(_env(obj_mode=ABS), objective_hook=_hook)
    mpc.set_cost(COST2)
    mpc.solve(torch.zeros((1, 2), dtype=torch.float64))
    assert fake.calls['sx_cem_perf_rollout_taylor_sat'] == iters and fake.calls['sx_cem_perf_rollout_taylor'] == 0
    args = fake.args['sx_cem_perf_rollout_taylor_sat'][0]
    assert len(args) == 22 and args[3:8] == (1, P, H, n_perf, 1)
    # a solver whose performance kind is not 'taylor' refuses the cost, naming the setting
    for kw in (dict(), dict(n_perf=n_perf), dict(n_perf=n_perf, perf_variance=True)):
        with pytest.raises(ValueError, match="cem_perf_type='taylor'"):
            mk(**kw).set_cost(COST2)


def test_multi_model_solve_needs_equal_costs(monkeypatch):
    fake = _fake_device(monkeypatch, 8, [])
    iters, P, H, n_perf = 2, 32, 4, 6
    solvers = [FusedCemMpc(_Ssm(20 + 10 * e), _env(obj_mode=ABS), H, P, 8, iters, device='cpu', init_std=0.2, seed=e,
                           n_perf=n_perf, perf_type='taylor') for e in range(3)]
    for s in solvers:
        s.set_cost(SaturatingCost(COST2.target, COST2.weight, 0))       # equal, not identical
    mpc = MultiModelPerfCemMpc.from_solvers(solvers)
    mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    assert fake.calls['sx_cem_perf_rollout_taylor_sat_multi'] == iters and fake.calls['sx_cem_perf_rollout_taylor_multi'] == 0
    assert fake.args['sx_cem_perf_rollout_taylor_sat_multi'][0][4:9] == (3, P, H, n_perf, 1)
    solvers[1].set_cost(None)
    with pytest.raises(ValueError, match='equal costs'):
        mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match='equal costs'):
        mpc.get_actions_multi(torch.zeros((3, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match='equal costs'):
        MultiModelPerfCemMpc.from_solvers(solvers)
    solvers[1].set_cost(SaturatingCost(COST2.target, 2 * COST2.weight, 0))
    with pytest.raises(ValueError, match='equal costs'):
        mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    mpc.set_cost(None)
    mpc.solve(torch.zeros((3, 2), dtype=torch.float64))
    assert fake.calls['sx_cem_perf_rollout_taylor_multi'] == iters


class _Mpc:
    """What init_solver reaches on an injected optimiser."""

    def __init__(self):
        self.costs = []

    def set_cost(self, cost):
        self.costs.append(cost)


def test_init_solver_hands_a_saturating_cost_to_the_optimiser():
    from safe_exploration_amd.cautious_mpc import CautiousCemMPC
    from safe_exploration_amd.safempc_cem import CemSafeMPC
    for cls, attrs in ((CautiousCemMPC, {}), (CemSafeMPC, dict(_perf=cem_mpc.PerfSpec(10, type='taylor')))):
        solver = cls.__new__(cls)
        solver._mpc, solver._cost = _Mpc(), None
        for k, v in attrs.items():
            setattr(solver, k, v)
        for other in (None, lambda *a: 0.0, 'cost', 3.0):
            solver.init_solver(other)                                   # any other value changes nothing
        assert solver._mpc.costs == [] and solver._cost is None
        solver.init_solver(COST2)
        assert solver._mpc.costs == [COST2] and solver._cost is COST2
        solver._mpc = None                                              # before the optimiser exists the cost is kept for it
        solver.init_solver(COST2)
        assert solver._cost is COST2
    for attrs in (dict(_perf=cem_mpc.PerfSpec(10, type='mean_equivalent')), dict(_perf=cem_mpc.PerfSpec(0, type='taylor'))):
        solver = CemSafeMPC.__new__(CemSafeMPC)
        solver._mpc, solver._cost = _Mpc(), None
        for k, v in attrs.items():
            setattr(solver, k, v)
        with pytest.raises(ValueError, match="cem_perf_type='taylor'"):
            solver.init_solver(COST2)
        solver.init_solver(lambda *a: 0.0)                              # ... and still ignores anything else
        assert solver._mpc.costs == []


# ---- the inputs of the GPU solve tests -----------------------------------------------------------------------------------------
SOLVE = dict(n_train=200, P=256, k=20, iters=4, init_std=1.0, seed=11, T=6, H=2, n_perf=6, r=1, gap=1e-6)
SOLVE_X0 = np.array([0.3, 0.0, 0.05, 0.0])


def solve_case():
    spec = problems.cartpole(n_train=SOLVE['n_train'])
    return spec, ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise), problems.oracle_problem(spec, ocem)


_SOLVES = {}


def oracle_solve(kind):
    """(best row, trace, noise) of the oracle's CEM with the cart-pole constants: kind 'cautious' | 'cautious_me' (propagate
    False) | 'taylor'.  Computed once and left unchanged."""
    if kind not in _SOLVES:
        c = SOLVE
        spec, gp, prob = solve_case()
        steps = c['T'] if kind.startswith('cautious') else c['H'] + c['n_perf'] - c['r']
        noise = np.random.default_rng(c['seed']).normal(size=(c['iters'], c['P'], steps, 1))
        if kind.startswith('cautious'):
            best, trace = so.cem_solve_cautious(CARTPOLE, prob, gp, SOLVE_X0, noise, c['k'], c['init_std'],
                                                propagate=kind == 'cautious')
        else:
            best, trace = so.cem_solve_perf_taylor(CARTPOLE, prob, gp, SOLVE_X0, noise, c['k'], c['H'], c['n_perf'], c['r'],
                                                   c['init_std'])
        _SOLVES[kind] = (best, trace, noise)
    return _SOLVES[kind]


@pytest.mark.parametrize('kind', ['cautious', 'cautious_me', 'taylor'])
def test_the_gpu_solve_inputs_are_decided(kind):
    """In every iteration of the oracle's solve the last elite and the first non-elite differ by more than 1e-6 (or in
    their constraint cost, which is exact), and so do the best two rows of the last one: rounding cannot swap them."""
    best, trace, _ = oracle_solve(kind)
    assert best is not None, 'the oracle\'s last iteration does not end feasible'
    gaps = so.elite_gaps(trace, SOLVE['k'])
    print(kind, 'elite gaps per iteration:', gaps)
    assert all(g > SOLVE['gap'] for g in gaps)
    con, obj, idx = trace[-1]
    order = ocem.rank(con, obj, 2)
    assert con[order[0]] != con[order[1]] or abs(obj[order[0]] - obj[order[1]]) > SOLVE['gap']
    for con, obj, idx in trace:
        assert np.isfinite(obj).all() and (obj > 0).all() and (obj < len(trace[0][0])).all()
    assert any((con > 0).any() for con, _, _ in trace), 'no constraint is ever active'
