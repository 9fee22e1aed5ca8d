"""CPU: static exploration in the CEM solver, host side -- sx_cem_rollout_starts and its form query are declared, exported
and bound, check their arguments before any device access and answer the form by the streaming kernel's LDS rule; the
numpy oracle (tests/static_explore_oracle.py) reduces to oracle.cem.cem_solve where all starts are equal and applies the
start rule to the known polytope geometries; a StaticCemMpc solve makes one rollout and one ranking launch per iteration
over rows of n_s + H n_u entries and picks among its restarts (fakes in place of the launches); StaticSafeMPCExploration
scales the start distribution as the reference's `_sample_start_state` does and keeps its return shapes; and
cem_rollout_stepwise makes the same calls for a start [n_s] and for that start tiled to [P x n_s]."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import static_explore_oracle as seo
from oracle import cem as ocem
from oracle.gp import ExactGP
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.cem_mpc import StaticCemMpc
from safe_exploration_amd.safempc_exploration import StaticSafeMPCExploration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
ENTRIES = ['sx_cem_rollout_starts', 'sx_cem_rollout_starts_form']


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ENTRIES)
def test_entries_are_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    assert re.search(r'\bint ' + name + r'\(', header)
    assert name in _lib.SIGNATURES
    fn = getattr(_lib.lib(), name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert len(fn.argtypes) == (15 if name == 'sx_cem_rollout_starts' else 2)


def _model(n_s=2, n_u=1, n_train=20):
    """A model as far as the host reads it: the pointers are never dereferenced (every call below is answered before any
    device access)."""
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.n_pad = (n_train + 1 + n_s + n_u + 15) // 16 * 16       # sx_gp.hpp: gp_n_pad
    m.x_train, m.a_pack, m.stage_tab = 16, 16, 16
    for i in range(n_s * (n_s + n_u)):
        m.inv_ls2[i] = 1.0
    for i in range(n_s):
        m.outputscale[i] = 1.0
    return m


def _env(n_s=2, n_u=1, m=4):
    env = _lib.SxEnv()
    env.n_s, env.n_u, env.m = n_s, n_u, m
    return env


def _call(*, model=(), env=(), no_model=False, no_env=False, E=2, P=4, H=5, mean=16, std=16, noise=16, rows=16, obj=16, con=16,
          status=16):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    m, e = _model(*model), _env(*env)
    return _lib.lib().sx_cem_rollout_starts(None if no_model else ctypes.byref(m), None if no_env else ctypes.byref(e), E, P, H,
                                            p(mean), p(std), p(noise), p(rows), None, None, p(obj), p(con), p(status), None)


REFUSALS = [
    ('model null', dict(no_model=True), ARG),
    ('env null', dict(no_env=True), ARG),
    ('rows null', dict(rows=None), ARG),
    ('obj_cost null', dict(obj=None), ARG),
    ('con_cost null', dict(con=None), ARG),
    ('status null', dict(status=None), ARG),
    ('E = 0', dict(E=0), ARG),
    ('P = 0', dict(P=0), ARG),
    ('H = 0', dict(H=0), ARG),
    ('P < 0', dict(P=-3), ARG),
    ('noise without mean', dict(mean=None), ARG),
    ('noise without std', dict(std=None), ARG),
    ('model and env disagree on n_u', dict(model=(2, 2)), ARG),
    ('model and env disagree on n_s', dict(env=(4, 1)), ARG),
    ('n_train = 0', dict(model=(2, 1, 0)), ARG),
    ('a null pointer before an uncompiled shape', dict(model=(3, 2), env=(3, 2), rows=None), ARG),
    ('a shape without a rollout kernel', dict(model=(3, 2), env=(3, 2)), UNSUPPORTED),
    ('m > SX_MAX_M', dict(env=(2, 1, 17)), UNSUPPORTED),
    ('m = 0', dict(env=(2, 1, 0)), UNSUPPORTED),
    ('a training set on the workspace path', dict(model=(2, 1, 2000)), UNSUPPORTED),
    ('n_s = 1 has no output-by-output form', dict(model=(1, 1, 1000), env=(1, 1), H=600), UNSUPPORTED),
]


@pytest.mark.parametrize('what,kw,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_without_a_gpu(what, kw, code):
    assert _call(**kw) == code


def test_the_workspace_model_is_one_the_plain_entry_serves():
    """sx_cem_rollout takes N = 2000 through its workspace path; the per-particle-start entry has none."""
    big = _model(2, 1, 2000)
    assert int(_lib.lib().sx_cem_rollout_workspace_bytes(ctypes.byref(big), 2, 4, 5)) > 0
    assert int(_lib.lib().sx_cem_rollout_starts_form(ctypes.byref(big), 5)) < 0


def lds_bytes(n_s, n_u, n_pad, H, byout):
    """rollout_stream_lds_bytes (csrc/sx_stream_launch.hpp) on 8 waves: gp_tile_lds_doubles + the tile's actions."""
    d = n_s + n_u
    doubles = ((n_pad * d + 1) & ~1) + (1 if byout else n_s) * n_pad * 16 + n_s * 256 + 8 * n_s * 16 + 32 * d + 512
    return 8 * (doubles + 16 * H * n_u)


def form_rule(n_s, n_u, n_pad, H):
    if n_pad <= 1024 and lds_bytes(n_s, n_u, n_pad, H, False) <= 160 * 1024:
        return SX_FORM_STREAM
    if n_s > 1 and n_pad <= 1024 and lds_bytes(n_s, n_u, n_pad, H, True) <= 160 * 1024:
        return SX_FORM_BYOUT
    return -1


def byout_model_size(n_s=4, n_u=1, H=3):
    """The smallest N whose (n_s, n_u) model takes the output-by-output form at horizon H (None if there is none)."""
    for N in range(16, 1024):
        m = _model(n_s, n_u, N)
        if m.n_pad <= 1024 and int(_lib.lib().sx_cem_rollout_starts_form(ctypes.byref(m), H)) == SX_FORM_BYOUT:
            return N
    return None


@pytest.mark.parametrize('n_s,n_u', [(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2)])
def test_form_query_follows_the_lds_rule(n_s, n_u):
    lib = _lib.lib()
    seen = set()
    for H in (3, 15, 400):
        for N in list(range(1, 1200, 13)) + [2000]:
            m = _model(n_s, n_u, N)
            got = int(lib.sx_cem_rollout_starts_form(ctypes.byref(m), H))
            assert got == form_rule(n_s, n_u, m.n_pad, H), (N, H)
            seen.add(got)
    assert seen == ({SX_FORM_STREAM, -1} if n_s == 1 else {SX_FORM_STREAM, SX_FORM_BYOUT, -1})
    assert int(lib.sx_cem_rollout_starts_form(None, 3)) < 0 and int(lib.sx_cem_rollout_starts_form(ctypes.byref(m), 0)) < 0
    assert int(lib.sx_cem_rollout_starts_form(ctypes.byref(_model(3, 2, 20)), 3)) < 0          # no rollout kernel


def test_an_output_by_output_model_exists_at_4_1_within_1024():
    N = byout_model_size()
    assert N is not None and _model(4, 1, N).n_pad <= 1024
    assert form_rule(4, 1, _model(4, 1, N).n_pad, 3) == SX_FORM_BYOUT


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def _pendulum(n_train=40):
    spec = problems.pendulum(n_train=n_train, seed=0)
    gp = ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)
    return problems.oracle_problem(spec, ocem), gp


def test_oracle_with_equal_starts_is_the_plain_cem_solve():
    """start_std = 0 puts every particle at start_mean (dyadic values: every refit of the start columns is exact), inside
    the polytope: rollouts, ranking, refits and the answer are oracle.cem.cem_solve's from that start."""
    prob, gp = _pendulum()
    P, H, k, iters = 24, 3, 6, 3
    x0 = np.array([0.0625, -0.03125])
    rng = np.random.default_rng(4)
    noise = rng.normal(size=(iters, P, prob.n_s + H * prob.n_u))
    best, costs, ok, trace = seo.cem_solve(prob, gp, noise, k, x0, 0.0, init_std=0.3)
    act_noise = noise[:, :, prob.n_s:].reshape(iters, P, H, prob.n_u)
    ref_best, ref_trace = ocem.cem_solve(prob, gp, x0, act_noise, k, init_std=np.full((H, prob.n_u), 0.3))
    assert not seo.start_outside(prob, x0[None])[0]
    for it in range(iters):
        np.testing.assert_array_equal(trace[it][2], ref_trace.elites[it])
        assert trace[it][0][trace[it][2][0]] == ref_trace.best_con[it]
    assert ok == (ref_best is not None) and ok, 'the test problem should be feasible'
    np.testing.assert_array_equal(best[:prob.n_s], x0)
    np.testing.assert_array_equal(best[prob.n_s:].reshape(H, prob.n_u), ref_best)


def test_oracle_start_rule_on_the_known_geometries(golden_dir):
    """The box [0, 10]^2 of tests/golden/polytope.npz: (5, 5) is inside, (0, 0) lies on two faces (d = 0 counts as outside,
    the reference's "inside iff no d >= 0"), (20, 20) is outside.  The cost is STATE_VIOLATION_COST once, in either mode."""
    g = np.load(os.path.join(golden_dir, 'polytope.npz'))
    prob, gp = _pendulum()
    prob.h_mat, prob.h_vec = g['box_A'], g['box_b']
    np.testing.assert_array_equal(seo.start_outside(prob, g['p3']), [False, True, True])
    np.testing.assert_array_equal(seo.start_outside(prob, g['p3']), ~g['inside'].astype(bool) | np.array([False, True, False]))
    rows = np.concatenate((g['p3'], np.zeros((3, 2))), axis=1)          # H = 2 zero actions
    for con_mode in (ocem.CON_TERMINAL, ocem.CON_ALL_STATES):
        prob.con_mode = con_mode
        res = seo.rollout(prob, gp, rows)
        np.testing.assert_array_equal(res.start_cost, [0.0, 10.0, 10.0])
        plain = ocem.rollout(prob, gp, rows[:, :2], rows[:, 2:].reshape(3, 2, 1))
        np.testing.assert_array_equal(res.con_cost, plain.con_cost + res.start_cost)
        np.testing.assert_array_equal(res.obj_cost, -plain.sigma.sum(axis=(1, 2)))


def test_oracle_choice_among_restarts():
    assert seo.choose([False, True, True], [-9.0, -1.0, -2.0]) == 2
    assert seo.choose([True, True, False], [-1.0, -1.0, -5.0]) == 0            # a tie goes to the lower index
    assert seo.choose([False, False], [-1.0, -2.0]) is None


# ---- StaticCemMpc over fake launches -----------------------------------------------------------------------------------------
class _Ssm:
    num_states, num_actions, kernel_family = 2, 1, 'rbf'

    def __init__(self, family='rbf'):
        self.kernel_family = family
        self.device_model = _model()


def _fakes(monkeypatch, k, final=None):
    """Records the calls.  Ranking i (from 1) refits to mean i, std 10 i; `final` [E x (con, obj)] are the costs of the last
    ranking's best rows, whose row e is filled with e + 1."""
    calls = []

    def rollout(ssm, env, horizon, *, mean, std, noise, want_traj=False, status=None, **kw):
        calls.append(('rollout', tuple(mean.shape), tuple(noise.shape), float(mean[0, 0]), float(std[0, 0]), env.obj_mode))
        E, P, L = noise.shape
        return dict(rows=torch.zeros((E, P, L), dtype=torch.float64), obj_cost=torch.zeros((E, P)),
                    con_cost=torch.zeros((E, P)), traj=None, sigma=None, status=status)

    def rank(con, obj, rows, kk, want_rows=False, want_refit=True):
        assert kk == k
        E, L, i = con.size(0), rows.size(2), 1 + sum(c[0] == 'rank' for c in calls)
        calls.append(('rank', L, want_rows, want_refit))
        full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64)
        elite = None
        if want_rows:
            elite = full(0, E, k, 2 + L)
            if final is not None:
                elite[:, 0, :2] = torch.tensor(final, dtype=torch.float64)
        best = torch.arange(1, E + 1, dtype=torch.float64).view(E, 1).expand(E, L).contiguous()
        ok = (elite[:, 0, 0] == 0).to(torch.int32) if elite is not None else torch.zeros(E, dtype=torch.int32)
        return dict(elite_rows=elite, mean=full(i, E, L), std=full(10 * i, E, L), best=best, best_ok=ok)

    def hand_off(owner, best, best_ok, status, q_block):
        calls.append(('hand_off', tuple(best.shape)))
        return status.to(torch.int64), best_ok != 0, False, best.clone()

    monkeypatch.setattr(cem_mpc, 'cem_rollout_starts', rollout)
    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)
    monkeypatch.setattr(cem_mpc, '_hand_off', hand_off)
    return calls


def _solver(E=3, P=32, H=5, k=4, iters=3, **kw):
    env = _env()
    env.obj_mode = _lib.SX_OBJ_AFFINE_ABS
    return StaticCemMpc(_Ssm(), env, H, P, k, iters, start_mean=[0.5, -0.5], start_std=[0.25, 0.125], n_restarts=E,
                        init_std=0.2, device='cpu', **kw)


def test_solve_makes_one_rollout_and_one_ranking_per_iteration_over_long_rows(monkeypatch):
    E, P, H, k, iters = 3, 32, 5, 4, 3
    L = 2 + H * 1
    calls = _fakes(monkeypatch, k, final=[[0.0, -1.0]] * E)
    mpc = _solver(E, P, H, k, iters)
    best, costs, ok, history, status = mpc.solve()
    assert tuple(best.shape) == (E, L) and tuple(costs.shape) == (E, 2) and tuple(ok.shape) == (E,)
    assert tuple(status.shape) == (1,) and history == []
    var = _lib.SX_OBJ_NEG_VARIANCE          # whatever the environment's objective: the solver's copy has the variance one
    want = [('rollout', (E, L), (E, P, L), 0.5, 0.25, var), ('rank', L, False, True)]
    for i in range(1, iters):
        want += [('rollout', (E, L), (E, P, L), float(i), 10.0 * i, var), ('rank', L, i == iters - 1, True)]
    assert calls == want
    assert mpc._env.obj_mode == var and mpc._env.m == 4


def test_first_distribution_is_start_then_actions():
    mpc = _solver(H=3)
    np.testing.assert_array_equal(mpc._mean0.numpy(), [0.5, -0.5, 0, 0, 0])
    np.testing.assert_array_equal(mpc._std0.numpy(), [0.25, 0.125, 0.2, 0.2, 0.2])


def test_restarts_draw_their_own_noise_from_seed_plus_e():
    a, b = _solver(E=3, seed=5), _solver(E=2, seed=6)
    na, nb = a.sample_noise(), b.sample_noise()
    assert tuple(na.shape) == (3, 3, 32, 7)
    assert torch.equal(na[:, 1], nb[:, 0]) and torch.equal(na[:, 2], nb[:, 1]) and not torch.equal(na[:, 0], na[:, 1])


@pytest.mark.parametrize('final,chosen', [
    ([[0.0, -1.0], [0.0, -3.0], [0.0, -2.0]], 1),       # the lowest objective among the feasible
    ([[0.0, -1.0], [10.0, -9.0], [0.0, -2.0]], 2),      # an infeasible restart is out, whatever its objective
    ([[0.0, -2.0], [0.0, -2.0], [0.0, -1.0]], 0),       # a tie goes to the lowest e
    ([[3.0, -2.0], [10.0, -2.0], [13.0, -1.0]], None),  # none feasible
])
def test_find_selects_among_the_restarts(monkeypatch, final, chosen):
    E, H = 3, 5
    calls = _fakes(monkeypatch, 4, final=final)
    mpc = _solver(E=E, H=H)
    out = mpc.find()
    assert [c for c in calls if c[0] == 'hand_off'] == [('hand_off', (E, 2 + H + 2))]       # one hand-off per call
    assert mpc.last_choice == chosen
    if chosen is None:
        assert out is None
        return
    x0, actions, obj = out
    assert tuple(x0.shape) == (2,) and tuple(actions.shape) == (H, 1) and obj == final[chosen][1]
    assert torch.all(x0 == chosen + 1) and torch.all(actions == chosen + 1)                  # restart e's row is e + 1
    np.testing.assert_array_equal(mpc.last_costs.numpy(), final)


def test_find_raises_on_nan_and_repeats_step_by_step_on_nan_with_zero_fix(monkeypatch):
    calls = _fakes(monkeypatch, 4, final=[[0.0, -1.0]] * 3)
    mpc = _solver()
    words = iter([_lib.SX_STATUS_NAN | _lib.SX_STATUS_ZERO_FIX, _lib.SX_STATUS_ZERO_FIX])
    real = cem_mpc._hand_off
    monkeypatch.setattr(cem_mpc, '_hand_off', lambda *a: (torch.tensor([next(words)]),) + real(*a)[1:])
    stepwise = []
    monkeypatch.setattr(mpc, '_rollout_stepwise', lambda mean, std, eps, status: stepwise.append(eps) or dict(
        rows=torch.zeros_like(eps), obj_cost=torch.zeros(eps.shape[:2]), con_cost=torch.zeros(eps.shape[:2]), traj=None))
    first_noise = []
    monkeypatch.setattr(mpc, 'sample_noise', lambda: first_noise.append(torch.randn(3, 3, 32, 7, dtype=torch.float64))
                        or first_noise[-1])
    assert mpc.find() is not None and mpc.stepwise_fallbacks == 1 and mpc.last_status == _lib.SX_STATUS_ZERO_FIX
    assert len(first_noise) == 1 and len(stepwise) == 3                                       # the same draws, step by step
    assert all(torch.equal(stepwise[it], first_noise[0][it]) for it in range(3))
    monkeypatch.setattr(cem_mpc, '_hand_off', lambda *a: (torch.tensor([_lib.SX_STATUS_NAN]),) + real(*a)[1:])
    monkeypatch.setattr(cem_mpc, 'save_failure_state', lambda *a, **kw: None)
    with pytest.raises(ValueError, match='nan in StaticCemMpc.find'):
        mpc.find()


def test_solver_refusals():
    env = _env()
    kw = dict(start_mean=[0, 0], start_std=[1, 1], device='cpu')
    for family in ('feature', 'mlp', 'rbf_junk', 'stepwise'):
        with pytest.raises(NotImplementedError, match=family):
            StaticCemMpc(_Ssm(family), env, 5, 32, 4, 3, **kw)
    with pytest.raises(NotImplementedError, match='process group'):
        StaticCemMpc(_Ssm(), env, 5, 32, 4, 3, process_group=object(), **kw)
    with pytest.raises(ValueError, match='num_elites'):
        StaticCemMpc(_Ssm(), env, 5, 32, 33, 3, **kw)
    with pytest.raises(ValueError, match='n_restarts'):
        StaticCemMpc(_Ssm(), env, 5, 32, 4, 3, n_restarts=0, **kw)
    with pytest.raises(NotImplementedError, match="'feature'"):
        cem_mpc.cem_rollout_starts(_Ssm('feature'), env, 5, rows=torch.zeros((1, 4, 7), dtype=torch.float64))


def test_junk_dimension_models_are_refused():
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    junk = JunkDimensionsSSM(lambda state_dimen, action_dimen: _Ssm(), state_dimen=2, action_dimen=1, junk_states=1,
                             junk_actions=1)
    assert junk.kernel_family == 'rbf_junk'
    with pytest.raises(NotImplementedError, match='rbf_junk'):
        StaticCemMpc(junk, _env(), 5, 32, 4, 3, start_mean=[0, 0], start_std=[1, 1], device='cpu')


# ---- StaticSafeMPCExploration over a fake solver -----------------------------------------------------------------------------
class _StaticSolver:
    def __init__(self, answer):
        self.answer, self.finds = answer, 0

    def find(self):
        self.finds += 1
        return self.answer


class _SafeMpc:
    state_dimen, action_dimen, safety_trajectory_length = 2, 1, 5
    x_train = np.zeros((3, 3))

    def __init__(self, answer):
        self.solver, self.asked, self.updates = _StaticSolver(answer), [], []

    def init_solver(self, cost_func=None):
        pass

    def static_solver(self, n_restarts, sample_mean, sample_std):
        self.asked.append((n_restarts, np.array(sample_mean), np.array(sample_std)))
        return self.solver

    def update_model(self, *args):
        self.updates.append(args)

    def information_gain(self):
        return 'gain'

    def ssm_predict(self, z):
        return 'prediction', z


def _environment():
    return types.SimpleNamespace(init_m=np.array([0.1, -0.2]), init_std=np.array([0.3, 0.4]),
                                 inv_norm=[np.array([2.0, 0.5]), np.array([4.0])])


def test_exploration_scales_the_start_distribution_and_keeps_the_reference_shapes():
    answer = (torch.tensor([0.2, -0.1], dtype=torch.float64),
              torch.tensor([[0.7], [0.1], [0.2], [0.3], [0.4]], dtype=torch.float64), -0.5)
    mpc = _SafeMpc(answer)
    ex = StaticSafeMPCExploration(mpc, _environment(), n_restarts_optimizer=6, verbosity=0)
    (n, mean, std), = mpc.asked
    assert n == 6 and ex.T == 5 and ex.n_s == 2 and ex.n_u == 1
    np.testing.assert_array_equal(mean, [0.2, -0.1])        # init_m * inv_norm[0]
    np.testing.assert_array_equal(std, [0.6, 0.2])          # init_std * inv_norm[0]
    x, u = ex.find_max_variance(None)
    assert x.shape == (2, 1) and u.shape == (1, 1) and mpc.solver.finds == 1
    np.testing.assert_array_equal(x[:, 0], [0.2, -0.1])
    np.testing.assert_array_equal(u, [[0.7]])               # the first action of the plan
    ex.update_model('x', 'y', True, False)
    assert mpc.updates == [('x', 'y', True, False)]
    assert ex.get_information_gain() == 'gain' and ex.ssm_predict('z') == ('prediction', 'z') and ex.x_train.shape == (3, 3)
    with pytest.raises(NotImplementedError):
        ex.find_max_variance_verbose(None)


def test_exploration_takes_a_given_distribution_and_answers_none_none():
    mpc = _SafeMpc(None)
    ex = StaticSafeMPCExploration(mpc, _environment(), 2, sample_mean=np.array([1.0, 1.0]), sample_std=np.array([0.5, 2.0]))
    (n, mean, std), = mpc.asked
    assert n == 2
    np.testing.assert_array_equal(mean, [2.0, 0.5])
    np.testing.assert_array_equal(std, [1.0, 1.0])
    assert ex.find_max_variance(None) == (None, None)
    assert StaticSafeMPCExploration(_SafeMpc(None), _environment()).n_restarts_optimizer == 1


def test_exploration_refuses_a_solver_without_a_static_form():
    with pytest.raises(NotImplementedError, match='static_solver'):
        StaticSafeMPCExploration(types.SimpleNamespace(state_dimen=2, action_dimen=1), _environment())


# ---- the step-by-step rollout with a start per particle ----------------------------------------------------------------------
def _stepwise_calls(monkeypatch, x0, actions):
    calls = []

    class Ssm:
        num_states, num_actions = 2, 1

        def predict_without_jacobians(self, p, u):
            calls.append(('predict', p.clone(), u.clone()))
            return 0.1 * p, 0.01 + 0.0 * p

        def predict_with_jacobians(self, p, u):
            calls.append(('predict_jac', p.clone(), u.clone()))
            return 0.1 * p, 0.01 + 0.0 * p, torch.zeros((p.size(0), 2, 3), dtype=torch.float64)

    class Lib:
        def sx_onestep_reach(self, env, P, p, q, u, mean, var, jac, p1, q1, sigma, status, stream):
            calls.append(('reach', P, q is None, jac is None))
            return 0

        def sx_polytope_distance(self, env, P, p, q, c, d, inside, stream):
            calls.append(('polytope', P, c))
            return 0

    monkeypatch.setattr(_lib, 'lib', lambda: Lib())
    monkeypatch.setattr(_lib, 'stream_ptr', lambda dev: None)
    monkeypatch.setattr(torch, 'empty', torch.zeros)        # the fakes write nothing: the step's outputs are then zeros
    monkeypatch.setattr(torch, 'empty_like', torch.zeros_like)
    status = torch.zeros(1, dtype=torch.int32)
    env = _env()
    env.con_mode = _lib.SX_CON_ALL_STATES
    out = cem_mpc.cem_rollout_stepwise(Ssm(), env, x0, actions, status=status)
    return calls, out


def test_stepwise_rollout_makes_the_same_calls_for_a_start_and_for_that_start_tiled(monkeypatch):
    P, H = 5, 3
    actions = torch.linspace(-1, 1, P * H, dtype=torch.float64).view(P, H, 1)
    x0 = torch.tensor([0.3, -0.2], dtype=torch.float64)
    one, out_one = _stepwise_calls(monkeypatch, x0, actions)
    tiled, out_tiled = _stepwise_calls(monkeypatch, x0.expand(P, 2).contiguous(), actions)
    assert [c[0] for c in one] == ['predict', 'reach', 'polytope'] + ['predict_jac', 'reach', 'polytope'] * (H - 1)
    assert len(one) == len(tiled)
    for a, b in zip(one, tiled):
        assert a[0] == b[0]
        assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a[1:], b[1:]))
    assert tuple(one[0][1].shape) == (P, 2)
    assert torch.equal(out_one['obj_cost'], out_tiled['obj_cost']) and torch.equal(out_one['con_cost'], out_tiled['con_cost'])
    # distinct starts reach the first prediction as they are
    starts = torch.arange(2 * P, dtype=torch.float64).view(P, 2)
    calls, _ = _stepwise_calls(monkeypatch, starts, actions)
    assert torch.equal(calls[0][1], starts)
