"""GPU: multi-step reachability under a feedback gain per particle and step -- sx_cem_rollout_gains
(cem_rollout_kernel<StreamGains>) against the chained numpy oracle (tests/multistep_oracle.py: one
oracle.reachability.onestep_reachability per rollout and step with that step's gain, plus the costs sx_cem_rollout_starts
charges), in both forms, at the edges of the gain, against sx_cem_rollout_starts under a constant gain, past one pass of the
grid, with a non-finite gain; `multistep_reachability` against the reference's own runs (tests/golden/multistep_*.npz), its
one launch and its step-by-step path; and `run_uncertainty_propagation` end to end.

Shapes: every (n_s, n_u) of {(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2)} with N = 40 training points, E = 1, P = 37
particles (three tiles, the last with 5 live lanes) and H = 4; (2, 1) also with E = 2; a (4, 1) model whose training set
takes the output-by-output form, found through the form query.  The polytope of a case comes from oracle/cases.py over the
oracle's trajectories with the start as step 0.

Tolerance: 1e-10, the fused-against-oracle convention of tests/test_gpu_junk_fused.py, of |got - want| relative to
max(1, max_t |Q_t|) of the PARTICLE compared (no looser than relative to the largest |Q| of the launch); constraint costs
and status exactly; bit-equality where two launches of the kernel must agree.  Every figure is printed before it is
asserted."""
import collections
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import multistep_oracle as mo
import test_gpu_rollout_matrix as rm
from oracle import cases
from oracle import cem as ocem
from oracle.gp import ExactGP
from safe_exploration_amd import _lib
from test_gpu_junk_fused import CountingLib
from test_multistep_host import LinearEnv

pytestmark = pytest.mark.gpu
T = rm.T
P, H, N = 37, 4, 40
TOL = 1e-10
VAR, ABS = _lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS
TERMINAL, ALL_STATES = _lib.SX_CON_TERMINAL, _lib.SX_CON_ALL_STATES
MODES = ((VAR, ALL_STATES), (ABS, TERMINAL))
SX_FORM_BYOUT = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SHAPES = [(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2)]


def byout_size(n_s, n_u, horizon):
    """The smallest N whose model takes the output-by-output form at this horizon, by sx_cem_rollout_gains_form."""
    from test_static_explore_host import _model
    for n in range(16, 1024):
        m = _model(n_s, n_u, n)
        if m.n_pad <= 1024 and int(_lib.lib().sx_cem_rollout_gains_form(ctypes.byref(m), horizon)) == SX_FORM_BYOUT:
            return n
    raise AssertionError('no output-by-output model')


@functools.lru_cache(maxsize=None)
def model_data(n_s, n_u, n_train=N):
    """(X, Y, lengthscales, outputscales, noise, the numpy oracle) of a case's exact GP.  CPU only."""
    X, Y = rm.training_set(n_s, n_u, n_train, 23 + n_s + 3 * n_u)
    rng = np.random.default_rng(600 + 10 * n_s + n_u)
    ls, s, nz = rng.uniform(0.6, 1.4, size=(n_s, n_s + n_u)), rng.uniform(1e-4, 3e-4, size=n_s), rng.uniform(1e-6, 5e-6, size=n_s)
    return X, Y, ls, s, nz, ExactGP(X, Y, ls, s, nz)


@functools.lru_cache(maxsize=None)
def model(n_s, n_u, n_train=N):
    """(GpCemSSM with data on the GPU, its numpy oracle)."""
    X, Y, ls, s, nz, gp = model_data(n_s, n_u, n_train)
    ssm = rm.constructor('rbf')(state_dimen=n_s, action_dimen=n_u)
    ssm.set_hyperparameters(ls, s, nz)
    ssm.update_model(T(X), T(Y), replace_old=True)
    return ssm, gp


Case = collections.namedtuple('Case', 'n_s n_u n_train gp sysd con rows gains refs')


@functools.lru_cache(maxsize=None)
def case(n_s, n_u, E=1, horizon=H, n_train=N, gains='random'):
    """The inputs of one case and the oracle's answers, computed once (CPU only) and shared by the checks:
    refs[(obj_mode, con_mode)][e] is multistep_oracle.rollout of problem e.  `gains`: 'random' (0.3 randn, different per
    particle AND step), 'edge' (particle 0 all-zero, particle 1 of magnitude 5, the rest random), 'constant' (env's k_fb)."""
    gp = model_data(n_s, n_u, n_train)[-1]
    sysd = rm.system(n_s, n_u)
    rng = np.random.default_rng(70 + 10 * n_s + n_u + E + horizon)
    rows = np.concatenate((rng.normal(0, 0.1, size=(E, P, n_s)), rng.normal(0, 0.3, size=(E, P, horizon * n_u))), axis=2)
    k = 0.3 * rng.normal(size=(E, P, horizon - 1, n_u, n_s))
    if gains == 'edge':
        k[:, 0] = 0.0
        k[:, 1] = 5.0 * np.sign(k[:, 1])
    elif gains == 'constant':
        k[:] = sysd['k_fb']
    wide = rm.Constraints(sysd, np.vstack((np.eye(n_s), -np.eye(n_s))), np.full((2 * n_s, 1), 1e30), np.full(n_u, -1e3),
                          np.full(n_u, 1e3))
    free = [mo.rollout(wide.problem(VAR, ALL_STATES), gp, rows[e], k[e]) for e in range(E)]
    assert not any(f.status.any() for f in free)
    traj_p = np.concatenate([np.concatenate((rows[e][:, None, :n_s], free[e].traj_p), axis=1) for e in range(E)])
    traj_q = np.concatenate([np.concatenate((np.zeros((P, 1, n_s, n_s)), free[e].traj_q), axis=1) for e in range(E)])
    h_mat, h_vec = cases.active_polytope(np.random.default_rng(5 + n_s + n_u), traj_p, traj_q, np.zeros((E, n_s)),
                                         m=2 * n_s + 1)
    bound = np.full(n_u, np.abs(rows[:, :, n_s:]).max() + 1.0)
    bound[-1] = np.quantile(np.abs(rows[:, :, n_s:].reshape(E, P, horizon, n_u)[..., -1]).ravel(), 0.9)
    con = rm.Constraints(sysd, h_mat, h_vec, -bound, bound.copy())
    assert cases.min_abs_distance(traj_p, traj_q, h_mat, h_vec) > 1e-8
    refs = {(o, c): [mo.rollout(con.problem(o, c), gp, rows[e], k[e]) for e in range(E)] for o, c in MODES}
    return Case(n_s, n_u, n_train, gp, sysd, con, rows, k, refs)


def ssm_of(c):
    return model(c.n_s, c.n_u, c.n_train)[0]


def launch(c, env, gains=None, rows=None, horizon=H):
    from safe_exploration_amd.cem_mpc import cem_rollout_gains
    return cem_rollout_gains(ssm_of(c), env, horizon, rows=T(c.rows if rows is None else rows),
                             gains=T(c.gains if gains is None else gains), want_traj=True, want_sigma=True)


def unpack(r, e, n_s):
    traj = r['traj'][e].cpu().numpy()
    return (traj[..., :n_s], traj[..., n_s:].reshape(traj.shape[0], traj.shape[1], n_s, n_s), r['sigma'][e].cpu().numpy(),
            r['obj_cost'][e].cpu().numpy(), r['con_cost'][e].cpu().numpy())


def particle_err(got, want, q_ref):
    """[P]: max |got - want| of each particle relative to max(1, max_t |Q_t|) of that particle."""
    n = got.shape[0]
    scale = np.maximum(1.0, np.abs(q_ref).reshape(n, -1).max(axis=1))
    return np.abs(got - want).reshape(n, -1).max(axis=1) / scale


def check_against(r, e, ref, n_s, what):
    tp, tq, sig, obj, con = unpack(r, e, n_s)
    errs = dict(centres=particle_err(tp, ref.traj_p, ref.traj_q).max(), shapes=particle_err(tq, ref.traj_q, ref.traj_q).max(),
                sigma=particle_err(sig, ref.sigma, ref.traj_q).max(), obj=particle_err(obj, ref.obj_cost, ref.traj_q).max())
    print(f'  {what}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()) + f' con differs at {int((con != ref.con_cost).sum())}'
          f' max |Q| {np.abs(ref.traj_q).max():.3g}')
    assert all(v <= TOL for v in errs.values()), errs
    np.testing.assert_array_equal(con, ref.con_cost)


def non_vacuous(c):
    """Some particles leave the polytope and some do not, and the two modes price them differently."""
    a, b = (np.concatenate([r.con_cost for r in c.refs[m]]) for m in MODES)
    assert (a == 0).any() and (a >= ocem.STATE_VIOLATION_COST).any() and (a != b).any()


def env_without_gain(c, o, cm):
    """The case's sx_env with a k_fb that would poison the result if it were read."""
    env = c.con.env(o, cm)
    _lib.fill(env.k_fb, np.full((c.n_u, c.n_s), np.nan))
    return env


def run_case(c, E, what):
    non_vacuous(c)
    for o, cm in MODES:
        r = launch(c, env_without_gain(c, o, cm))
        status = int(r['status'].item())
        for e in range(E):
            check_against(r, e, c.refs[(o, cm)][e], c.n_s, f'{what} obj {o} con {cm} problem {e}')
        assert status == int(np.bitwise_or.reduce(np.concatenate([ref.status for ref in c.refs[(o, cm)]]))) == 0


# ---- against the chained oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_rollout_matches_the_chained_oracle(n_s, n_u):
    c = case(n_s, n_u)
    assert int(_lib.lib().sx_cem_rollout_gains_form(ctypes.byref(ssm_of(c).device_model), H)) == 0
    # the gains differ per particle and per step
    assert len(np.unique(c.gains.reshape(-1, n_u * n_s), axis=0)) == P * (H - 1)
    run_case(c, 1, f'({n_s},{n_u})')


def test_two_problems_in_one_launch():
    run_case(case(2, 1, E=2), 2, '(2,1) E=2')


def test_output_by_output_form():
    n = byout_size(4, 1, H)
    c = case(4, 1, n_train=n)
    assert int(_lib.lib().sx_cem_rollout_gains_form(ctypes.byref(ssm_of(c).device_model), H)) == SX_FORM_BYOUT
    print(f'N = {n}')
    run_case(c, 1, '(4,1) output by output')


@pytest.mark.parametrize('n_s,n_u', [(2, 1), (4, 2)])
def test_zero_gains_and_large_gains(n_s, n_u):
    c = case(n_s, n_u, gains='edge')
    assert not c.gains[0, 0].any() and (np.abs(c.gains[0, 1]) == 5.0).all()
    run_case(c, 1, f'({n_s},{n_u}) edge gains')


# ---- against sx_cem_rollout_starts under one gain ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u', [(2, 1), (4, 2)])
def test_constant_gains_equal_the_starts_rollout(n_s, n_u):
    from safe_exploration_amd.cem_mpc import cem_rollout_starts
    c = case(n_s, n_u, gains='constant')
    for o, cm in MODES:
        env = c.con.env(o, cm)
        r = launch(c, env_without_gain(c, o, cm))
        s = cem_rollout_starts(ssm_of(c), env, H, rows=T(c.rows), want_traj=True, want_sigma=True)
        tp, tq, sig, obj, con = unpack(r, 0, n_s)
        sp, sq, ssig, sobj, scon = unpack(s, 0, n_s)
        errs = dict(centres=particle_err(tp, sp, sq).max(), shapes=particle_err(tq, sq, sq).max(),
                    sigma=particle_err(sig, ssig, sq).max(), obj=particle_err(obj, sobj, sq).max())
        print(f'  ({n_s},{n_u}) obj {o} con {cm}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        assert all(v <= TOL for v in errs.values()), errs
        np.testing.assert_array_equal(con, scon)
        assert int(r['status'].item()) == int(s['status'].item())
        check_against(r, 0, c.refs[(o, cm)][0], n_s, 'against the oracle')


# ---- more workgroups than compute units -----------------------------------------------------------------------------------------
def test_grid_past_one_pass_repeats_the_first_particles():
    big, horizon = 4099, 3
    c = case(2, 1, horizon=horizon)
    idx = np.arange(big) % P
    rows, gains = c.rows[:, idx], c.gains[:, idx]
    r = launch(c, env_without_gain(c, VAR, ALL_STATES), gains=gains, rows=rows, horizon=horizon)
    assert (big + 15) // 16 > 256
    first = torch.as_tensor(idx[:P], device=r['traj'].device)
    for key in ('traj', 'sigma', 'obj_cost', 'con_cost'):
        out = r[key][0]
        full = out[:(big // P) * P].reshape((big // P, P) + tuple(out.shape[1:]))
        assert torch.equal(full, out[:P][None].expand_as(full)), key
        assert torch.equal(out[(big // P) * P:], out[first[:big % P]]), key
    assert int(r['status'].item()) == 0
    head = {k: (v[:, :P] if k in ('traj', 'sigma', 'obj_cost', 'con_cost') else v) for k, v in r.items()}
    check_against(head, 0, c.refs[(VAR, ALL_STATES)][0], 2, 'P = 4099, the first 37')


# ---- a non-finite gain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u', [(2, 1), (4, 1)])
def test_a_nan_gain_is_reported_and_stays_with_its_particle(n_s, n_u):
    c = case(n_s, n_u)
    env = env_without_gain(c, VAR, ALL_STATES)
    clean = launch(c, env)
    bad, step = 21, 1                      # a particle of the second tile, the gain of step 2
    gains = c.gains.copy()
    gains[0, bad, step, -1, 0] = np.nan
    r = launch(c, env, gains=gains)
    torch.cuda.synchronize()
    assert int(clean['status'].item()) == 0
    assert int(r['status'].item()) & _lib.SX_STATUS_NAN
    others = torch.as_tensor([i for i in range(P) if i != bad], device=r['traj'].device)
    for key in ('traj', 'sigma', 'obj_cost', 'con_cost'):
        assert torch.equal(r[key][0][others], clean[key][0][others]), key
    # the particle itself: as without the NaN up to the step that reads it, NaN shapes from there on
    assert torch.equal(r['traj'][0, bad, :step + 1], clean['traj'][0, bad, :step + 1])
    assert torch.isnan(r['traj'][0, bad, step + 1, n_s:]).any()


# ---- multistep_reachability ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_model(name):
    g, gp = mo.load_golden(os.path.join(GOLDEN, f'multistep_{name}.npz'))
    n_s = g['p_0'].shape[1]
    ssm = rm.constructor('rbf')(state_dimen=n_s, action_dimen=1)
    ssm.set_hyperparameters(g['ls'], g['s'], g['noise'])
    ssm.update_model(T(g['X']), T(g['Y']), replace_old=True)
    return g, gp, ssm


@pytest.mark.parametrize('name', ['pendulum', 'cartpole'])
def test_goldens_through_multistep_reachability(name, monkeypatch):
    from safe_exploration_amd import gp_reachability_pytorch as grp
    g, _, ssm = golden_model(name)
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: counting)
    p_new, q_new, p_all, q_all = grp.multistep_reachability(T(g['p_0']), ssm, T(g['k_fb']), T(g['k_ff']), T(g['l_mu']),
                                                            T(g['l_sigma']), c_safety=float(g['c_safety']), verbose=0,
                                                            a=T(g['a']), b=T(g['b']))
    monkeypatch.undo()
    assert counting.calls['sx_cem_rollout_gains'] == 1
    ep = particle_err(p_all.cpu().numpy(), g['p_all'], g['q_all']).max()
    eq = particle_err(q_all.cpu().numpy(), g['q_all'], g['q_all']).max()
    print(f'{name}: centres {ep:.2e} shapes {eq:.2e} max |Q| {np.abs(g["q_all"]).max():.3g}')
    assert ep <= TOL and eq <= TOL
    assert torch.equal(p_new, p_all[:, -1]) and torch.equal(q_new, q_all[:, -1])


def test_one_launch_then_step_by_step(monkeypatch):
    from safe_exploration_amd import gp_reachability_pytorch as grp
    ssm, gp = model(2, 1)
    sysd = rm.system(2, 1)
    R, n = 5, 3
    rng = np.random.default_rng(3)
    p_0, k_fb, k_ff = rng.normal(0, 0.1, size=(R, 2)), 0.3 * rng.normal(size=(R, n - 1, 1, 2)), rng.normal(0, 0.3, size=(R, n, 1))
    args = (T(p_0), ssm, T(k_fb), T(k_ff), T(sysd['l_mu']), T(sysd['l_sigma']))
    kw = dict(c_safety=sysd['beta'], verbose=0, a=T(sysd['a']), b=T(sysd['b']))
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: counting)
    _, _, p_all, q_all = grp.multistep_reachability(*args, **kw)
    torch.cuda.synchronize()
    assert counting.calls['sx_cem_rollout_gains'] == 1
    assert counting.calls['sx_gp_predict'] == 0 and counting.calls['sx_onestep_reach'] == 0
    counting.calls.clear()
    monkeypatch.setattr(grp, 'fused_gains_form', lambda ssm, n: -1)
    _, _, p_step, q_step = grp.multistep_reachability(*args, **kw)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert counting.calls['sx_cem_rollout_gains'] == 0 and counting.calls['sx_onestep_reach'] == R * n
    ref_p, ref_q, _, status = mo.multistep(gp, p_0, k_fb, k_ff, sysd['l_mu'], sysd['l_sigma'], sysd['beta'], sysd['a'], sysd['b'])
    assert not status.any()
    for what, (gp_, gq_) in dict(fused=(p_all, q_all), stepwise=(p_step, q_step)).items():
        ep = particle_err(gp_.cpu().numpy(), ref_p, ref_q).max()
        eq = particle_err(gq_.cpu().numpy(), ref_q, ref_q).max()
        print(f'{what} against the oracle: centres {ep:.2e} shapes {eq:.2e}')
        assert ep <= TOL and eq <= TOL
    ep = particle_err(p_all.cpu().numpy(), p_step.cpu().numpy(), ref_q).max()
    eq = particle_err(q_all.cpu().numpy(), q_step.cpu().numpy(), ref_q).max()
    print(f'fused against step by step: centres {ep:.2e} shapes {eq:.2e}')
    assert ep <= TOL and eq <= TOL
    # the reference's own shapes
    p1, q1, pa, qa = grp.multistep_reachability(T(p_0[0][:, None]), ssm, T(k_fb[0]), T(k_ff[0]), *args[4:], **kw)
    assert tuple(p1.shape) == (2, 1) and tuple(q1.shape) == (2, 2)
    assert torch.equal(pa, p_all[0]) and torch.equal(qa, q_all[0])


# ---- the runner ---------------------------------------------------------------------------------------------------------------------
class GpMeanEnv(LinearEnv):
    """The scripted linear environment plus the oracle GP's posterior mean: a true system the model's bounds hold for, so
    that some states do lie inside their ellipsoids."""

    def __init__(self, gp):
        super().__init__()
        self.gp = gp

    def simulate_onestep(self, state, action):
        nxt, _ = super().simulate_onestep(state, action)
        z = np.concatenate((np.asarray(state, dtype=np.float64).reshape(-1), np.asarray(action, dtype=np.float64).reshape(-1)))
        nxt = nxt + self.gp.predict(z[None], jacobians=False)[0][0]
        return nxt, nxt


def test_runner_end_to_end(monkeypatch):
    from safe_exploration_amd import uncertainty_propagation_runner as upr
    ssm, gp = model(2, 1)
    env = GpMeanEnv(gp)
    safempc = types.SimpleNamespace(ssm=ssm, lin_model=(env.A, env.B), n_safe=4)
    conf = types.SimpleNamespace(n_rollouts=8, n_safe=4, beta_safety=2.0, verbosity=1, save_results=False, save_path=None)
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: counting)
    np.random.seed(5)
    res = upr.run_uncertainty_propagation(env, safempc, conf)
    monkeypatch.undo()
    assert counting.calls['sx_cem_rollout_gains'] == 1 and counting.calls['sx_onestep_reach'] == 0
    R, n = 8, 4
    np.random.seed(5)
    k_fb, k_ff, x_0 = np.empty((R, n - 1, 1, 2)), np.empty((R, n, 1)), np.empty((R, 2))
    for i in range(R):
        k_fb[i], k_ff[i], x_0[i] = .1 * np.random.randn(n - 1, 1, 2), .1 * np.random.randn(n, 1), 0.1 * np.random.rand(2)
    ref_p, ref_q, _, status = mo.multistep(gp, x_0, k_fb, k_ff, env.l_mu, env.l_sigm, 2.0, env.A, env.B)
    assert not status.any()
    ep, eq = particle_err(res['p_all'], ref_p, ref_q).max(), particle_err(res['q_all'], ref_q, ref_q).max()
    print(f'runner: centres {ep:.2e} shapes {eq:.2e}; inside per step {res["inside_ellipsoid_per_step"].mean(axis=0)}')
    assert ep <= TOL and eq <= TOL
    assert res['x_all'].shape == (R, n + 1, 2) and np.array_equal(res['x_all'][:, 0], x_0)
    for i in range(R):
        for s in range(n):
            d = res['x_all'][i, s + 1] - res['p_all'][i, s]
            assert bool(res['inside_ellipsoid_per_step'][i, s]) == bool(d @ np.linalg.inv(res['q_all'][i, s]) @ d < 1.0)
        assert bool(res['inside_ellipsoid_all'][i]) == bool(res['inside_ellipsoid_per_step'][i].all())
    assert res['inside_ellipsoid_per_step'].any()
