"""GPU: the variance form of the CEM solver's performance trajectory -- sx_cem_perf_rollout_var against the numpy oracle
(tests/perf_var_oracle.py) and against the project's other kernels, its independence of the launch's grid, FusedCemMpc.solve
with perf_variance against a numpy CEM, CemSafeMPC.get_action / DynamicSafeMPCExploration over an objective-less environment.

The kernel cases: shapes (2, 1), (4, 1), (2, 2); N = 7 and 200 (Kstar of all outputs in LDS) and 590 (output by output at
every one of these shapes: n_pad = 608 does not fit with all outputs); E = 2; (n_perf, r) in {(2, 1), (15, 1), (15, 3), (40, 3)};
the drawn and the given-tail form and both objective modes in every case.  P = 37 runs the full cross; P = 4096 + 53 a covering
set (every shape, every N, every n_perf, both r).  Tolerances: rows, means and the affine objective rtol 1e-10, atol 1e-12
(tests/test_gpu_perf_traj.py); perf_sigma and the variance objective rtol 1e-8, atol 1e-11, what tests/test_gpu_parity.py asks
of `sigma` along a chained rollout (the variance is a difference s - |W k*|^2 and does not keep ten digits near training
points).  Every case prints its measured errors before it asserts."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.gp import ExactGP
from perf_var_oracle import cem_solve_perf_var, perf_var_rollout
from safe_exploration_amd import _lib, problems

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 5
SMALL, LARGE = 37, 4096 + 53
SHAPES = [(2, 1), (4, 1), (2, 2)]
SIZES = [7, 200, 590]
HORIZONS = [(2, 1), (15, 1), (15, 3), (40, 3)]      # (n_perf, r)
LARGE_CASES = [(2, 1, 200, 15, 1), (2, 1, 590, 2, 1), (4, 1, 590, 2, 1), (4, 1, 7, 40, 3), (4, 1, 200, 15, 3),
               (2, 2, 7, 40, 3), (2, 2, 200, 2, 1), (2, 2, 590, 15, 1), (2, 1, 7, 15, 3)]
VAR, ABS = _lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS
MODES = {'variance': VAR, 'affine': ABS}
SIGMA_TOL = dict(rtol=1e-8, atol=1e-11)


def T(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def N_(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def close(a, b, rtol=1e-10, atol=1e-12):
    np.testing.assert_allclose(N_(a), N_(b), rtol=rtol, atol=atol)


def worst(a, b, rtol, atol):
    """max of |a - b| / (atol + rtol |b|): <= 1 passes assert_allclose."""
    a, b = N_(a), N_(b)
    return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())


_CASES = {}


def case(n_s, n_u, N):
    """(GpCemSSM on the GPU, {mode: sx_env}, spec, ExactGP, {mode: oracle Problem}): the case of tests/test_gpu_perf_traj.py
    -- a stable random prior, a box |u| <= 1, the separable objective, per-output ARD length-scales -- in both objective
    modes over ONE fitted GP."""
    if (n_s, n_u, N) in _CASES:
        return _CASES[(n_s, n_u, N)]
    rng = np.random.default_rng(1000 + 100 * n_s + 10 * n_u + N)
    X, Y = problems.synthetic_training_set(N, n_s, n_u, seed=N + n_s, scale=0.6, amp=0.05, noise_std=0.002)
    a = 0.85 * np.eye(n_s) + 0.05 * rng.normal(size=(n_s, n_s))
    b = 0.3 * rng.normal(size=(n_s, n_u))
    spec = problems.ProblemSpec('perf_var', n_s, n_u, X, Y, rng.uniform(0.6, 1.4, size=(n_s, n_s + n_u)),
                                rng.uniform(1e-3, 3e-3, size=n_s), rng.uniform(1e-5, 5e-5, size=n_s), a, b,
                                rng.uniform(-0.3, 0.0, size=(n_u, n_s)), np.full(n_s, 0.02), np.full(n_s, 0.02), 2.0,
                                np.vstack((np.eye(n_s), -np.eye(n_s))), np.full((2 * n_s, 1), 2.0), np.full(n_u, -1.0),
                                np.full(n_u, 1.0), obj_mode=ABS)
    spec.obj_w_abs, spec.obj_target = rng.uniform(0.2, 1.0, size=n_s), rng.normal(0, 0.1, size=n_s)
    spec.obj_w_lin = rng.normal(0, 0.2, size=n_s)
    ssm, env = problems.build(spec, device=DEV)
    env_var = _lib.SxEnv.from_buffer_copy(env)
    env_var.obj_mode = VAR
    gp = ExactGP(X, Y, spec.lengthscale, spec.outputscale, spec.noise)
    prob = problems.oracle_problem(spec, ocem)
    probs = {ABS: prob, VAR: dataclasses.replace(prob, obj_mode=ocem.OBJ_NEG_VARIANCE)}
    _CASES[(n_s, n_u, N)] = out = (ssm, {ABS: env, VAR: env_var}, spec, gp, probs)
    return out


def inputs(n_s, n_u, P, n_perf, r, seed):
    rng = np.random.default_rng(seed)
    E, Tl = 2, n_perf - r
    return dict(x0=rng.normal(0, 0.05, size=(E, n_s)), safe=rng.normal(0, 0.5, size=(E, P, H, n_u)),
                mean=rng.normal(0, 0.2, size=(E, Tl, n_u)), std=rng.uniform(0.3, 0.8, size=(E, Tl, n_u)),
                noise=rng.normal(size=(E, P, Tl, n_u)), con0=3.0 * rng.integers(0, 5, size=(E, P)).astype(np.float64))


def launch(ssm, env, inp, n_perf, r, rows=None):
    """The drawn form, or with `rows` the given-tail form.  obj_cost starts as NaN (it is overwritten), con_cost as con0
    (it is added to)."""
    from safe_exploration_amd.cem_mpc import cem_perf_rollout_var
    E, P = inp['safe'].shape[:2]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    obj = torch.full((E, P), float('nan'), dtype=torch.float64, device=DEV)
    kw = (dict(tail_mean=T(inp['mean']), tail_std=T(inp['std']), tail_noise=T(inp['noise'])) if rows is None
          else dict(rows=rows))
    out = cem_perf_rollout_var(ssm, env, T(inp['x0']), H, n_perf, r, safe_actions=T(inp['safe']), obj_cost=obj,
                               con_cost=T(inp['con0']), status=status, want_traj=True, want_sigma=True, **kw)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


def oracle_objective(prob, ref):
    """sum_t oracle.cem.objective_cost(prob, mu_{t+1}, var_t) over the oracle's trajectory, in prob's mode."""
    return sum(ocem.objective_cost(prob, ref.traj[:, t], ref.sigma[:, t]) for t in range(ref.traj.shape[1]))


def check_against_oracle(n_s, n_u, N, P, n_perf, r):
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    inp = inputs(n_s, n_u, P, n_perf, r, seed=n_s + 7 * n_u + N + P + 100 * n_perf + r)
    refs = []
    for e in range(2):
        tail = inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e]
        refs.append(perf_var_rollout(probs[VAR], gp, inp['x0'][e], inp['safe'][e], tail, r))
        assert np.array_equal(refs[e].obj_cost, oracle_objective(probs[VAR], refs[e]))
    assert sum(int(ref.violations.sum()) for ref in refs) > 0, 'no tail action leaves the box'
    outs = {}
    for mode_name, mode in MODES.items():
        drawn = launch(ssm, envs[mode], inp, n_perf, r)
        given_rows = drawn['rows'].clone()
        given_rows[:, :, :H] = float('nan')                  # the safety part of the rows is an output in both forms
        given = launch(ssm, envs[mode], inp, n_perf, r, rows=given_rows)
        for e, ref in enumerate(refs):
            want_obj = oracle_objective(probs[mode], ref)
            obj_tol = SIGMA_TOL if mode == VAR else dict(rtol=1e-10, atol=1e-12)
            for name, out in (('drawn', drawn), ('given', given)):
                print(f'({n_s},{n_u}) N={N} P={P} n_perf={n_perf} r={r} e={e} {mode_name} {name}: '
                      f'max |traj - oracle| = {float(np.abs(N_(out["perf_traj"][e]) - ref.traj).max()):.3e}, '
                      f'max |sigma - oracle| = {float(np.abs(N_(out["perf_sigma"][e]) - ref.sigma).max()):.3e} '
                      f'({worst(out["perf_sigma"][e], ref.sigma, **SIGMA_TOL):.3f} of the tolerance; smallest variance '
                      f'{ref.sigma.min():.3e}), max |obj - oracle| = '
                      f'{float(np.abs(N_(out["obj_cost"][e]) - want_obj).max()):.3e} '
                      f'({worst(out["obj_cost"][e], want_obj, **obj_tol):.3f} of the tolerance)')
                close(out['rows'][e], ref.rows)
                close(out['perf_traj'][e], ref.traj)
                close(out['perf_sigma'][e], ref.sigma, **SIGMA_TOL)
                close(out['obj_cost'][e], want_obj, **obj_tol)
                close(out['con_cost'][e] - T(inp['con0'][e]), ref.con_cost, rtol=0, atol=0)
            assert torch.equal(drawn['rows'][e, :, :H], T(inp['safe'][e]))           # the shared actions: bit-identical
        # the two forms see the same tail bits
        for name in ('perf_traj', 'perf_sigma', 'obj_cost', 'con_cost'):
            assert torch.equal(drawn[name], given[name]), name
        outs[mode] = drawn
    # the objective mode changes the objective only
    for name in ('rows', 'perf_traj', 'perf_sigma', 'con_cost'):
        assert torch.equal(outs[VAR][name], outs[ABS][name]), name
    return inp, outs


@pytest.mark.parametrize('n_perf,r', HORIZONS)
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_kernel_matches_the_oracle(n_s, n_u, N, n_perf, r):
    check_against_oracle(n_s, n_u, N, SMALL, n_perf, r)


@pytest.mark.parametrize('n_s,n_u,N,n_perf,r', LARGE_CASES)
def test_kernel_matches_the_oracle_past_one_grid_and_does_not_depend_on_it(n_s, n_u, N, n_perf, r):
    """P = 4096 + 53 per problem, against the oracle; then the first 37 particles of each problem in a launch of their own
    give bit-identical rows, means, variances and costs."""
    inp, big = check_against_oracle(n_s, n_u, N, LARGE, n_perf, r)
    ssm, envs = case(n_s, n_u, N)[:2]
    sub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in inp.items()}
    for mode in MODES.values():
        small = launch(ssm, envs[mode], sub, n_perf, r)
        for name in ('rows', 'perf_traj', 'perf_sigma', 'obj_cost', 'con_cost'):
            assert torch.equal(small[name], big[mode][name][:, :SMALL]), name


def test_the_forms_the_training_sets_take():
    """N = 200 runs with all outputs in LDS and 590 output by output (sx_cem_rollout_form reports the streaming safety
    kernel's choice, made by the same rule at the same LDS budget); N = 1100 (n_pad = 1104) has no form.  1024 is not the
    limit the form query answers for n_s > 1: one output's Kstar and the training inputs fill the LDS before n_pad = 1024,
    and sooner the longer the trajectory (tests/test_gpu_perf_shapes.py finds the largest N of every shape: 988 here)."""
    from safe_exploration_amd.cem_mpc import cem_perf_rollout_var
    form = lambda ssm: int(_lib.lib().sx_cem_rollout_form(ssm.device_model, 40))
    SX_FORM_BYOUT = 3
    for n_s, n_u in SHAPES:
        assert form(case(n_s, n_u, 590)[0]) == SX_FORM_BYOUT
        assert form(case(n_s, n_u, 200)[0]) != SX_FORM_BYOUT
    ssm, envs = case(2, 1, 1100)[:2]
    inp = inputs(2, 1, SMALL, 2, 1, seed=1)
    with pytest.raises(_lib.SxError, match='no form'):
        cem_perf_rollout_var(ssm, envs[VAR], T(inp['x0']), H, 2, 1, safe_actions=T(inp['safe']),
                             obj_cost=torch.empty((2, SMALL), dtype=torch.float64, device=DEV), con_cost=T(inp['con0']),
                             status=torch.zeros(1, dtype=torch.int32, device=DEV), tail_mean=T(inp['mean']),
                             tail_std=T(inp['std']), tail_noise=T(inp['noise']))


# ---- against the project's other kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_against_the_mean_only_kernel_the_safety_rollout_and_gp_predict(n_s, n_u, N):
    from safe_exploration_amd.cem_mpc import cem_perf_rollout, cem_rollout
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    n_perf, r = 15, 1
    inp = inputs(n_s, n_u, SMALL, n_perf, r, seed=5 + n_s + N)
    var = launch(ssm, envs[ABS], inp, n_perf, r)
    E, P = 2, SMALL
    # the means and the affine objective: sx_cem_perf_rollout sums k* . alpha in another order
    obj = torch.full((E, P), float('nan'), dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    mean_only = cem_perf_rollout(ssm, envs[ABS], T(inp['x0']), H, n_perf, r, safe_actions=T(inp['safe']), obj_cost=obj,
                                 con_cost=T(inp['con0']), status=status, tail_mean=T(inp['mean']), tail_std=T(inp['std']),
                                 tail_noise=T(inp['noise']), want_traj=True)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert torch.equal(var['rows'], mean_only['rows']) and torch.equal(var['con_cost'], mean_only['con_cost'])
    close(var['perf_traj'], mean_only['perf_traj'])
    close(var['obj_cost'], mean_only['obj_cost'])
    # var_0 is the variance the safety rollout stores for its first step from the same point (point branch, before any
    # fix-up: the oracle's variances are all positive here, so no zero fix is in play)
    for e in range(E):
        tail = inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e]
        assert perf_var_rollout(probs[VAR], gp, inp['x0'][e], inp['safe'][e], tail, r).sigma.min() > 0
    safety = cem_rollout(ssm, envs[ABS], T(inp['x0']), H, actions=T(inp['safe']), want_sigma=True)
    torch.cuda.synchronize()
    print(f'({n_s},{n_u}) N={N}: max |var_0 - safety sigma_0| = '
          f'{float((var["perf_sigma"][:, :, 0] - safety["sigma"][:, :, 0]).abs().max()):.3e}')
    close(var['perf_sigma'][:, :, 0], safety['sigma'][:, :, 0], **SIGMA_TOL)
    # per step: sx_gp_predict's variance (and mean) at the recorded [mu_t, v_t]
    mu = torch.cat([T(inp['x0'])[:, None, None, :].expand(E, P, 1, n_s), var['perf_traj'][:, :, :-1]], dim=2)
    v = torch.cat([var['rows'][:, :, :r], var['rows'][:, :, H:]], dim=2)
    mean_p, var_p = ssm.predict_without_jacobians(mu.reshape(-1, n_s).contiguous(), v.reshape(-1, n_u).contiguous())
    torch.cuda.synchronize()
    print(f'({n_s},{n_u}) N={N}: max |perf_sigma - sx_gp_predict| = '
          f'{float((var["perf_sigma"].reshape(-1, n_s) - var_p).abs().max()):.3e}')
    close(var['perf_sigma'].reshape(-1, n_s), var_p, **SIGMA_TOL)
    a, b = T(spec.a), T(spec.b)
    close(var['perf_traj'].reshape(-1, n_s), mu.reshape(-1, n_s) @ a.t() + v.reshape(-1, n_u) @ b.t() + mean_p)


# ---- the whole solve -------------------------------------------------------------------------------------------------------
SOLVE = dict(H=5, n_perf=15, r=1, P=512, k=50, iters=4, init_std=0.2, seed=0)
GAP = 1e-5      # 1000 x the variance tolerance


def pendulum():
    spec = problems.pendulum(n_train=200, seed=0, obj_mode=VAR)
    return spec, ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)


def decided(con, obj, i, j):
    """Do candidates i and j differ in constraint cost, or by a relative objective gap of at least GAP?"""
    return con[i] != con[j] or abs(obj[i] - obj[j]) >= GAP * max(abs(obj[i]), abs(obj[j]))


def test_solve_with_the_variance_objective_matches_the_numpy_cem():
    """The comparison means something only where no decision hangs on the tolerance: the conditions are asserted on the
    ORACLE's values before the GPU is touched.  Noise seed 0 passes all of them, the rank-1 / rank-2 gap of the last
    iteration included."""
    from safe_exploration_amd.cem_mpc import FusedCemMpc
    c = SOLVE
    spec, gp = pendulum()
    prob = problems.oracle_problem(spec, ocem)
    assert prob.obj_mode == ocem.OBJ_NEG_VARIANCE
    steps = c['H'] + c['n_perf'] - c['r']
    noise = np.random.default_rng(c['seed']).normal(size=(c['iters'], c['P'], steps, 1))
    x0 = np.array([0.02, -0.03])
    ref_best, trace = cem_solve_perf_var(prob, gp, x0, noise, c['k'], c['H'], c['n_perf'], c['r'], c['init_std'])
    assert ref_best is not None, 'the oracle\'s last iteration does not end feasible'
    for it, (con, obj, idx, var_min) in enumerate(trace):
        order = ocem.rank(con, obj, c['k'] + 1)
        gap = abs(obj[order[-2]] - obj[order[-1]]) / max(abs(obj[order[-2]]), abs(obj[order[-1]]))
        print(f'iteration {it}: {int((con == 0).sum())} feasible, elite boundary gap {gap:.2e} (relative), smallest variance '
              f'{var_min:.3e}')
        assert var_min > 0
        assert decided(con, obj, order[-2], order[-1]), f'iteration {it}: the elite set hangs on the tolerance'
    con, obj, idx, _ = trace[-1]
    order = ocem.rank(con, obj, 2)
    print(f'last iteration: rank 1 / rank 2 gap '
          f'{abs(obj[order[0]] - obj[order[1]]) / max(abs(obj[order[0]]), abs(obj[order[1]])):.2e} (relative)')
    assert decided(con, obj, order[0], order[1]), 'the best row hangs on the tolerance: choose another seed'
    ssm, env = problems.build(spec, device=DEV)
    mpc = FusedCemMpc(ssm, env, c['H'], c['P'], c['k'], c['iters'], device=DEV, init_std=c['init_std'],
                      n_perf=c['n_perf'], perf_r=c['r'], perf_variance=True)
    best, ok, _, status = mpc.solve(T(x0[None]), noise=T(noise[:, None]))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert bool(ok[0].item())
    assert tuple(best.shape) == (1, steps, 1)
    print(f'best row: max |device - numpy CEM| = {float(np.abs(N_(best[0]) - ref_best).max()):.3e}')
    close(best[0], ref_best, rtol=0, atol=1e-9)


def test_recorded_rollouts_keep_the_variances():
    from safe_exploration_amd.cem_mpc import FusedCemMpc
    spec, _ = pendulum()
    ssm, env = problems.build(spec, device=DEV)
    mpc = FusedCemMpc(ssm, env, 5, 64, 8, 2, device=DEV, init_std=0.2, n_perf=6, perf_variance=True, record_rollouts=True)
    _, _, history, status = mpc.solve(T(np.array([[0.02, -0.03]])))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and len(history) == 2
    for h in history:
        assert tuple(h.perf_sigma.shape) == tuple(h.perf_trajectories.shape) == (64, 6, 2)
        close(h.objective_costs, -h.perf_sigma.sum(dim=(1, 2)), **SIGMA_TOL)


def test_without_the_setting_the_solve_is_the_parents():
    """perf_variance absent and perf_variance=False, with and without a performance trajectory: bit-identical best rows."""
    from safe_exploration_amd.cem_mpc import FusedCemMpc
    spec = problems.pendulum(n_train=200, seed=0, obj_mode=ABS)
    ssm, env = problems.build(spec, device=DEV)
    P, k, iters = 512, 50, 4
    x0 = T(np.array([[0.02, -0.03]]))
    for kw, steps in ((dict(), H), (dict(n_perf=15, perf_r=1), H + 14)):
        noise = T(np.random.default_rng(1).normal(size=(iters, 1, P, steps, 1)))
        a = FusedCemMpc(ssm, env, H, P, k, iters, device=DEV, init_std=0.2, **kw).solve(x0, noise=noise)
        b = FusedCemMpc(ssm, env, H, P, k, iters, device=DEV, init_std=0.2, perf_variance=False, **kw).solve(x0, noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[0].shape) == (1, steps, 1)


class Conf:
    mpc_time_horizon = 5
    cem_num_rollouts = 512
    cem_num_elites = 50
    cem_num_iterations = 4
    cem_init_std = 0.2
    cem_n_perf = 10
    cem_perf_variance = True
    plot_cem_optimisation = False
    plot_cem_terminal_states = False
    device = DEV
    use_state_constraint = True
    use_prior_model = True
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'


def test_get_action_and_find_max_variance_over_an_exploration_environment():
    from safe_exploration_amd.safempc_cem import MpcResult
    from safe_exploration_amd.safempc_exploration import DynamicSafeMPCExploration
    spec = problems.pendulum(n_train=200, seed=0)
    env = problems.StubEnv(spec, np.zeros(2))                       # no objective: the solver explores
    assert env.objective_cost_function(torch.zeros((1, 2), dtype=torch.float64)) is None
    solver, _ = problems.make_solver(spec, Conf(), env, device=DEV)
    assert solver.performance_trajectory_length == 10
    x0 = np.array([0.02, -0.03])
    action, result = solver.get_action(x0)
    assert action.shape == (1,) and result == MpcResult.FOUND_SOLUTION
    assert solver._last_mpc_actions.shape == (Conf.mpc_time_horizon, 1)
    mpc = solver._solver()
    assert mpc._perf.variance and mpc._env.obj_mode == VAR and mpc._objective_hook is None
    assert tuple(mpc.last_perf_actions.shape) == (1, 10 - 1, 1) and mpc.last_status == 0
    explorer = DynamicSafeMPCExploration(solver, env)
    assert (explorer.n_safe, explorer.n_perf) == (5, 10)
    x, u = explorer.find_max_variance(x0)
    assert x.shape == (2, 1) and u.shape == (1, 1)
    assert np.array_equal(u[:, 0], solver._last_mpc_actions[0]) and mpc.last_status == 0
    xs, us, results = explorer.find_max_variance_batch(np.stack([x0, x0]))
    assert xs.shape == (2, 2) and us.shape == (2, 1) and len(results) == 2
    assert all(res == MpcResult.FOUND_SOLUTION for res in results)
    assert tuple(mpc.last_perf_actions.shape) == (2, 10 - 1, 1)
