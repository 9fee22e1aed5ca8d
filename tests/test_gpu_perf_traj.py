"""GPU: the performance trajectory of the CEM solver -- sx_cem_perf_rollout against the numpy oracle
(tests/perf_traj_oracle.py), its independence of the launch's grid, its first mean against the safety kernel's first
centre, FusedCemMpc.solve with a performance trajectory against a numpy CEM, and CemSafeMPC.get_action with cem_n_perf.

The kernel cases: shapes (2, 1), (4, 1), (2, 2); N = 7, 200 and 590 (more than one pass of a lane's stride over the
training points, and not a multiple of it); E = 2; n_perf in {2, 15, 40} with r in {1, 3} (n_perf > r); both the drawn and
the given-tail form in every case.  P = 37 runs the full cross of these; P = 4096 + 53 runs a covering set (every shape,
every N, every n_perf, both r) whose oracle -- ExactGP.predict computes the N x N variance product it does not need -- stays
within seconds.  Tolerance: 1e-10 relative (atol 1e-12), that of tests/test_gpu_junk_fused.py."""
import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.gp import ExactGP
from perf_traj_oracle import cem_solve_perf, perf_rollout
from safe_exploration_amd import _lib, problems

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 5
SMALL, LARGE = 37, 4096 + 53
SHAPES = [(2, 1), (4, 1), (2, 2)]
HORIZONS = [(2, 1), (15, 1), (15, 3), (40, 1), (40, 3)]      # (n_perf, r)
LARGE_CASES = [(2, 1, 200, 15, 1), (2, 1, 590, 2, 1), (4, 1, 590, 2, 1), (4, 1, 7, 40, 1), (4, 1, 200, 15, 3),
               (2, 2, 7, 40, 3), (2, 2, 200, 2, 1), (2, 2, 590, 15, 1), (2, 1, 7, 15, 3)]


def T(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def close(a, b, rtol=1e-10, atol=1e-12):
    np.testing.assert_allclose(a.cpu().numpy() if torch.is_tensor(a) else a, b.cpu().numpy() if torch.is_tensor(b) else b,
                               rtol=rtol, atol=atol)


_CASES = {}


def case(n_s, n_u, N):
    """(GpCemSSM on the GPU, sx_env, spec, ExactGP, oracle Problem): a stable random prior, a box |u| <= 1, the separable
    objective, and a GP with per-output ARD length-scales."""
    if (n_s, n_u, N) in _CASES:
        return _CASES[(n_s, n_u, N)]
    rng = np.random.default_rng(1000 + 100 * n_s + 10 * n_u + N)
    X, Y = problems.synthetic_training_set(N, n_s, n_u, seed=N + n_s, scale=0.6, amp=0.05, noise_std=0.002)
    a = 0.85 * np.eye(n_s) + 0.05 * rng.normal(size=(n_s, n_s))
    b = 0.3 * rng.normal(size=(n_s, n_u))
    spec = problems.ProblemSpec('perf', n_s, n_u, X, Y, rng.uniform(0.6, 1.4, size=(n_s, n_s + n_u)),
                                rng.uniform(1e-3, 3e-3, size=n_s), rng.uniform(1e-5, 5e-5, size=n_s), a, b,
                                rng.uniform(-0.3, 0.0, size=(n_u, n_s)), np.full(n_s, 0.02), np.full(n_s, 0.02), 2.0,
                                np.vstack((np.eye(n_s), -np.eye(n_s))), np.full((2 * n_s, 1), 2.0), np.full(n_u, -1.0),
                                np.full(n_u, 1.0), obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    spec.obj_w_abs, spec.obj_target = rng.uniform(0.2, 1.0, size=n_s), rng.normal(0, 0.1, size=n_s)
    spec.obj_w_lin = rng.normal(0, 0.2, size=n_s)
    ssm, env = problems.build(spec, device=DEV)
    gp = ExactGP(X, Y, spec.lengthscale, spec.outputscale, spec.noise)
    _CASES[(n_s, n_u, N)] = out = (ssm, env, spec, gp, problems.oracle_problem(spec, ocem))
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
    from safe_exploration_amd.cem_mpc import cem_perf_rollout
    E, P = inp['safe'].shape[:2]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    obj = torch.full((E, P), float('nan'), dtype=torch.float64, device=DEV)
    kw = (dict(tail_mean=T(inp['mean']), tail_std=T(inp['std']), tail_noise=T(inp['noise'])) if rows is None
          else dict(rows=rows))
    out = cem_perf_rollout(ssm, env, T(inp['x0']), H, n_perf, r, safe_actions=T(inp['safe']), obj_cost=obj,
                           con_cost=T(inp['con0']), status=status, want_traj=True, **kw)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


def check_against_oracle(n_s, n_u, N, P, n_perf, r):
    ssm, env, spec, gp, prob = case(n_s, n_u, N)
    inp = inputs(n_s, n_u, P, n_perf, r, seed=n_s + 7 * n_u + N + P + 100 * n_perf + r)
    drawn = launch(ssm, env, inp, n_perf, r)
    given_rows = drawn['rows'].clone()
    given_rows[:, :, :H] = float('nan')                      # the safety part of the rows is an output in both forms
    given = launch(ssm, env, inp, n_perf, r, rows=given_rows)
    violations = 0
    for e in range(2):
        tail = inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e]
        ref = perf_rollout(prob, gp, inp['x0'][e], inp['safe'][e], tail, r)
        violations += int(ref.violations.sum())
        for name, out in (('drawn', drawn), ('given', given)):
            err = float(np.abs(out['perf_traj'][e].cpu().numpy() - ref.traj).max())
            print(f'({n_s},{n_u}) N={N} P={P} n_perf={n_perf} r={r} e={e} {name}: max |traj - oracle| = {err:.3e}, '
                  f'max |obj - oracle| = {float(np.abs(out["obj_cost"][e].cpu().numpy() - ref.obj_cost).max()):.3e}')
            close(out['rows'][e], ref.rows)
            close(out['perf_traj'][e], ref.traj)
            close(out['obj_cost'][e], ref.obj_cost)
            close(out['con_cost'][e] - T(inp['con0'][e]), ref.con_cost, rtol=0, atol=0)
        assert torch.equal(drawn['rows'][e, :, :H], T(inp['safe'][e]))           # the shared actions: bit-identical
    assert violations > 0, 'no tail action leaves the box: the constraint increment is not tested'
    # the two forms see the same tail bits
    assert torch.equal(drawn['perf_traj'], given['perf_traj']) and torch.equal(drawn['obj_cost'], given['obj_cost'])
    return inp, drawn


@pytest.mark.parametrize('n_perf,r', HORIZONS)
@pytest.mark.parametrize('N', [7, 200, 590])
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_kernel_matches_the_oracle(n_s, n_u, N, n_perf, r):
    check_against_oracle(n_s, n_u, N, SMALL, n_perf, r)


@pytest.mark.parametrize('n_s,n_u,N,n_perf,r', LARGE_CASES)
def test_kernel_matches_the_oracle_past_one_grid_and_does_not_depend_on_it(n_s, n_u, N, n_perf, r):
    """P = 4096 + 53 per problem, against the oracle; then the first 37 particles of each problem in a launch of their own
    give bit-identical rows, means and costs."""
    inp, big = check_against_oracle(n_s, n_u, N, LARGE, n_perf, r)
    ssm, env = case(n_s, n_u, N)[:2]
    sub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in inp.items()}
    small = launch(ssm, env, sub, n_perf, r)
    for name in ('rows', 'perf_traj', 'obj_cost', 'con_cost'):
        assert torch.equal(small[name], big[name][:, :SMALL]), name


@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_first_mean_is_the_safety_kernels_first_centre(n_s, n_u):
    """r = 1: mu_1 and the safety rollout's first centre are a x + b u + mean at the same point, from two kernels."""
    from safe_exploration_amd.cem_mpc import cem_rollout
    ssm, env = case(n_s, n_u, 200)[:2]
    inp = inputs(n_s, n_u, SMALL, 15, 1, seed=5 + n_s)
    perf = launch(ssm, env, inp, 15, 1)
    safety = cem_rollout(ssm, env, T(inp['x0']), H, actions=T(inp['safe']), want_traj=True)
    torch.cuda.synchronize()
    close(perf['perf_traj'][:, :, 0, :], safety['traj'][:, :, 0, :n_s])


# ---- the whole solve -------------------------------------------------------------------------------------------------------
SOLVE = dict(H=5, n_perf=15, r=1, P=512, k=50, iters=4, init_std=0.2, seed=0)     # seed 0: feasible, no ties (checked below)


def pendulum():
    spec = problems.pendulum(n_train=200, seed=0, obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    return spec, ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)


def test_solve_with_a_performance_trajectory_matches_the_numpy_cem():
    from safe_exploration_amd.cem_mpc import FusedCemMpc
    c = SOLVE
    spec, gp = pendulum()
    prob = problems.oracle_problem(spec, ocem)
    steps = c['H'] + c['n_perf'] - c['r']
    noise = np.random.default_rng(c['seed']).normal(size=(c['iters'], c['P'], steps, 1))
    x0 = np.array([0.02, -0.03])
    ref_best, trace = cem_solve_perf(prob, gp, x0, noise, c['k'], c['H'], c['n_perf'], c['r'], c['init_std'])
    # the comparison means something only if the oracle's solve ends feasible and no elite set hangs on a tie
    con, obj, idx = trace[-1]
    assert ref_best is not None and int((con == 0).sum()) >= 1
    for con, obj, idx in trace:
        order = ocem.rank(con, obj, c['k'] + 1)
        pairs = [(con[i], obj[i]) for i in order]
        assert len(set(pairs)) == len(pairs), 'ties in (con, obj) among the elites: choose another seed'
    ssm, env = problems.build(spec, device=DEV)
    mpc = FusedCemMpc(ssm, env, c['H'], c['P'], c['k'], c['iters'], device=DEV, init_std=c['init_std'],
                      n_perf=c['n_perf'], perf_r=c['r'])
    best, ok, _, status = mpc.solve(T(x0[None]), noise=T(noise[:, None]))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert bool(ok[0].item()) == (ref_best is not None)
    assert tuple(best.shape) == (1, steps, 1)
    err = float(np.abs(best[0].cpu().numpy() - ref_best).max())
    print(f'best row: max |device - numpy CEM| = {err:.3e}')
    close(best[0], ref_best, rtol=0, atol=1e-9)


def test_without_the_setting_the_solve_is_the_parents():
    """n_perf absent and n_perf = 0: bit-identical best actions (and no performance launch: tests/test_perf_traj_host.py)."""
    from safe_exploration_amd.cem_mpc import FusedCemMpc
    spec, _ = pendulum()
    ssm, env = problems.build(spec, device=DEV)
    P, k, iters = 512, 50, 4
    noise = T(np.random.default_rng(1).normal(size=(iters, 1, P, H, 1)))
    x0 = T(np.array([[0.02, -0.03]]))
    a = FusedCemMpc(ssm, env, H, P, k, iters, device=DEV, init_std=0.2).solve(x0, noise=noise)
    b = FusedCemMpc(ssm, env, H, P, k, iters, device=DEV, init_std=0.2, n_perf=0).solve(x0, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[0].shape) == (1, H, 1)


def test_objective_hook_is_evaluated_on_the_performance_trajectory():
    """The same objective through the hook (torch, on the recorded means) and through the kernel selects the same row."""
    from safe_exploration_amd.cem_mpc import FusedCemMpc
    c = SOLVE
    spec, _ = pendulum()
    ssm, env = problems.build(spec, device=DEV)
    noise = T(np.random.default_rng(c['seed']).normal(size=(c['iters'], 1, c['P'], c['H'] + c['n_perf'] - c['r'], 1)))
    x0 = T(np.array([[0.02, -0.03]]))
    best = []
    for hook in (None, lambda p: torch.abs(spec.obj_target[1] - p[:, 1])):
        mpc = FusedCemMpc(ssm, env, c['H'], c['P'], c['k'], c['iters'], device=DEV, init_std=c['init_std'],
                          n_perf=c['n_perf'], perf_r=c['r'])
        mpc.set_env(env, objective_hook=hook)
        b, ok, _, status = mpc.solve(x0, noise=noise)
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and bool(ok[0].item())
        best.append(b)
    close(best[0], best[1], rtol=0, atol=1e-9)


class Conf:
    mpc_time_horizon = 5
    cem_num_rollouts = 512
    cem_num_elites = 50
    cem_num_iterations = 4
    cem_init_std = 0.2
    cem_n_perf = 10
    plot_cem_optimisation = False
    plot_cem_terminal_states = False
    device = DEV
    use_state_constraint = True
    use_prior_model = True
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'


def test_get_action_with_a_performance_trajectory():
    from safe_exploration_amd.safempc_cem import MpcResult
    spec = problems.pendulum(n_train=200, seed=0, obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=-0.1)
    solver, _ = problems.make_solver(spec, Conf(), env, device=DEV)
    assert solver.performance_trajectory_length == 10
    action, result = solver.get_action(np.array([0.02, -0.03]))
    assert action.shape == (1,) and result == MpcResult.FOUND_SOLUTION
    assert solver._last_mpc_actions.shape == (Conf.mpc_time_horizon, 1)
    mpc = solver._solver()
    assert tuple(mpc.last_perf_actions.shape) == (1, 10 - 1, 1) and mpc.last_status == 0
