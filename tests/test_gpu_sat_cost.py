"""GPU: the PILCO saturating cost as a kernel objective -- sx_sat_cost_eval against the numpy oracle
(tests/sat_cost_oracle.py: the reference's inverse / determinant form over the materialised augmented covariance, which the
kernels never form), the three _sat rollouts against their parent entries (everything but obj_cost bit for bit), against the
oracle's cost of the kernel's own traj / cov and against the oracle's rollout, their independence of the launch's grid, a
cautious and a Taylor-performance solve with the reference's cart-pole constants against the numpy CEM, and
CautiousCemMPC / CemSafeMPC.get_action after init_solver(SaturatingCost).

Shapes: P = 37 (three tiles, the last one partial), E = 2; (n_s, n_u, N) in {(2,1,7), (2,1,200), (4,1,200), (4,1,590: output
by output), (2,2,200)}; 3 and 15 steps.  The other compiled shapes -- (3,1), (1,1), (4,2) at N = 7, 200, 590 --, (2,1) and
(2,2) output by output, and costs without an angle, with the angle first or last and of rank 1 are in
tests/test_gpu_cost_shapes.py.
Tolerances.  The loss lies in [0, 1] and is under 200 flops plus three library calls of a few ulp on inputs that keep the
exponent q below 50: 1e-12 absolute for sx_sat_cost_eval, and 1e-12 per step summed for a rollout's obj_cost against the
oracle's cost of the kernel's OWN traj / cov (the same formula on the same inputs).  Against the oracle's rollout obj_cost is
held to SIGMA_TOL of tests/test_gpu_perf_var.py: a smooth bounded function of covariances held to that tolerance.  Constraint
costs exactly; a solve's best row within 1e-9 (test_solve_matches_the_numpy_cem).  Every case prints its worst error before it
asserts.  Measured figures: DESIGN.md section 3.12."""
from unittest import mock

import numpy as np
import pytest
import torch

import sat_cost_oracle as so
import test_gpu_perf_multi as multi
from cautious_oracle import cautious_rollout
from oracle import cem as ocem
from perf_taylor_oracle import perf_taylor_rollout
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.costs import SaturatingCost
from test_gpu_cautious import Conf as CautiousConf
from test_gpu_cautious import OUTPUTS as CAUTIOUS_OUTPUTS
from test_gpu_cautious import drawn_rows, make_cautious, rows_inputs
from test_gpu_perf_taylor import Conf as TaylorConf
from test_gpu_perf_taylor import OUTPUTS as TAYLOR_OUTPUTS
from test_gpu_perf_taylor import tails
from test_gpu_perf_var import ABS, DEV, H, SIGMA_TOL, VAR, N_, T, case, close, inputs, worst
from test_sat_cost_host import SOLVE, SOLVE_X0, oracle_solve, random_spd, random_weight, solve_case

pytestmark = pytest.mark.gpu
SMALL, LARGE = 37, 4096 + 53
CASES = [(2, 1, 7), (2, 1, 200), (4, 1, 200), (4, 1, 590), (2, 2, 200)]
MULTI_CASES = [(2, 1, (7, 200)), (2, 1, (200, 100)), (4, 1, (200, 100)), (4, 1, (590, 200)), (2, 2, (200, 100))]
STEPS = [3, 15]
LOSS_TOL = 1e-12


def cost_for(n_s):
    """(SaturatingCost, its oracle twin): the reference's cart-pole constants at n_s = 4; at n_s = 2 the angle is state 1 and
    the weight a full-rank non-diagonal one."""
    if n_s == 4:
        z, w, i = so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, so.CARTPOLE_TRIG_IDX
    else:
        rng = np.random.default_rng(77)
        z, w, i = np.array([0.4, 0.1, 0.9]), random_weight(rng, 3, 3) * 0.4, 1
    return SaturatingCost(z, w, i), so.Cost(z, w, i)


# ---- the cost alone ----------------------------------------------------------------------------------------------------------
EVAL = [(2, 0, 1), (2, 1, 3), (2, -1, 2), (4, 2, 2), (4, 2, 5), (1, 0, 2), (3, -1, 3)]


def eval_case(n_s, trig_idx, rank):
    rng = np.random.default_rng(50 + 10 * n_s + rank)
    n_a = n_s + (trig_idx >= 0)
    if (n_s, trig_idx, rank) == (4, 2, 2):
        z, w = so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT
    else:
        z, w = rng.normal(0, 0.5, size=n_a), random_weight(rng, n_a, rank) * 0.5
    i = None if trig_idx < 0 else trig_idx
    mu = rng.normal(0, 1.0, size=(SMALL, n_s))
    cov = np.stack([random_spd(rng, n_s, rng.uniform(0.01, 0.5)) for _ in range(SMALL)])
    cov[0] = 0.0                                              # a point
    cov[1] = np.diag(rng.uniform(0.01, 0.1, size=n_s))
    cov[1, max(trig_idx, 0), max(trig_idx, 0)] = 50.0         # e0, e1 -> 0 on the angle
    return SaturatingCost(z, w, i), so.Cost(z, w, i), mu, cov


@pytest.mark.parametrize('n_s,trig_idx,rank', EVAL)
def test_eval_matches_the_oracle(n_s, trig_idx, rank):
    cost, twin, mu, cov = eval_case(n_s, trig_idx, rank)
    assert cost.rank == rank
    want = so.losses(twin, mu, cov)
    assert np.isfinite(want).all() and want.min() >= 0 and want.max() <= 1 and want.max() - want.min() > 0.1
    assert -2 * np.log1p(-want).max() < 50                   # (q <= -2 log(1 - loss): the exponent stays below 50)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = cost.evaluate_device(T(mu), T(cov), status)
    torch.cuda.synchronize()
    print(f'n_s={n_s} trig_idx={trig_idx} rank={rank}: max |device - oracle| = {np.abs(N_(got) - want).max():.3e}, '
          f'against SaturatingCost.__call__ on the device {float((got - cost(T(mu), T(cov))).abs().max()):.3e}')
    assert int(status.item()) == 0
    assert np.abs(N_(got) - want).max() <= LOSS_TOL
    assert float((got - cost(T(mu), T(cov))).abs().max()) <= LOSS_TOL
    # a NaN row sets the status and is NaN alone
    bad = mu.copy()
    bad[5, n_s - 1] = np.nan
    status.zero_()
    nan = cost.evaluate_device(T(bad), T(cov), status)
    torch.cuda.synchronize()
    assert int(status.item()) == _lib.SX_STATUS_NAN and bool(torch.isnan(nan[5]))
    keep = [p for p in range(SMALL) if p != 5]
    assert torch.equal(nan[keep], got[keep])


# ---- the rollouts ------------------------------------------------------------------------------------------------------------
def own_cost(twin, traj, cov):
    """The oracle's trajectory cost of a kernel's own means and covariances [P x T x ...] -> [P]."""
    return so.losses(twin, N_(traj), N_(cov)).sum(axis=1)


def check_objective(label, twin, obj, traj, cov, ref, steps):
    own, oracle = own_cost(twin, traj, cov), so.trajectory_cost(twin, ref)
    print(f'{label}: obj_cost against the oracle\'s cost of the kernel\'s own traj / cov {np.abs(N_(obj) - own).max():.3e} '
          f'(tolerance {LOSS_TOL * steps:.1e}); against the oracle\'s rollout {worst(obj, oracle, **SIGMA_TOL):.3f} of SIGMA_TOL; '
          f'objective in [{oracle.min():.3f}, {oracle.max():.3f}]')
    assert oracle.max() - oracle.min() > 1e-3, 'the objective does not tell the particles apart'
    assert np.abs(N_(obj) - own).max() <= LOSS_TOL * steps
    close(obj, oracle, **SIGMA_TOL)


def launch_taylor(ssm, env, inp, n_perf, r, cost=None):
    E, P = inp['safe'].shape[:2]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    obj = torch.full((E, P), float('nan'), dtype=torch.float64, device=DEV)
    out = cem_mpc.cem_perf_rollout_taylor(ssm, env, T(inp['x0']), H, n_perf, r, safe_actions=T(inp['safe']), obj_cost=obj,
                                          con_cost=T(inp['con0']), status=status, want_traj=True, want_sigma=True,
                                          want_cov=True, tail_mean=T(inp['mean']), tail_std=T(inp['std']),
                                          tail_noise=T(inp['noise']), **({} if cost is None else dict(cost=cost)))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


@pytest.mark.parametrize('steps', STEPS)
@pytest.mark.parametrize('n_s,n_u,N', CASES)
def test_taylor_sat_rollout(n_s, n_u, N, steps):
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    cost, twin = cost_for(n_s)
    inp = inputs(n_s, n_u, SMALL, steps, 1, seed=n_s + 7 * n_u + N + steps)
    parent, sat = launch_taylor(ssm, envs[ABS], inp, steps, 1), launch_taylor(ssm, envs[ABS], inp, steps, 1, cost)
    for name in TAYLOR_OUTPUTS:
        if name != 'obj_cost':
            assert torch.equal(parent[name], sat[name]), name
    assert torch.equal(sat['obj_cost'], launch_taylor(ssm, envs[VAR], inp, steps, 1, cost)['obj_cost'])   # obj_mode is not read
    for e, tail in enumerate(tails(inp)):
        ref = perf_taylor_rollout(probs[ABS], gp, inp['x0'][e], inp['safe'][e], tail, 1)
        check_objective(f'taylor ({n_s},{n_u}) N={N} n_perf={steps} e={e}', twin, sat['obj_cost'][e], sat['perf_traj'][e],
                        sat['perf_cov'][e], ref, steps)


def launch_cautious(ssm, env, inp, steps, propagate, cost=None):
    out = cem_mpc.cem_cautious_rollout(ssm, env, T(inp['x0']), steps, propagate=propagate, want_traj=True, want_sigma=True,
                                       want_cov=True, want_margins=True, mean=T(inp['mean']), std=T(inp['std']),
                                       noise=T(inp['noise']), **({} if cost is None else dict(cost=cost)))
    torch.cuda.synchronize()
    assert int(out['status'].item()) == 0
    return out


@pytest.mark.parametrize('propagate', [True, False])
@pytest.mark.parametrize('steps', STEPS)
@pytest.mark.parametrize('n_s,n_u,N', CASES)
def test_cautious_sat_rollout(n_s, n_u, N, steps, propagate):
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    cost, twin = cost_for(n_s)
    inp = rows_inputs(n_s, n_u, SMALL, steps, seed=n_s + 7 * n_u + N + 100 * steps)
    parent = launch_cautious(ssm, envs[ABS], inp, steps, propagate)
    sat = launch_cautious(ssm, envs[ABS], inp, steps, propagate, cost)
    for name in CAUTIOUS_OUTPUTS:
        if name != 'obj_cost':
            assert torch.equal(parent[name], sat[name]), name
    assert torch.equal(sat['obj_cost'], launch_cautious(ssm, envs[VAR], inp, steps, propagate, cost)['obj_cost'])
    if not propagate:
        assert torch.equal(sat['cov'], torch.diag_embed(sat['sigma']))      # the cost prices diag(var_t)
    for e, rows in enumerate(drawn_rows(inp)):
        ref = cautious_rollout(probs[ABS], gp, inp['x0'][e], rows, propagate)
        check_objective(f'cautious ({n_s},{n_u}) N={N} T={steps} propagate={propagate} e={e}', twin, sat['obj_cost'][e],
                        sat['traj'][e], sat['cov'][e], ref, steps)


def launch_multi(ssms, env, inp, n_perf, r, cost=None):
    status = torch.zeros(len(ssms), dtype=torch.int32, device=DEV)
    out = cem_mpc.cem_perf_rollout_taylor_multi(ssms, env, T(inp['x0']), multi.H, n_perf, r, status=status, want_sigma=True,
                                                want_cov=True, **multi._kw(inp, slice(None), None),
                                                **({} if cost is None else dict(cost=cost)))
    torch.cuda.synchronize()
    assert status.tolist() == [0] * len(ssms)
    return out


@pytest.mark.parametrize('steps', STEPS)
@pytest.mark.parametrize('n_s,n_u,sizes', MULTI_CASES)
def test_taylor_sat_multi_rollout(n_s, n_u, sizes, steps):
    ssms, envs, gps, probs = multi.case(n_s, n_u, sizes)
    cost, twin = cost_for(n_s)
    inp = multi.inputs(len(sizes), n_s, n_u, SMALL, steps, 1, seed=n_s + 7 * n_u + sum(sizes) + steps)
    parent, sat = launch_multi(ssms, envs[ABS], inp, steps, 1), launch_multi(ssms, envs[ABS], inp, steps, 1, cost)
    for name in TAYLOR_OUTPUTS:
        if name != 'obj_cost':
            assert torch.equal(parent[name], sat[name]), name
    for e in range(len(sizes)):
        tail = inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e]
        ref = perf_taylor_rollout(probs[ABS], gps[e], inp['x0'][e], inp['safe'][e], tail, 1)
        check_objective(f'multi ({n_s},{n_u}) N={sizes} n_perf={steps} e={e}', twin, sat['obj_cost'][e], sat['perf_traj'][e],
                        sat['perf_cov'][e], ref, steps)


# ---- the grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,N,steps', [(2, 1, 200, 15), (4, 1, 590, 3)])
def test_a_tile_does_not_depend_on_the_grid(n_s, n_u, N, steps):
    """P = 4096 + 53 per problem; the first 37 particles of each problem in a launch of their own are bit-identical."""
    ssm, envs = case(n_s, n_u, N)[:2]
    cost, _ = cost_for(n_s)
    inp = inputs(n_s, n_u, LARGE, steps, 1, seed=n_s + N)
    sub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in inp.items()}
    big, small = launch_taylor(ssm, envs[ABS], inp, steps, 1, cost), launch_taylor(ssm, envs[ABS], sub, steps, 1, cost)
    for name in TAYLOR_OUTPUTS:
        assert torch.equal(small[name], big[name][:, :SMALL]), name
    rows = {k: inp[k] for k in ('x0', 'mean', 'std', 'noise')}
    sub = dict(rows, noise=np.ascontiguousarray(rows['noise'][:, :SMALL]))
    big, small = launch_cautious(ssm, envs[ABS], rows, steps - 1, True, cost), launch_cautious(ssm, envs[ABS], sub, steps - 1,
                                                                                               True, cost)
    for name in CAUTIOUS_OUTPUTS:
        assert torch.equal(small[name], big[name][:, :SMALL]), name
    sizes = (N, 100)
    ssms, menvs = multi.case(n_s, n_u, sizes)[:2]
    minp = multi.inputs(2, n_s, n_u, LARGE, steps, 1, seed=n_s + N)
    msub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in minp.items()}
    big, small = launch_multi(ssms, menvs[ABS], minp, steps, 1, cost), launch_multi(ssms, menvs[ABS], msub, steps, 1, cost)
    for name in TAYLOR_OUTPUTS:
        assert torch.equal(small[name], big[name][:, :SMALL]), name


# ---- the whole solve, with the cart-pole constants -------------------------------------------------------------------------------
def cartpole_cost():
    return SaturatingCost(so.CARTPOLE_TARGET, so.CARTPOLE_WEIGHT, so.CARTPOLE_TRIG_IDX)


def check_solve(history, trace, best, ref_best, k):
    assert len(history) == len(trace)
    for it, (h, (con, obj, idx)) in enumerate(zip(history, trace)):
        print(f'iteration {it}: objective {worst(h.objective_costs, obj, **SIGMA_TOL):.3f} of SIGMA_TOL, '
              f'{int((con > 0).sum())} of {len(con)} rows violate')
        close(h.constraint_costs, con, rtol=0, atol=0)
        close(h.objective_costs, obj, **SIGMA_TOL)
        assert set(ocem.rank(N_(h.constraint_costs), N_(h.objective_costs), k)) == set(idx)
    print(f'best row: max |device - numpy CEM| = {float(np.abs(N_(best) - ref_best).max()):.3e}')
    close(best, ref_best, rtol=0, atol=1e-9)


@pytest.mark.parametrize('kind', ['cautious', 'cautious_me'])
def test_cautious_solve_matches_the_numpy_cem(kind):
    """The inputs are those tests/test_sat_cost_host.py checks on the CPU: every elite set is decided by more than 1e-6."""
    c = SOLVE
    ref_best, trace, noise = oracle_solve(kind)
    spec = solve_case()[0]
    ssm, env = problems.build(spec, device=DEV)
    mpc = cem_mpc.CautiousCemMpc(ssm, env, c['T'], c['P'], c['k'], c['iters'], device=DEV, init_std=c['init_std'],
                                 propagate=kind == 'cautious', record_rollouts=True)
    mpc.set_cost(cartpole_cost())
    best, ok, history, status = mpc.solve(T(SOLVE_X0[None]), noise=T(noise[:, None]))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and bool(ok[0].item())
    check_solve(history, trace, best[0], ref_best, c['k'])


def test_taylor_performance_solve_matches_the_numpy_cem():
    c = SOLVE
    ref_best, trace, noise = oracle_solve('taylor')
    spec = solve_case()[0]
    ssm, env = problems.build(spec, device=DEV)
    mpc = cem_mpc.FusedCemMpc(ssm, env, c['H'], c['P'], c['k'], c['iters'], device=DEV, init_std=c['init_std'],
                              n_perf=c['n_perf'], perf_r=c['r'], perf_type='taylor', record_rollouts=True)
    mpc.set_cost(cartpole_cost())
    best, ok, history, status = mpc.solve(T(SOLVE_X0[None]), noise=T(noise[:, None]))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and bool(ok[0].item())
    check_solve(history, trace, best[0], ref_best, c['k'])


# ---- through the classes -----------------------------------------------------------------------------------------------------
def pendulum_cost():
    """The pendulum's angle is state 1 (problems.pendulum: (velocity, angle)); upright is cos = 1."""
    return SaturatingCost([0.0, 0.0, 1.0], np.diag([0.1, 1.0, 1.0]), trig_idx=1)


def test_cautious_get_action_after_init_solver():
    from safe_exploration_amd.safempc_cem import MpcResult
    spec = problems.pendulum(n_train=200, seed=0, obj_mode=ABS)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=-0.1)
    solver, _ = make_cautious(spec, type('C', (CautiousConf,), dict(cautious_state_polytope='safe'))(), env)
    cost = pendulum_cost()
    solver.init_solver(lambda *a: 0.0)
    assert solver._cost is None
    solver.init_solver(cost)
    x = np.array([0.02, -0.03])
    with mock.patch.object(cem_mpc, 'cem_cautious_rollout', wraps=cem_mpc.cem_cautious_rollout) as spy:
        action, result, means, covs, row, margins = solver.get_action_verbose(x)
    mpc = solver._solver()
    assert result == MpcResult.FOUND_SOLUTION and mpc._cost is cost and mpc.last_status == 0
    assert spy.call_count >= CautiousConf.cem_num_iterations and all(c[1].get('cost') is cost for c in spy.call_args_list)
    assert np.array_equal(row[0], action) and row.shape == (CautiousConf.T, 1)
    # the plan is the sat solve's: the same solver without the cost plans another row
    plain, _ = make_cautious(spec, type('C', (CautiousConf,), dict(cautious_state_polytope='safe'))(), env)
    other = plain.get_action_verbose(x)[4]
    assert not np.array_equal(other, row)
    # ... and its cost, priced by the entry on the plan itself, is the smallest feasible one the last iteration saw
    out = mpc.evaluate(T(x[None]), T(row[None, None]))
    torch.cuda.synchronize()
    assert float(out['con_cost'].item()) == 0.0 and 0.0 < float(out['obj_cost'].item()) < CautiousConf.T


def test_safempc_get_action_after_init_solver():
    from safe_exploration_amd.safempc_cem import MpcResult
    spec = problems.pendulum(n_train=200, seed=0, obj_mode=ABS)
    env = problems.StubEnv(spec, np.zeros(2), objective_target=-0.1)
    solver, _ = problems.make_solver(spec, TaylorConf(), env, device=DEV)
    cost = pendulum_cost()
    solver.init_solver(cost)
    with mock.patch.object(cem_mpc, 'cem_perf_rollout_taylor', wraps=cem_mpc.cem_perf_rollout_taylor) as spy:
        action, result = solver.get_action(np.array([0.02, -0.03]))
    mpc = solver._solver()
    assert result == MpcResult.FOUND_SOLUTION and action.shape == (1,) and mpc._cost is cost and mpc.last_status == 0
    assert spy.call_count >= TaylorConf.cem_num_iterations and all(c[1].get('cost') is cost for c in spy.call_args_list)
    assert np.array_equal(np.asarray(solver._last_mpc_actions).reshape(-1)[:1], np.asarray(action).reshape(-1))
    # a solver without the Taylor form refuses the cost
    plain, _ = problems.make_solver(spec, type('C', (TaylorConf,), dict(cem_perf_type='mean_equivalent',
                                                                       cem_perf_terminal_safety=False))(), env, device=DEV)
    with pytest.raises(ValueError, match="cem_perf_type='taylor'"):
        plain.init_solver(cost)
