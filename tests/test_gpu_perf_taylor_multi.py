"""GPU: Taylor uncertainty propagation for E problems with an exact GP each -- sx_cem_perf_rollout_taylor_multi against the
numpy oracle per problem (tests/perf_taylor_oracle.py with that problem's ExactGP: it assembles the block matrices and does
not share the kernel's short form) and against sx_cem_perf_rollout_taylor model by model (bit for bit where the launch's
form is the model's own), past one pass of the grid, the terminal-safety coupling with one polytope for three models, the
per-problem status word, the MultiModelPerfCemMpc solve with perf_type='taylor' against FusedCemMpc per model, and the
lockstep runner / find_max_variance_multi over one cem_perf_type='taylor' solver per scenario.

The cases are those of tests/test_gpu_perf_multi.py (its case() / inputs(): ONE sx_env with a non-zero k_fb, H = 5, E = 3 GPs
with data and hyper-parameters of their own; SIZES = (7, 200, 590) goes output by output for all three, SIZES_STREAM =
(7, 100, 200) keeps all outputs in LDS).  Tolerances: MEAN_TOL (rtol 1e-10, atol 1e-12) for rows, means and the affine
objective; SIGMA_TOL (rtol 1e-8, atol 1e-11) for perf_sigma = diag G, perf_cov and the variance objective; the con_cost
increment exactly; solve-level comparisons atol 1e-9, as tests/test_gpu_multi_model.py and tests/test_gpu_perf_multi.py ask
of a multi-model solve against per-model solves.  Every case prints its worst error as a fraction of the tolerance before
it asserts.  Measured figures: DESIGN.md section 3.9, "multi-model Taylor form"."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from perf_taylor_oracle import perf_taylor_rollout
from safe_exploration_amd import _lib, problems
from safe_exploration_amd.cem_mpc import (FusedCemMpc, FusedMultiUnsupported, GpModelTable, MultiModelPerfCemMpc,
                                          cem_perf_rollout_taylor, cem_perf_rollout_taylor_multi)
from test_gpu_perf_multi import (ABS, DEV, H, MEAN_TOL, SIGMA_TOL, SIZES, SIZES_STREAM, SX_FORM_BYOUT, SX_FORM_STREAM, VAR,
                                 N_, T, _kw, _pendulums, case, close, given_rows, inputs, worst)

pytestmark = pytest.mark.gpu
SMALL, LARGE = 37, 1381            # 3 tiles per problem; 87 tiles per problem = 261 workgroups, the last tile with 5 live slots
OUTPUTS = ('rows', 'perf_traj', 'perf_sigma', 'perf_cov', 'obj_cost', 'con_cost')


def seed_of(n_s, n_u, sizes):
    return 29 + n_s + 7 * n_u + sum(sizes)


def launch_multi(ssms, env, inp, n_perf, r, rows=None, table=None, terminal_safety=False, expect_status=0):
    E = len(ssms)
    status = torch.zeros(E, dtype=torch.int32, device=DEV)
    out = cem_perf_rollout_taylor_multi(ssms, env, T(inp['x0']), H, n_perf, r, status=status, table=table, want_sigma=True,
                                        want_cov=True, terminal_safety=terminal_safety, **_kw(inp, slice(None), rows))
    torch.cuda.synchronize()
    if expect_status is not None:
        assert status.tolist() == [expect_status] * E
    return out


def launch_single(ssm, env, inp, e, n_perf, r, rows=None, terminal_safety=False):
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = cem_perf_rollout_taylor(ssm, env, T(inp['x0'][e:e + 1]), H, n_perf, r, status=status, want_sigma=True,
                                  want_cov=True, terminal_safety=terminal_safety, **_kw(inp, slice(e, e + 1), rows))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


def forms(ssms, n_perf):
    """(the launch's form, every model's own form), from the form queries."""
    lib = _lib.lib()
    models = (_lib.SxGpModel * len(ssms))(*[s.device_model for s in ssms])
    return (int(lib.sx_cem_perf_rollout_taylor_multi_form(models, len(ssms), n_perf)),
            [int(lib.sx_cem_perf_rollout_taylor_form(s.device_model, n_perf)) for s in ssms])


def expected_form(own):
    assert all(f in (SX_FORM_STREAM, SX_FORM_BYOUT) for f in own), own
    return SX_FORM_BYOUT if SX_FORM_BYOUT in own else SX_FORM_STREAM


def tail_of(inp, e):
    return inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e]


def oracle_objective(prob, ref):
    return sum(ocem.objective_cost(prob, ref.traj[:, t], ref.sigma[:, t]) for t in range(ref.traj.shape[1]))


def against_the_oracle(out, e, ref, want_obj, obj_tol, con0, label):
    """Prints problem e's worst errors as fractions of their tolerances, then asserts them."""
    print(f'{label}: of the tolerance: rows {worst(out["rows"][e], ref.rows, **MEAN_TOL):.3f}, traj '
          f'{worst(out["perf_traj"][e], ref.traj, **MEAN_TOL):.3f}, diag G '
          f'{worst(out["perf_sigma"][e], ref.sigma, **SIGMA_TOL):.3f}, cov '
          f'{worst(out["perf_cov"][e], ref.cov, **SIGMA_TOL):.3f}, obj {worst(out["obj_cost"][e], want_obj, **obj_tol):.3f}; '
          f'largest propagated part of diag G {float((ref.sigma - ref.var).max()):.3e}, smallest variance {ref.var.min():.3e}')
    close(out['rows'][e], ref.rows, **MEAN_TOL)
    close(out['perf_traj'][e], ref.traj, **MEAN_TOL)
    close(out['perf_sigma'][e], ref.sigma, **SIGMA_TOL)
    close(out['perf_cov'][e], ref.cov, **SIGMA_TOL)
    close(out['obj_cost'][e], want_obj, **obj_tol)
    close(out['con_cost'][e] - T(con0[e]), ref.con_cost, rtol=0, atol=0)


def against_the_single_model_launch(out, e, one, same_form, obj_tol, label):
    """Bit for bit where the launch's form is the model's own; within the tolerances where the model runs output by output
    only because another model needs it (another summation order than the model's own launch)."""
    if same_form:
        for n in OUTPUTS:
            assert torch.equal(out[n][e], one[n][0]), f'{label} {n}'
        return
    print(f'{label}: another form than the model\'s own; of the tolerance against its own launch: traj '
          f'{worst(out["perf_traj"][e], one["perf_traj"][0], **MEAN_TOL):.3f}, diag G '
          f'{worst(out["perf_sigma"][e], one["perf_sigma"][0], **SIGMA_TOL):.3f}, cov '
          f'{worst(out["perf_cov"][e], one["perf_cov"][0], **SIGMA_TOL):.3f}, obj '
          f'{worst(out["obj_cost"][e], one["obj_cost"][0], **obj_tol):.3f}')
    close(out['perf_traj'][e], one['perf_traj'][0], **MEAN_TOL)
    close(out['perf_sigma'][e], one['perf_sigma'][0], **SIGMA_TOL)
    close(out['perf_cov'][e], one['perf_cov'][0], **SIGMA_TOL)
    close(out['obj_cost'][e], one['obj_cost'][0], **obj_tol)
    assert torch.equal(out['rows'][e], one['rows'][0]) and torch.equal(out['con_cost'][e], one['con_cost'][0])


_REFS = {}


def oracle_refs(n_s, n_u, sizes, P, n_perf, r):
    """(inputs, the oracle's rollout per problem), computed once per case and left unchanged."""
    key = (n_s, n_u, sizes, P, n_perf, r)
    if key not in _REFS:
        gps, probs = case(n_s, n_u, sizes)[2:]
        inp = inputs(len(sizes), n_s, n_u, P, n_perf, r, seed=seed_of(n_s, n_u, sizes))
        _REFS[key] = (inp, [perf_taylor_rollout(probs[VAR], gps[e], inp['x0'][e], inp['safe'][e], tail_of(inp, e), r)
                            for e in range(len(sizes))])
    return _REFS[key]


# ---- 1: against the oracle and the single-model launch ---------------------------------------------------------------------
def check_kernel(n_s, n_u, sizes, P, n_perf, r, modes=(VAR, ABS), given=True):
    ssms, envs, gps, probs = case(n_s, n_u, sizes)
    E = len(ssms)
    multi_form, own = forms(ssms, n_perf)
    assert multi_form == expected_form(own)
    inp, refs = oracle_refs(n_s, n_u, sizes, P, n_perf, r)
    # on the oracle alone: the action box is violated somewhere, and the propagated part of diag G is there to be checked
    violations = sum(int(ref.violations.sum()) for ref in refs)
    propagated = max(float((ref.sigma - ref.var).max()) for ref in refs)
    print(f'({n_s},{n_u}) N={sizes} P={P} n_perf={n_perf} r={r}: form {multi_form} (own {own}); oracle: {violations} box '
          f'violations, propagated part {propagated:.3e}, smallest variance {min(ref.var.min() for ref in refs):.3e}')
    assert violations > 0, 'no tail action leaves the box'
    assert propagated > 100 * SIGMA_TOL['atol']
    table = GpModelTable()
    outs, identical = {}, 0
    for mode in modes:
        obj_tol = SIGMA_TOL if mode == VAR else MEAN_TOL
        drawn = launch_multi(ssms, envs[mode], inp, n_perf, r, table=table)
        launches = [('drawn', drawn, None)]
        if given:
            rows = given_rows(drawn)
            launches.append(('given', launch_multi(ssms, envs[mode], inp, n_perf, r, rows=rows, table=table), rows))
        for e, ref in enumerate(refs):
            want_obj = oracle_objective(probs[mode], ref)
            for name, out, rows in launches:
                label = f'({n_s},{n_u}) N={sizes[e]} P={P} n_perf={n_perf} r={r} mode={mode} {name}'
                against_the_oracle(out, e, ref, want_obj, obj_tol, inp['con0'], label)
                one = launch_single(ssms[e], envs[mode], inp, e, n_perf, r, rows=rows)
                against_the_single_model_launch(out, e, one, own[e] == multi_form, obj_tol, label)
            identical += own[e] == multi_form
            assert torch.equal(drawn['rows'][e, :, :H], T(inp['safe'][e]))           # the shared actions: bit-identical
        for name, out, _ in launches:
            assert torch.equal(out['perf_cov'], out['perf_cov'].transpose(-1, -2)), name   # symmetric to the bit
            for n in OUTPUTS:
                assert torch.equal(out[n], drawn[n]), (name, n)                      # the two forms see the same tail bits
        outs[mode] = drawn
    assert identical >= len(modes), 'no problem runs in its own form: nothing is compared bit for bit'
    if len(modes) == 2:
        for n in OUTPUTS:
            if n != 'obj_cost':
                assert torch.equal(outs[VAR][n], outs[ABS][n]), n                   # the mode changes the objective only
    return outs, inp


@pytest.mark.parametrize('sizes', [SIZES, SIZES_STREAM])
@pytest.mark.parametrize('n_s,n_u', [(2, 1), (4, 1), (2, 2)])
def test_taylor_multi_matches_the_oracle_and_the_single_model_launch(n_s, n_u, sizes):
    check_kernel(n_s, n_u, sizes, SMALL, 8, 1)


@pytest.mark.parametrize('n_perf,r', [(8, 3), (2, 1)])
@pytest.mark.parametrize('sizes', [SIZES, SIZES_STREAM])
def test_taylor_multi_at_other_horizons(sizes, n_perf, r):
    check_kernel(2, 1, sizes, SMALL, n_perf, r)


# ---- 2: more workgroups than compute units ----------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,sizes,n_perf,r', [(2, 1, SIZES, 8, 3), (4, 1, SIZES_STREAM, 2, 1), (2, 2, SIZES, 2, 1)])
def test_taylor_multi_past_one_pass_of_the_grid(n_s, n_u, sizes, n_perf, r):
    """P = 1381: 87 tiles per problem, 261 workgroups, a last tile with 5 live slots.  The first 37 particles of each problem
    equal, bit for bit, a P = 37 launch over the same first 37 inputs: a tile depends on its 16 particles alone."""
    assert (LARGE + 15) // 16 == 87 and LARGE % 16 == 5
    outs, inp = check_kernel(n_s, n_u, sizes, LARGE, n_perf, r, modes=(VAR,), given=False)
    ssms, envs = case(n_s, n_u, sizes)[:2]
    sub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in inp.items()}
    small = launch_multi(ssms, envs[VAR], sub, n_perf, r)
    for n in OUTPUTS:
        assert torch.equal(small[n], outs[VAR][n][:, :SMALL]), n


# ---- 3: the terminal-safety coupling ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,sizes', [(2, 1, SIZES), (4, 1, SIZES_STREAM), (2, 2, SIZES)])
def test_terminal_safety_with_one_polytope_for_three_models(n_s, n_u, sizes):
    """The polytope's offset comes from the oracle, pooled over the three problems: every particle's largest row distance
    with h_vec = 0, the 111 values sorted, and a common h_vec in the widest gap between neighbours inside the middle half."""
    ssms, envs, gps, probs = case(n_s, n_u, sizes)
    E, n_perf, r = len(ssms), 8, 1
    assert n_perf >= H + 2
    inp = inputs(E, n_s, n_u, SMALL, n_perf, r, seed=seed_of(n_s, n_u, sizes))
    m = probs[VAR].h_mat.shape[0]
    zero = dataclasses.replace(probs[VAR], h_vec=np.zeros((m, 1)))
    d_max = np.concatenate([perf_taylor_rollout(zero, gps[e], inp['x0'][e], inp['safe'][e], tail_of(inp, e), r)
                            .distances.max(axis=1) for e in range(E)])
    assert len(d_max) == E * SMALL
    order = np.sort(d_max)
    lo, hi = len(order) // 4, 3 * len(order) // 4
    i = lo + int(np.argmax(np.diff(order[lo:hi + 1])))
    gap, offset = order[i + 1] - order[i], 0.5 * (order[i] + order[i + 1])
    prob = dataclasses.replace(probs[VAR], h_vec=np.full((m, 1), offset))
    refs = [perf_taylor_rollout(prob, gps[e], inp['x0'][e], inp['safe'][e], tail_of(inp, e), r, terminal_safety=True)
            for e in range(E)]
    unsafe = [int(ref.unsafe.sum()) for ref in refs]
    nearest = min(float(np.abs(ref.distances.max(axis=1)).min()) for ref in refs)
    print(f'({n_s},{n_u}) N={sizes}: offset {offset:.6e}, gap {gap:.3e}, violating per problem {unsafe} of {SMALL}, the '
          f'nearest particle {nearest:.3e} from the polytope\'s boundary')
    assert gap > 1e-6
    assert all(0 < u < SMALL for u in unsafe)                      # every problem has violating and non-violating particles
    assert nearest >= 0.5 * gap * (1 - 1e-9)                       # no decision hangs on the last bits
    env = _lib.SxEnv.from_buffer_copy(envs[VAR])
    for j in range(m):
        env.h_vec[j] = offset
    table = GpModelTable()
    on = launch_multi(ssms, env, inp, n_perf, r, table=table, terminal_safety=True)
    off = launch_multi(ssms, env, inp, n_perf, r, table=table)
    for e, ref in enumerate(refs):
        got = on['con_cost'][e] - T(inp['con0'][e])
        print(f'({n_s},{n_u}) N={sizes[e]}: con_cost increments differing from the oracle: '
              f'{int((N_(got) != ref.con_cost).sum())} of {SMALL}')
        close(got, ref.con_cost, rtol=0, atol=0)
        close(off['con_cost'][e] - T(inp['con0'][e]), ocem.ACTION_VIOLATION_COST * ref.violations, rtol=0, atol=0)
    for n in OUTPUTS[:5]:
        assert torch.equal(on[n], off[n]), n
    # the flag with a trajectory that ends before the checked state: ValueError from the wrapper
    short = inputs(E, n_s, n_u, SMALL, H + 1, r, seed=1)
    with pytest.raises(ValueError, match='n_perf'):
        launch_multi(ssms, env, short, H + 1, r, terminal_safety=True)


# ---- 4: the status word -----------------------------------------------------------------------------------------------------
def test_a_nan_model_sets_only_its_own_status_word():
    """A data NaN in the packed operands of problem 1 (a_pack[0]: the first fragment of output 0's first row-block, which
    every tile of that problem reads)."""
    n_s, n_u, n_perf, r, bad = 2, 1, 6, 1, 1
    ssms, envs = case(n_s, n_u, SIZES)[:2]
    inp = inputs(3, n_s, n_u, SMALL, n_perf, r, seed=17)
    clean = launch_multi(ssms, envs[VAR], inp, n_perf, r)
    poisoned = ssms[bad]._buffers[1].view(-1)
    keep = poisoned[0].clone()
    poisoned[0] = float('nan')
    try:
        out = launch_multi(ssms, envs[VAR], inp, n_perf, r, expect_status=None)
    finally:
        poisoned[0] = keep
    words = [int(w) for w in out['status'].tolist()]
    assert words[bad] & _lib.SX_STATUS_NAN and [w for e, w in enumerate(words) if e != bad] == [0, 0], words
    for e in range(3):
        if e != bad:
            for n in OUTPUTS:
                assert torch.equal(out[n][e], clean[n][e]), (e, n)
    assert bool(torch.isnan(out['obj_cost'][bad]).all())
    again = launch_multi(ssms, envs[VAR], inp, n_perf, r)            # the value is back
    assert torch.equal(again['obj_cost'], clean['obj_cost'])


# ---- 5: a model without a form ----------------------------------------------------------------------------------------------
def test_a_model_without_a_form_makes_the_launch_unsupported():
    ssms, envs = case(2, 1, (7, 1100))[:2]
    multi_form, own = forms(ssms, 2)
    assert multi_form < 0 and own[0] >= 0 and own[1] < 0
    inp = inputs(2, 2, 1, SMALL, 2, 1, seed=1)
    obj = torch.full((2, SMALL), float('nan'), dtype=torch.float64, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(FusedMultiUnsupported, match='taylor'):
        cem_perf_rollout_taylor_multi(ssms, envs[VAR], T(inp['x0']), H, 2, 1, status=status, safe_actions=T(inp['safe']),
                                      obj_cost=obj, con_cost=T(inp['con0']), tail_mean=T(inp['mean']),
                                      tail_std=T(inp['std']), tail_noise=T(inp['noise']))
    torch.cuda.synchronize()
    assert bool(torch.isnan(obj).all()) and status.tolist() == [0, 0]          # refused before any launch: nothing written


# ---- 6: the whole solve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('safety', [False, True])
def test_multi_model_solve_is_the_single_model_solve_per_problem(safety):
    """Injected noise: problem e's best row against FusedCemMpc(perf_type='taylor').solve of model e with the same noise."""
    ssms, env = _pendulums(VAR)
    E, P, k, iters, n_perf, r = len(ssms), 256, 20, 4, 8, 1
    assert H + 2 <= n_perf
    steps = H + n_perf - r
    noise = np.random.default_rng(5).normal(size=(iters, E, P, steps, 1))
    x0 = np.array([[0.02, -0.03], [-0.01, 0.02], [0.03, 0.0]])
    kw = dict(device=DEV, init_std=0.2, n_perf=n_perf, perf_r=r, perf_type='taylor', perf_terminal_safety=safety)
    mpc = MultiModelPerfCemMpc(ssms, env, H, P, k, iters, **kw)
    assert mpc.fused_applies() is True
    best, ok, status = mpc.solve(T(x0), noise=T(noise))
    torch.cuda.synchronize()
    assert tuple(best.shape) == (E, steps, 1) and status.tolist() == [0] * E
    feasible = 0
    for e in range(E):
        one = FusedCemMpc(ssms[e], env, H, P, k, iters, **kw)
        b, o, _, st = one.solve(T(x0[e:e + 1]), noise=T(noise[:, e:e + 1]))
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and bool(o[0].item()) == bool(ok[e].item()), e
        if bool(o[0].item()):
            feasible += 1
            print(f'terminal safety {safety}, problem {e}: max |multi - single| = {float((best[e] - b[0]).abs().max()):.3e} '
                  f'({float((best[e] - b[0]).abs().max()) / 1e-9:.3f} of the tolerance)')
            close(best[e], b[0], rtol=0, atol=1e-9)
    print(f'terminal safety {safety}: {feasible} of {E} problems feasible')
    if not safety:
        assert feasible > 0, 'the test problems should be feasible'


# ---- 7: the lockstep runner and the exploration helper ----------------------------------------------------------------------
class Conf:
    mpc_time_horizon, cem_num_rollouts, cem_num_elites, cem_num_iterations, cem_init_std = 5, 256, 24, 4, 0.2
    cem_n_perf, cem_perf_type = 5, 'taylor'
    device, use_state_constraint, use_prior_model = DEV, True, True
    exact_gp_training_iterations, exact_gp_kernel = 0, 'rbf'
    plot_cem_optimisation = plot_cem_terminal_states = False


def _scenarios():
    specs = [problems.pendulum(n_train=N, seed=s) for N, s in ((60, 3), (120, 4), (200, 5))]
    x0s = problems.start_states(2, len(specs), seed=5, std=0.03)

    def scenario(e):
        env = problems.StubEnv(specs[e], x0s[e])                  # no objective: the solvers explore
        return problems.make_solver(specs[e], Conf(), env)[0], env
    return specs, x0s, scenario


def test_lockstep_runner_with_one_taylor_solver_per_scenario_matches_do_rollout():
    from safe_exploration_amd.episode_runner import do_rollout, do_rollout_batch
    from safe_exploration_amd.safempc_cem import MpcResult
    specs, _, scenario = _scenarios()
    steps = 6
    seq = []
    for e in range(len(specs)):
        solver, env = scenario(e)
        seq.append(do_rollout(env, steps, solver=solver))
    pairs = [scenario(e) for e in range(len(specs))]
    solvers, envs = [p[0] for p in pairs], [p[1] for p in pairs]
    res = do_rollout_batch(envs, steps, solvers)
    multi = solvers[0]._multi[1]
    assert isinstance(multi, MultiModelPerfCemMpc) and multi._perf.kind == 'taylor' and multi.per_model_solves == 0
    for s in solvers:
        assert s._solver()._perf.type == 'taylor'
        assert tuple(s._solver().last_perf_actions.shape) == (1, Conf.cem_n_perf - 1, 1)
    for e, (r, (xx, yy, cc, codes, failed)) in enumerate(zip(res, seq)):
        assert r.safety_failure == failed and r.xx.shape == xx.shape, e
        print(f'scenario {e}: max |lockstep - one by one| = {float(np.abs(r.xx - xx).max()):.3e} (states), '
              f'{float(np.abs(r.yy - yy).max()):.3e} (targets); tolerance 1e-9')
        np.testing.assert_allclose(r.xx, xx, rtol=0, atol=1e-9, err_msg=f'scenario {e}')
        np.testing.assert_allclose(r.yy, yy, rtol=0, atol=1e-9, err_msg=f'scenario {e}')
        np.testing.assert_array_equal(r.exit_codes, codes)
        assert MpcResult.FOUND_SOLUTION in r.mpc_results


def test_find_max_variance_multi_gives_what_the_explorations_give_one_by_one():
    from safe_exploration_amd.safempc_exploration import DynamicSafeMPCExploration, find_max_variance_multi
    specs, x0s, scenario = _scenarios()
    one_by_one = []
    for e in range(len(specs)):
        solver, env = scenario(e)
        one_by_one.append(DynamicSafeMPCExploration(solver, env).find_max_variance(x0s[e])[1][:, 0])
    explorations = [DynamicSafeMPCExploration(*scenario(e)) for e in range(len(specs))]
    x, u, results = find_max_variance_multi(explorations, x0s)
    assert np.array_equal(x, x0s) and u.shape == (len(specs), 1) and len(results) == len(specs)
    print(f'max |multi - one by one| = {float(np.abs(u - np.stack(one_by_one)).max()):.3e}; tolerance 1e-9')
    np.testing.assert_allclose(u, np.stack(one_by_one), rtol=0, atol=1e-9)
    multi = explorations[0].safempc._multi[1]
    assert isinstance(multi, MultiModelPerfCemMpc) and multi._perf.kind == 'taylor' and multi.per_model_solves == 0
