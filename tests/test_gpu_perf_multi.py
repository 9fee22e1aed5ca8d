"""GPU: the performance trajectory for E problems with an exact GP each -- sx_cem_perf_rollout_multi and
sx_cem_perf_rollout_var_multi against the single-model entries model by model (bit for bit where the kernel form is the
model's own) and against the numpy oracles (tests/perf_traj_oracle.py, tests/perf_var_oracle.py), the per-problem status
word, the MultiModelPerfCemMpc solve against FusedCemMpc(n_perf=...) per model, and the lockstep runner / find_max_variance
over one cem_n_perf solver per scenario.

The kernel cases: shapes (2, 1), (4, 1), (2, 2); E = 3 models of N = 7, 200 and 590 over one sx_env, with length-scales
and output-scales of their own -- no two problems share n_pad, the launch's LDS is the largest model's, and 590 forces the
variance kernel output by output for all three; (7, 100, 200) keeps it with all outputs in LDS.  P = 37 and P = 4096 + 53
(more than one problem-aligned pass of tiles, and a last tile with empty slots).  Tolerances: those of
tests/test_gpu_perf_traj.py (rtol 1e-10, atol 1e-12: rows, means, the affine objective) and tests/test_gpu_perf_var.py
(rtol 1e-8, atol 1e-11: perf_sigma and the variance objective).  Every case prints its measured errors before it asserts."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.gp import ExactGP
from perf_traj_oracle import perf_rollout
from perf_var_oracle import perf_var_rollout
from safe_exploration_amd import _lib, problems
from safe_exploration_amd.cem_mpc import (FusedCemMpc, GpModelTable, MultiModelPerfCemMpc, PerfModelTable, cem_perf_rollout,
                                          cem_perf_rollout_multi, cem_perf_rollout_var)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 5
SMALL, LARGE = 37, 4096 + 53
SHAPES = [(2, 1), (4, 1), (2, 2)]
SIZES = (7, 200, 590)             # the variance launch goes output by output: 590 needs it
SIZES_STREAM = (7, 100, 200)      # ... and with all outputs in LDS
VAR, ABS = _lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
MEAN_TOL = dict(rtol=1e-10, atol=1e-12)
SIGMA_TOL = dict(rtol=1e-8, atol=1e-11)
NAMES = ('rows', 'perf_traj', 'obj_cost', 'con_cost')


def T(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def N_(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def close(a, b, rtol, atol):
    np.testing.assert_allclose(N_(a), N_(b), rtol=rtol, atol=atol)


def worst(a, b, rtol, atol):
    """max of |a - b| / (atol + rtol |b|): <= 1 passes assert_allclose."""
    a, b = N_(a), N_(b)
    return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())


_CASES = {}


def case(n_s, n_u, sizes):
    """(E GpCemSSMs on the GPU, {mode: sx_env}, E ExactGPs, {mode: oracle Problem}): ONE environment -- the stable random
    prior, box |u| <= 1 and separable objective of tests/test_gpu_perf_traj.py -- and a GP per problem with its own training
    set, ARD length-scales, output-scales and noise."""
    key = (n_s, n_u, sizes)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(2000 + 100 * n_s + 10 * n_u)
    a = 0.85 * np.eye(n_s) + 0.05 * rng.normal(size=(n_s, n_s))
    b = 0.3 * rng.normal(size=(n_s, n_u))
    base = problems.ProblemSpec('perf_multi', n_s, n_u, None, None, None, None, None, a, b,
                                rng.uniform(-0.3, 0.0, size=(n_u, n_s)), np.full(n_s, 0.02), np.full(n_s, 0.02), 2.0,
                                np.vstack((np.eye(n_s), -np.eye(n_s))), np.full((2 * n_s, 1), 2.0), np.full(n_u, -1.0),
                                np.full(n_u, 1.0), obj_mode=ABS)
    base.obj_w_abs, base.obj_target = rng.uniform(0.2, 1.0, size=n_s), rng.normal(0, 0.1, size=n_s)
    base.obj_w_lin = rng.normal(0, 0.2, size=n_s)
    ssms, gps, env = [], [], None
    for N in sizes:
        X, Y = problems.synthetic_training_set(N, n_s, n_u, seed=N + n_s, scale=0.6, amp=0.05, noise_std=0.002)
        spec = dataclasses.replace(base, X=X, Y=Y, lengthscale=rng.uniform(0.6, 1.4, size=(n_s, n_s + n_u)),
                                   outputscale=rng.uniform(1e-3, 3e-3, size=n_s), noise=rng.uniform(1e-5, 5e-5, size=n_s))
        ssm, env_e = problems.build(spec, device=DEV)
        env = env if env is not None else env_e
        assert bytes(env) == bytes(env_e)                  # the constants do not depend on the model
        ssms.append(ssm)
        gps.append(ExactGP(X, Y, spec.lengthscale, spec.outputscale, spec.noise))
    env_var = _lib.SxEnv.from_buffer_copy(env)
    env_var.obj_mode = VAR
    prob = problems.oracle_problem(base, ocem)
    probs = {ABS: prob, VAR: dataclasses.replace(prob, obj_mode=ocem.OBJ_NEG_VARIANCE)}
    _CASES[key] = out = (ssms, {ABS: env, VAR: env_var}, gps, probs)
    return out


def inputs(E, n_s, n_u, P, n_perf, r, seed):
    rng = np.random.default_rng(seed)
    Tl = n_perf - r
    return dict(x0=rng.normal(0, 0.05, size=(E, n_s)), safe=rng.normal(0, 0.5, size=(E, P, H, n_u)),
                mean=rng.normal(0, 0.2, size=(E, Tl, n_u)), std=rng.uniform(0.3, 0.8, size=(E, Tl, n_u)),
                noise=rng.normal(size=(E, P, Tl, n_u)), con0=3.0 * rng.integers(0, 5, size=(E, P)).astype(np.float64))


def _kw(inp, sel, rows):
    """The buffers of a launch over the problems `sel`: obj_cost starts as NaN (overwritten), con_cost as con0 (added to)."""
    E, P = inp['safe'][sel].shape[:2]
    kw = dict(safe_actions=T(inp['safe'][sel]), obj_cost=torch.full((E, P), float('nan'), dtype=torch.float64, device=DEV),
              con_cost=T(inp['con0'][sel]), want_traj=True)
    if rows is None:
        kw.update(tail_mean=T(inp['mean'][sel]), tail_std=T(inp['std'][sel]), tail_noise=T(inp['noise'][sel]))
    else:
        kw.update(rows=rows[sel].clone())
    return kw


def launch_multi(ssms, env, inp, n_perf, r, variance, rows=None, table=None, expect_status=0):
    E = len(ssms)
    status = torch.zeros(E, dtype=torch.int32, device=DEV)
    out = cem_perf_rollout_multi(ssms, env, T(inp['x0']), H, n_perf, r, variance=variance, status=status, table=table,
                                 **_kw(inp, slice(None), rows), **(dict(want_sigma=True) if variance else {}))
    torch.cuda.synchronize()
    if expect_status is not None:
        assert status.tolist() == [expect_status] * E
    return out


def launch_single(ssm, env, inp, e, n_perf, r, variance, rows=None):
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    fn, extra = (cem_perf_rollout_var, dict(want_sigma=True)) if variance else (cem_perf_rollout, {})
    out = fn(ssm, env, T(inp['x0'][e:e + 1]), H, n_perf, r, status=status, **_kw(inp, slice(e, e + 1), rows), **extra)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


def given_rows(drawn):
    rows = drawn['rows'].clone()
    rows[:, :, :H] = float('nan')             # the safety part of the rows is an output in both forms
    return rows


# ---- the mean-only form ------------------------------------------------------------------------------------------------------
def check_mean_only(n_s, n_u, P, n_perf, r):
    ssms, envs, gps, probs = case(n_s, n_u, SIZES)
    E = len(ssms)
    inp = inputs(E, n_s, n_u, P, n_perf, r, seed=n_s + 7 * n_u + P + 100 * n_perf + r)
    table = PerfModelTable()
    drawn = launch_multi(ssms, envs[ABS], inp, n_perf, r, False, table=table)
    given = launch_multi(ssms, envs[ABS], inp, n_perf, r, False, rows=given_rows(drawn), table=table)
    violations = 0
    for e in range(E):
        tail = inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e]
        ref = perf_rollout(probs[ABS], gps[e], inp['x0'][e], inp['safe'][e], tail, r)
        violations += int(ref.violations.sum())
        for name, out, rows in (('drawn', drawn, None), ('given', given, given_rows(drawn))):
            one = launch_single(ssms[e], envs[ABS], inp, e, n_perf, r, False, rows=rows)
            print(f'({n_s},{n_u}) N={SIZES[e]} P={P} n_perf={n_perf} r={r} {name}: max |traj - oracle| = '
                  f'{float(np.abs(N_(out["perf_traj"][e]) - ref.traj).max()):.3e}, max |obj - oracle| = '
                  f'{float(np.abs(N_(out["obj_cost"][e]) - ref.obj_cost).max()):.3e}, bits differing from the single-model '
                  f'launch: {[int((out[n][e] != one[n][0]).sum()) for n in NAMES]}')
            for n in NAMES:        # the lanes per particle and the model's n_pad are the single-model kernel's
                assert torch.equal(out[n][e], one[n][0]), f'problem {e} {name} {n}'
            close(out['rows'][e], ref.rows, **MEAN_TOL)
            close(out['perf_traj'][e], ref.traj, **MEAN_TOL)
            close(out['obj_cost'][e], ref.obj_cost, **MEAN_TOL)
            close(out['con_cost'][e] - T(inp['con0'][e]), ref.con_cost, rtol=0, atol=0)
        assert torch.equal(drawn['rows'][e, :, :H], T(inp['safe'][e]))
    assert violations > 0, 'no tail action leaves the box: the constraint increment is not tested'
    assert torch.equal(drawn['perf_traj'], given['perf_traj']) and torch.equal(drawn['obj_cost'], given['obj_cost'])


@pytest.mark.parametrize('n_perf,r', [(15, 1), (6, 3)])
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_mean_only_multi_is_the_single_model_launch_per_problem(n_s, n_u, n_perf, r):
    check_mean_only(n_s, n_u, SMALL, n_perf, r)


@pytest.mark.parametrize('n_s,n_u,n_perf,r', [(2, 1, 15, 3), (4, 1, 2, 1), (2, 2, 2, 1)])
def test_mean_only_multi_past_one_pass_of_tiles(n_s, n_u, n_perf, r):
    check_mean_only(n_s, n_u, LARGE, n_perf, r)


# ---- the variance form -------------------------------------------------------------------------------------------------------
def forms(ssms, n_perf):
    lib = _lib.lib()
    models = (_lib.SxGpModel * len(ssms))(*[s.device_model for s in ssms])
    return (int(lib.sx_cem_perf_rollout_var_multi_form(models, len(ssms), n_perf)),
            [int(lib.sx_cem_perf_rollout_var_form(s.device_model, n_perf)) for s in ssms])


def oracle_objective(prob, ref):
    return sum(ocem.objective_cost(prob, ref.traj[:, t], ref.sigma[:, t]) for t in range(ref.traj.shape[1]))


def check_variance(n_s, n_u, sizes, P, n_perf, r, modes=(VAR, ABS)):
    ssms, envs, gps, probs = case(n_s, n_u, sizes)
    E = len(ssms)
    multi_form, own = forms(ssms, n_perf)
    assert multi_form == (SX_FORM_BYOUT if 590 in sizes else SX_FORM_STREAM) and all(f >= 0 for f in own)
    inp = inputs(E, n_s, n_u, P, n_perf, r, seed=3 + n_s + 7 * n_u + P + 100 * n_perf + r + sum(sizes))
    refs = []
    for e in range(E):
        tail = inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e]
        refs.append(perf_var_rollout(probs[VAR], gps[e], inp['x0'][e], inp['safe'][e], tail, r))
    assert sum(int(ref.violations.sum()) for ref in refs) > 0, 'no tail action leaves the box'
    table = GpModelTable()
    identical = 0
    for mode in modes:
        drawn = launch_multi(ssms, envs[mode], inp, n_perf, r, True, table=table)
        given = launch_multi(ssms, envs[mode], inp, n_perf, r, True, rows=given_rows(drawn), table=table)
        obj_tol = SIGMA_TOL if mode == VAR else MEAN_TOL
        for e, ref in enumerate(refs):
            want_obj = oracle_objective(probs[mode], ref)
            one = launch_single(ssms[e], envs[mode], inp, e, n_perf, r, True)
            for name, out in (('drawn', drawn), ('given', given)):
                print(f'({n_s},{n_u}) N={sizes[e]} P={P} n_perf={n_perf} r={r} mode={mode} {name}: form {multi_form} (own '
                      f'{own[e]}), max |traj - oracle| = {float(np.abs(N_(out["perf_traj"][e]) - ref.traj).max()):.3e}, '
                      f'|sigma - oracle| at {worst(out["perf_sigma"][e], ref.sigma, **SIGMA_TOL):.3f} and |obj - oracle| at '
                      f'{worst(out["obj_cost"][e], want_obj, **obj_tol):.3f} of the tolerance')
                close(out['rows'][e], ref.rows, **MEAN_TOL)
                close(out['perf_traj'][e], ref.traj, **MEAN_TOL)
                close(out['perf_sigma'][e], ref.sigma, **SIGMA_TOL)
                close(out['obj_cost'][e], want_obj, **obj_tol)
                close(out['con_cost'][e] - T(inp['con0'][e]), ref.con_cost, rtol=0, atol=0)
            if own[e] == multi_form:
                identical += 1
                for n in NAMES + ('perf_sigma',):
                    assert torch.equal(drawn[n][e], one[n][0]), f'problem {e} {n}'
            else:
                # output by output only because another model needs it: another summation order than the model's own launch
                close(drawn['perf_traj'][e], one['perf_traj'][0], **MEAN_TOL)
                close(drawn['perf_sigma'][e], one['perf_sigma'][0], **SIGMA_TOL)
                close(drawn['obj_cost'][e], one['obj_cost'][0], **obj_tol)
                assert torch.equal(drawn['rows'][e], one['rows'][0]) and torch.equal(drawn['con_cost'][e], one['con_cost'][0])
        for n in NAMES + ('perf_sigma',):
            assert torch.equal(drawn[n], given[n]), n
    assert identical > 0


@pytest.mark.parametrize('sizes', [SIZES, SIZES_STREAM])
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_variance_multi_matches_the_oracle_and_the_single_model_launch(n_s, n_u, sizes):
    check_variance(n_s, n_u, sizes, SMALL, 15, 1)


@pytest.mark.parametrize('n_s,n_u,sizes,n_perf,r', [(2, 1, SIZES, 2, 1), (4, 1, SIZES_STREAM, 6, 3), (2, 2, SIZES, 2, 1)])
def test_variance_multi_past_one_pass_of_tiles(n_s, n_u, sizes, n_perf, r):
    check_variance(n_s, n_u, sizes, LARGE, n_perf, r, modes=(VAR,))


def test_a_model_without_a_form_makes_the_launch_unsupported():
    from safe_exploration_amd.cem_mpc import FusedMultiUnsupported
    ssms, envs = case(2, 1, (7, 1100))[:2]
    assert forms(ssms, 2)[0] < 0
    inp = inputs(2, 2, 1, SMALL, 2, 1, seed=1)
    with pytest.raises(FusedMultiUnsupported):
        launch_multi(ssms, envs[VAR], inp, 2, 1, True)
    launch_multi(ssms, envs[ABS], inp, 2, 1, False)          # the mean-only form stages 1100 points without trouble


# ---- the status word ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variance', [False, True])
def test_a_nan_model_sets_only_its_own_status_word(variance):
    """A data NaN in what the form reads of the model: alpha for the mean-only form; the packed operands for the variance
    form (a_pack: W and the mean rows sx_gp_pack folded alpha into -- that kernel does not read alpha, and its table
    exponential drops a NaN training input)."""
    n_s, n_u, n_perf, r, bad = 2, 1, 6, 1, 1
    ssms, envs = case(n_s, n_u, SIZES)[:2]
    env = envs[VAR if variance else ABS]
    inp = inputs(3, n_s, n_u, SMALL, n_perf, r, seed=17)
    clean = launch_multi(ssms, env, inp, n_perf, r, variance)
    poisoned = (ssms[bad]._buffers[1] if variance else ssms[bad]._alpha).view(-1)
    keep = poisoned[0].clone()       # (a_pack[0]: the first fragment of output 0's first row-block, which every tile reads)
    poisoned[0] = float('nan')
    try:
        out = launch_multi(ssms, env, inp, n_perf, r, variance, expect_status=None)
    finally:
        poisoned[0] = keep
    words = [int(w) for w in out['status'].tolist()]
    assert words[bad] & _lib.SX_STATUS_NAN and [w for e, w in enumerate(words) if e != bad] == [0, 0], words
    for e in range(3):
        if e != bad:
            for n in NAMES + (('perf_sigma',) if variance else ()):
                assert torch.equal(out[n][e], clean[n][e]), (e, n)
    assert bool(torch.isnan(out['obj_cost'][bad]).any())


# ---- the whole solve ---------------------------------------------------------------------------------------------------------
def _pendulums(obj_mode):
    rows = [(60, 1, 1.0, 1.0), (200, 2, 0.8, 1.5), (250, 6, 1.3, 1.0)]
    specs = []
    for N, seed, ls, os_ in rows:
        spec = problems.pendulum(n_train=N, seed=seed, obj_mode=obj_mode)
        spec.lengthscale, spec.outputscale = spec.lengthscale * ls, spec.outputscale * os_
        specs.append(spec)
    built = [problems.build(s, DEV) for s in specs]
    return [b[0] for b in built], built[0][1]


@pytest.mark.parametrize('variance', [False, True])
def test_multi_model_solve_is_the_single_model_solve_per_problem(variance):
    """Injected noise: problem e's best row against FusedCemMpc(n_perf=...).solve of model e with the same noise (atol 1e-9,
    what tests/test_gpu_multi_model.py asks of the comparison without the trajectory: the safety rollouts may take other
    kernel forms)."""
    ssms, env = _pendulums(VAR if variance else ABS)
    E, P, k, iters, n_perf, r = len(ssms), 256, 20, 4, 8, 1
    steps = H + n_perf - r
    noise = np.random.default_rng(5).normal(size=(iters, E, P, steps, 1))
    x0 = np.array([[0.02, -0.03], [-0.01, 0.02], [0.03, 0.0]])
    kw = dict(device=DEV, init_std=0.2, n_perf=n_perf, perf_r=r, perf_variance=variance)
    mpc = MultiModelPerfCemMpc(ssms, env, H, P, k, iters, **kw)
    assert mpc.fused_applies()
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
            print(f'problem {e}: max |multi - single| = {float((best[e] - b[0]).abs().max()):.3e}')
            close(best[e], b[0], rtol=0, atol=1e-9)
    assert feasible > 0, 'the test problems should be feasible'


# ---- the lockstep runner and the exploration helper ------------------------------------------------------------------------
class Conf:
    mpc_time_horizon, cem_num_rollouts, cem_num_elites, cem_num_iterations, cem_init_std = 5, 256, 24, 4, 0.2
    cem_n_perf, cem_perf_variance = 5, True
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


def test_lockstep_runner_with_one_perf_solver_per_scenario_matches_do_rollout():
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
    assert isinstance(multi, MultiModelPerfCemMpc) and multi.per_model_solves == 0
    for s in solvers:
        assert tuple(s._solver().last_perf_actions.shape) == (1, Conf.cem_n_perf - 1, 1)
    for e, (r, (xx, yy, cc, codes, failed)) in enumerate(zip(res, seq)):
        assert r.safety_failure == failed and r.xx.shape == xx.shape, e
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
    np.testing.assert_allclose(u, np.stack(one_by_one), rtol=0, atol=1e-9)
    assert explorations[0].safempc._multi[1].per_model_solves == 0
