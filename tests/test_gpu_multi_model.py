"""GPU: E problems with an exact GP each in one rollout launch (sx_cem_rollout_multi / sx_cem_rollout_elites_multi), the
multi-model solve (MultiModelCemMpc) and the lockstep runner over one solver per scenario.  Reference: the single-model
entry points model by model, and the oracle."""
import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.gp import ExactGP
from safe_exploration_amd import _lib, problems
from safe_exploration_amd.cem_mpc import MultiModelCemMpc, cem_rollout, cem_rollout_multi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _spec(kind, N, seed, ls_scale=1.0, os_scale=1.0, obj_mode=0):
    spec = (problems.pendulum(n_train=N, seed=seed, obj_mode=obj_mode) if kind == 'pendulum'
            else problems.cartpole(n_train=N, seed=seed))
    spec.lengthscale = spec.lengthscale * ls_scale
    spec.outputscale = spec.outputscale * os_scale
    return spec


# (kind, [(N, seed, lengthscale factor, outputscale factor)]): different training sets, sizes and hyper-parameters; the
# 600-point pendulum and the 260-point cart-pole need the output-by-output kernel, which the whole launch then takes
CASES = {
    'pendulum': ('pendulum', [(60, 1, 1.0, 1.0), (200, 2, 0.8, 1.5), (600, 3, 1.2, 0.7), (150, 4, 0.9, 1.0),
                              (90, 5, 1.1, 2.0)]),
    'pendulum_stream': ('pendulum', [(60, 1, 1.0, 1.0), (200, 2, 0.8, 1.5), (250, 6, 1.3, 1.0)]),
    'cartpole': ('cartpole', [(80, 1, 1.0, 1.0), (260, 2, 0.9, 1.3), (128, 3, 1.1, 0.8)]),
}


def _problems(case, obj_mode=0):
    kind, rows = CASES[case]
    specs = [_spec(kind, N, seed, ls, os_, obj_mode=obj_mode) for N, seed, ls, os_ in rows]
    built = [problems.build(s, DEV) for s in specs]
    env = built[0][1]          # one sx_env for all problems (the constants do not depend on the training set)
    return specs, [b[0] for b in built], env


def _multi_form(ssms, H):
    models = (_lib.SxGpModel * len(ssms))(*[s.device_model for s in ssms])
    return _lib.lib().sx_cem_rollout_multi_form(models, len(ssms), H)


def _close(a, b, what):
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-10, atol=1e-14, err_msg=what)


def _close_traj(a, b, what):
    """rtol 1e-10 per entry, with an absolute floor of 1e-9 of the largest entry of the same flat state [p | Q]: the
    single-model reference runs another form of the kernel (RH / RW: other summation orders), and an off-diagonal of Q
    that cancels to a small fraction of the state's scale carries that rounding as a relative error of its own (seen:
    one entry of 1920 at 5.7e-4 agreeing to 8 digits)."""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    floor = 1e-9 * np.abs(b).max(axis=-1, keepdims=True) + 1e-14
    bad = np.abs(a - b) > 1e-10 * np.abs(b) + floor
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} entries differ, e.g. {a[bad][:4]} against {b[bad][:4]}'


@pytest.mark.parametrize('case', sorted(CASES))
def test_given_actions_match_single_model_rollouts(case):
    specs, ssms, env = _problems(case)
    E, n_s, n_u = len(ssms), specs[0].n_s, specs[0].n_u
    P, H = 100, 6
    assert _multi_form(ssms, H) == (3 if case != 'pendulum_stream' else 0)   # SX_FORM_BYOUT / SX_FORM_STREAM
    rng = np.random.default_rng(11)
    x0 = rng.normal(0, 0.03, size=(E, n_s))
    actions = rng.normal(0, 0.3, size=(E, P, H, n_u))
    r = cem_rollout_multi(ssms, env, T(x0), H, actions=T(actions), want_traj=True, want_sigma=True)
    assert r['status'].shape == (E,)
    for e in range(E):
        one = cem_rollout(ssms[e], env, T(x0[e:e + 1]), H, actions=T(actions[e:e + 1]), want_traj=True, want_sigma=True)
        for key in ('obj_cost', 'con_cost', 'sigma'):
            _close(r[key][e], one[key][0], f'{case}: problem {e} {key}')
        _close_traj(r['traj'][e], one['traj'][0], f'{case}: problem {e} traj')
        assert int(r['status'][e]) == int(one['status'][0])


@pytest.mark.parametrize('case', ['pendulum', 'cartpole'])
def test_elite_refit_prologue_matches_single_model_rollouts(case):
    specs, ssms, env = _problems(case)
    E, n_s, n_u = len(ssms), specs[0].n_s, specs[0].n_u
    P, H, k = 64, 5, 7
    rng = np.random.default_rng(12)
    x0 = rng.normal(0, 0.03, size=(E, n_s))
    rows = rng.normal(0, 0.2, size=(E, k, 2 + H * n_u))
    noise = rng.normal(size=(E, P, H, n_u))
    r = cem_rollout_multi(ssms, env, T(x0), H, elite_rows=T(rows), noise=T(noise), want_traj=True, want_sigma=True,
                          want_dist=True)
    for e in range(E):
        one = cem_rollout(ssms[e], env, T(x0[e:e + 1]), H, elite_rows=T(rows[e:e + 1]), noise=T(noise[e:e + 1]),
                          want_traj=True, want_sigma=True, want_dist=True)
        for key in ('actions', 'obj_cost', 'con_cost', 'sigma', 'mean', 'std'):
            _close(r[key][e], one[key][0], f'{case}: problem {e} {key}')
        _close_traj(r['traj'][e], one['traj'][0], f'{case}: problem {e} traj')


def test_multi_model_solve_matches_the_oracle_per_problem():
    """The whole CEM loop over three pendulum problems with their own GPs and injected noise, against oracle.cem.cem_solve
    problem by problem (as test_full_solve_vs_oracle does for one)."""
    specs, ssms, env = _problems('pendulum_stream', obj_mode=1)
    E, H, P, k, iters = len(ssms), 6, 256, 20, 4
    rng = np.random.default_rng(5)
    noise = rng.normal(size=(iters, E, P, H, 1))
    x0 = np.array([[0.02, -0.03], [-0.01, 0.02], [0.03, 0.0]])
    mpc = MultiModelCemMpc(ssms, env, H, P, k, iters, device=DEV, init_std=0.2)
    best, ok, status = mpc.solve(T(x0), noise=T(noise))
    assert status.shape == (E,) and [int(s) for s in status.tolist()] == [0] * E
    feasible = 0
    for e, spec in enumerate(specs):
        gp = ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)
        ref_best, _ = ocem.cem_solve(problems.oracle_problem(spec, ocem), gp, x0[e], noise[:, e], k,
                                     init_std=np.full((H, 1), 0.2))
        assert (ref_best is not None) == bool(ok[e]), e
        if ref_best is not None:
            feasible += 1
            np.testing.assert_allclose(best[e].cpu().numpy(), ref_best, rtol=0, atol=1e-9, err_msg=f'problem {e}')
    assert feasible > 0, 'the test problems should be feasible'


def test_a_nan_model_sets_only_its_own_status_word():
    specs, ssms, env = _problems('pendulum')
    E, P, H = len(ssms), 48, 4
    bad = 2
    ssms[bad]._buffers[0][0, 0] = float('nan')    # a NaN training input: every prediction of that GP is NaN
    rng = np.random.default_rng(13)
    x0 = rng.normal(0, 0.03, size=(E, 2))
    actions = rng.normal(0, 0.3, size=(E, P, H, 1))
    r = cem_rollout_multi(ssms, env, T(x0), H, actions=T(actions))
    words = [int(w) for w in r['status'].tolist()]
    assert words[bad] & _lib.SX_STATUS_NAN
    for e in range(E):
        if e != bad:
            one = cem_rollout(ssms[e], env, T(x0[e:e + 1]), H, actions=T(actions[e:e + 1]))
            assert not words[e] & _lib.SX_STATUS_NAN and words[e] == int(one['status'][0]), (e, words)
            _close(r['obj_cost'][e], one['obj_cost'][0], f'problem {e} obj_cost')


def test_lockstep_runner_with_one_solver_per_scenario_matches_do_rollout():
    """Three scenarios with their own training sets: do_rollout_batch over a list of solvers (one multi-model solve per
    step) against do_rollout scenario by scenario (one solve per step and scenario)."""
    from safe_exploration_amd.episode_runner import do_rollout, do_rollout_batch
    from safe_exploration_amd.safempc_cem import MpcResult

    class Conf:
        mpc_time_horizon, cem_num_rollouts, cem_num_elites, cem_num_iterations, cem_init_std = 5, 256, 24, 4, 0.2
        device, use_state_constraint, use_prior_model = DEV, True, True
        exact_gp_training_iterations, exact_gp_kernel = 0, 'rbf'
        plot_cem_optimisation = plot_cem_terminal_states = False

    specs = [problems.pendulum(n_train=N, seed=s) for N, s in ((60, 3), (120, 4), (200, 5))]
    x0s = problems.start_states(2, len(specs), seed=5, std=0.03)
    steps = 6

    def scenario(e):
        env = problems.StubEnv(specs[e], x0s[e])
        return problems.make_solver(specs[e], Conf(), env)[0], env

    seq = []
    for e in range(len(specs)):
        solver, env = scenario(e)
        seq.append(do_rollout(env, steps, solver=solver))
    pairs = [scenario(e) for e in range(len(specs))]
    solvers, envs = [p[0] for p in pairs], [p[1] for p in pairs]
    res = do_rollout_batch(envs, steps, solvers)
    assert all(s._multi is not None for s in solvers[:1]) and solvers[0]._multi[1].per_model_solves == 0
    for e, (r, (xx, yy, cc, codes, failed)) in enumerate(zip(res, seq)):
        assert r.safety_failure == failed and r.xx.shape == xx.shape, e
        np.testing.assert_allclose(r.xx, xx, rtol=0, atol=1e-9, err_msg=f'scenario {e}')
        np.testing.assert_allclose(r.yy, yy, rtol=0, atol=1e-9, err_msg=f'scenario {e}')
        np.testing.assert_array_equal(r.exit_codes, codes)
        assert MpcResult.FOUND_SOLUTION in r.mpc_results


def test_get_actions_multi_refuses_disagreeing_solvers():
    from safe_exploration_amd.safempc_cem import get_actions_multi

    class Conf:
        mpc_time_horizon, cem_num_rollouts, cem_num_elites, cem_num_iterations, cem_init_std = 5, 128, 12, 3, 0.2
        device, use_state_constraint, use_prior_model = DEV, True, True
        exact_gp_training_iterations, exact_gp_kernel = 0, 'rbf'
        plot_cem_optimisation = plot_cem_terminal_states = False

    class Longer(Conf):
        mpc_time_horizon = 6

    a = problems.make_solver(problems.pendulum(n_train=60, seed=1), Conf())[0]
    b = problems.make_solver(problems.pendulum(n_train=80, seed=2), Longer())[0]
    with pytest.raises(ValueError):
        get_actions_multi([a, b], np.zeros((2, 2)))
    c = problems.make_solver(problems.pendulum(n_train=80, seed=2, beta=2.0), Conf())[0]
    with pytest.raises(ValueError):
        get_actions_multi([a, c], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        MultiModelCemMpc([a.ssm], a._solver()._env, 5, 128, 12, 3, device=DEV, process_group=object())
