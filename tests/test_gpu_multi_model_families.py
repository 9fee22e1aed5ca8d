"""GPU: E problems with a feature-space GP ('linear', 'nn') or an MC-dropout ensemble each in one rollout launch
(sx_cem_rollout_feat_multi / sx_cem_rollout_mlp_multi), the multi-model solve over them (MultiModelCemMpc) and the
lockstep runner over one solver per scenario.  Reference: the single-model entry points problem by problem, which run the
same kernels' plain mode.  The MC-dropout cases run on the matrix-core kernels and with SX_MLP_PATH=valu on the
one-particle-per-lane kernels."""
import collections
import os

import numpy as np
import pytest
import torch

from safe_exploration_amd import _lib, problems
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc, cem_rollout, cem_rollout_multi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


@pytest.fixture(params=['mfma', 'valu'])
def mlp_path(request):
    """the library reads SX_MLP_PATH at every launch"""
    old = os.environ.pop('SX_MLP_PATH', None)
    if request.param == 'valu':
        os.environ['SX_MLP_PATH'] = 'valu'
    yield request.param
    os.environ.pop('SX_MLP_PATH', None)
    if old is not None:
        os.environ['SX_MLP_PATH'] = old


class Conf:
    exact_gp_training_iterations = 0
    nn_kernel_layers = [8, 6]
    nn_kernel_seed = 0
    mc_dropout_training_iterations = 20
    mc_dropout_hidden_features = [16, 16]
    mc_dropout_num_samples = 11
    mc_dropout_predict_std = False
    mc_dropout_reinitialize = False
    mc_dropout_type = 'fixed'
    mc_dropout_concrete_initial_probability = 0.1
    mc_dropout_fixed_probability = 0.1
    mc_dropout_on_input = True
    mc_dropout_lengthscale = 1e-4
    mc_dropout_seed = 3
    mpc_time_horizon = 5
    cem_num_rollouts = 200
    cem_num_elites = 20
    cem_num_iterations = 4
    cem_init_std = 0.2
    plot_cem_optimisation = False
    plot_cem_terminal_states = False
    use_state_constraint = True
    use_prior_model = True
    device = DEV


# 'linear' / 'nn': FeatureGpCemSSM; 'mc_dropout': fixed-rate dropout, two hidden layers; 'mc_dropout_std': concrete dropout
# with the log-std head (one hidden layer of 64: the straight-line matrix-core kernel); 'gal': GalConcreteDropoutSSM
KINDS = {'linear': dict(exact_gp_kernel='linear'), 'nn': dict(exact_gp_kernel='nn'),
         'mc_dropout': dict(),
         'mc_dropout_std': dict(mc_dropout_type='concrete', mc_dropout_predict_std=True, mc_dropout_hidden_features=[64],
                                mc_dropout_num_samples=6),
         'gal': dict(mc_dropout_type='concrete', mc_dropout_predict_std=True, mc_dropout_hidden_features=[16, 12])}
MLP_KINDS = ('mc_dropout', 'mc_dropout_std', 'gal')


def conf(kind, e=0):
    """The kind's settings; problem e's network gets its own initialisation and masks."""
    return type('C', (Conf,), dict(KINDS[kind], nn_kernel_seed=10 + e, mc_dropout_seed=3 + 7 * e))()


def make_ssm(kind, n_s, n_u, e=0):
    from safe_exploration_amd.ssm_cem.dropout_ssm_cem import McDropoutSSM
    from safe_exploration_amd.ssm_cem.gal_concrete_dropout import GalConcreteDropoutSSM
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    cls = GpCemSSM if kind in ('linear', 'nn') else GalConcreteDropoutSSM if kind == 'gal' else McDropoutSSM
    ssm = cls(conf(kind, e), n_s, n_u)
    if kind in ('linear', 'nn'):
        rng = np.random.default_rng(40 + e)
        ssm.set_hyperparameters(kernel_scale=rng.uniform(0.3, 0.8, size=n_s), noise=rng.uniform(1e-3, 4e-3, size=n_s))
    return ssm


def spec_of(system, N, seed):
    return problems.pendulum(n_train=N, seed=seed) if system == 'pendulum' else problems.cartpole(n_train=N, seed=seed)


# per system: (N, seed) of each problem -- different training sets and sizes
ROWS = {'pendulum': [(60, 1), (120, 2), (90, 3), (150, 4)], 'cartpole': [(80, 1), (140, 2), (100, 3)]}


def family_problems(kind, system):
    specs = [spec_of(system, N, seed) for N, seed in ROWS[system]]
    ssms = []
    for e, spec in enumerate(specs):
        ssm = make_ssm(kind, spec.n_s, spec.n_u, e)
        ssm.update_model(T(spec.X), T(spec.Y), replace_old=True)
        ssms.append(ssm)
    env = problems.build(specs[0], DEV)[1]          # one sx_env for all problems
    return specs, ssms, env


def _exact(a, b, what):
    """rtol 1e-12: the multi launch runs the single launch's arithmetic, so in practice bit-identical"""
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-12, atol=0, err_msg=what)


def _check_against_single(kind, ssms, env, x0, H, r, sampled, actions=None, mean=None, std=None, noise=None):
    E = len(ssms)
    assert r['status'].shape == (E,)
    for e in range(E):
        if sampled:
            one = cem_rollout(ssms[e], env, T(x0[e:e + 1]), H, mean=T(mean[e:e + 1]), std=T(std[e:e + 1]),
                              noise=T(noise[e:e + 1]), want_traj=True, want_sigma=True)
        else:
            one = cem_rollout(ssms[e], env, T(x0[e:e + 1]), H, actions=T(actions[e:e + 1]), want_traj=True,
                              want_sigma=True)
        keys = ('obj_cost', 'con_cost', 'traj', 'sigma') + (('actions',) if sampled else ())
        for key in keys:
            _exact(r[key][e], one[key][0], f'{kind}: problem {e} {key}')
        assert int(r['status'][e]) == int(one['status'][0]), (kind, e)


def _given(kind, system, P, H=5):
    specs, ssms, env = family_problems(kind, system)
    E, n_s, n_u = len(ssms), specs[0].n_s, specs[0].n_u
    rng = np.random.default_rng(11)
    x0 = rng.normal(0, 0.03, size=(E, n_s))
    actions = rng.normal(0, 0.3, size=(E, P, H, n_u))
    r = cem_rollout_multi(ssms, env, T(x0), H, actions=T(actions), want_traj=True, want_sigma=True)
    _check_against_single(kind, ssms, env, x0, H, r, False, actions=actions)


def _sampled(kind, system, P, H=4):
    specs, ssms, env = family_problems(kind, system)
    E, n_s, n_u = len(ssms), specs[0].n_s, specs[0].n_u
    rng = np.random.default_rng(12)
    x0 = rng.normal(0, 0.03, size=(E, n_s))
    mean, std = rng.normal(0, 0.1, size=(E, H, n_u)), rng.uniform(0.1, 0.4, size=(E, H, n_u))
    noise = rng.normal(size=(E, P, H, n_u))
    r = cem_rollout_multi(ssms, env, T(x0), H, mean=T(mean), std=T(std), noise=T(noise), want_traj=True, want_sigma=True)
    _check_against_single(kind, ssms, env, x0, H, r, True, mean=mean, std=std, noise=noise)


@pytest.mark.parametrize('P', [37, 8250])
@pytest.mark.parametrize('system', ['pendulum', 'cartpole'])
@pytest.mark.parametrize('kind', ['linear', 'nn'])
def test_feature_given_actions_match_single_model_rollouts(kind, system, P):
    _given(kind, system, P)


@pytest.mark.parametrize('P', [37, 8250])
@pytest.mark.parametrize('system', ['pendulum', 'cartpole'])
@pytest.mark.parametrize('kind', MLP_KINDS)
def test_mlp_given_actions_match_single_model_rollouts(kind, system, P, mlp_path):
    _given(kind, system, P)


@pytest.mark.parametrize('system', ['pendulum', 'cartpole'])
@pytest.mark.parametrize('kind', ['linear', 'nn'])
def test_feature_sampled_actions_match_single_model_rollouts(kind, system):
    _sampled(kind, system, 37)


@pytest.mark.parametrize('system', ['pendulum', 'cartpole'])
@pytest.mark.parametrize('kind', MLP_KINDS)
def test_mlp_sampled_actions_match_single_model_rollouts(kind, system, mlp_path):
    _sampled(kind, system, 37)


def _check_nan_isolation(kind):
    specs, ssms, env = family_problems(kind, 'pendulum')
    E, P, H, bad = len(ssms), 37, 4, 1
    # a NaN network weight in the device buffer problem `bad`'s model struct points at: every prediction of that model
    # is NaN -- (x, net, wbar, minv) of the feature GP, (net, masks) of the ensemble
    net = ssms[bad]._buffers[1] if kind == 'nn' else ssms[bad]._buffers[0]
    net[0] = float('nan')
    rng = np.random.default_rng(13)
    x0 = rng.normal(0, 0.03, size=(E, 2))
    actions = rng.normal(0, 0.3, size=(E, P, H, 1))
    r = cem_rollout_multi(ssms, env, T(x0), H, actions=T(actions))
    words = [int(w) for w in r['status'].tolist()]
    assert words[bad] & _lib.SX_STATUS_NAN, words
    for e in range(E):
        if e != bad:
            one = cem_rollout(ssms[e], env, T(x0[e:e + 1]), H, actions=T(actions[e:e + 1]))
            assert not words[e] & _lib.SX_STATUS_NAN and words[e] == int(one['status'][0]), (e, words)
            _exact(r['obj_cost'][e], one['obj_cost'][0], f'problem {e} obj_cost')
            _exact(r['con_cost'][e], one['con_cost'][0], f'problem {e} con_cost')


def test_a_nan_in_one_feature_gp_sets_only_its_own_status_word():
    _check_nan_isolation('nn')


def test_a_nan_in_one_ensemble_sets_only_its_own_status_word(mlp_path):
    _check_nan_isolation('mc_dropout')


@pytest.mark.parametrize('kind', ['linear', 'nn', 'mc_dropout', 'gal'])
def test_multi_model_solve_matches_sequential_solves(kind):
    specs, ssms, env = family_problems(kind, 'pendulum')
    E, H, P, k, iters = len(ssms), 5, 256, 20, 4
    rng = np.random.default_rng(5)
    noise = rng.normal(size=(iters, E, P, H, 1))
    x0 = rng.normal(0, 0.02, size=(E, 2))
    mpc = MultiModelCemMpc(ssms, env, H, P, k, iters, device=DEV, init_std=0.2)
    assert mpc.fused_applies()
    best, ok, status = mpc.solve(T(x0), noise=T(noise))
    assert status.shape == (E,)
    for e in range(E):
        one = FusedCemMpc(ssms[e], env, H, P, k, iters, device=DEV, init_std=0.2)
        b1, ok1, _, st1 = one.solve(T(x0[e:e + 1]), noise=T(noise[:, e:e + 1]))
        assert int(status[e]) == int(st1.reshape(-1)[0]), e
        assert bool(ok[e]) == bool(ok1[0]), e
        if bool(ok1[0]):   # (best is written for a feasible problem only)
            np.testing.assert_allclose(best[e].cpu().numpy(), b1[0].cpu().numpy(), rtol=0, atol=1e-9, err_msg=f'{e}')


class CountingLib:
    """libsxamd with a call counter per entry point."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def make_solver(kind, spec, e, env=None):
    """A CemSafeMPC over a model of `kind` with the spec's data (as problems.make_solver does for the exact GP)."""
    from safe_exploration_amd.safempc_cem import CemSafeMPC, construct_constraints
    env = env if env is not None else problems.StubEnv(spec, np.zeros(spec.n_s))
    c = conf(kind, e)
    ssm = make_ssm(kind, spec.n_s, spec.n_u, e)
    if kind in ('linear', 'nn'):
        # (a confident GP, as the junk-dimension solver tests use: the problems then have feasible plans)
        ssm.set_hyperparameters(kernel_scale=0.05 * (1 + 0.2 * e), noise=1e-4)
    solver = CemSafeMPC(ssm, construct_constraints(c, env), env, c, {'lin_model': (spec.a, spec.b)},
                        wx_feedback_cost=np.diag([1.0, 2.0]), wu_feedback_cost=25.0 * np.eye(spec.n_u),
                        beta_safety=spec.beta, safe_policy=lambda x: spec.k_fb @ x)
    y = spec.Y + spec.X[:, :spec.n_s] @ spec.a.T + spec.X[:, spec.n_s:] @ spec.b.T
    solver.update_model(spec.X, y, opt_hyp=False, replace_old=True)
    return solver, env


@pytest.mark.parametrize('kind', ['nn', 'mc_dropout'])
def test_get_actions_multi_takes_the_fused_path_and_matches_get_action(kind, monkeypatch):
    from safe_exploration_amd.safempc_cem import get_actions_multi
    specs = [problems.pendulum(n_train=N, seed=s) for N, s in ((70, 3), (110, 4), (90, 5))]
    states = problems.start_states(2, len(specs), seed=6, std=0.02)
    c = Conf

    def solvers():
        # (solver e of either set draws the same noise: the same seed, the same generator state)
        return [make_solver(kind, spec, e)[0] for e, spec in enumerate(specs)]

    seq = solvers()
    ref = [s.get_action(states[e]) for e, s in enumerate(seq)]
    multi = solvers()
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: counting)
    actions, results = get_actions_multi(multi, states)
    torch.cuda.synchronize()
    monkeypatch.undo()
    entry = 'sx_cem_rollout_feat_multi' if kind == 'nn' else 'sx_cem_rollout_mlp_multi'
    assert counting.calls[entry] == c.cem_num_iterations, dict(counting.calls)
    for name in ('sx_cem_rollout_feat', 'sx_cem_rollout_mlp', 'sx_feat_predict', 'sx_mlp_predict', 'sx_onestep_reach'):
        assert counting.calls[name] == 0, (name, dict(counting.calls))
    assert multi[0]._multi[1].per_model_solves == 0
    for e, (a, r) in enumerate(ref):
        assert results[e] == r, e
        np.testing.assert_allclose(actions[e], a, rtol=0, atol=1e-9, err_msg=f'scenario {e}')


@pytest.mark.parametrize('kind', ['nn', 'mc_dropout'])
def test_lockstep_runner_with_one_solver_per_scenario_matches_do_rollout(kind):
    from safe_exploration_amd.episode_runner import do_rollout, do_rollout_batch
    from safe_exploration_amd.safempc_cem import MpcResult
    specs = [problems.pendulum(n_train=N, seed=s) for N, s in ((60, 3), (100, 4), (80, 5))]
    x0s = problems.start_states(2, len(specs), seed=5, std=0.03)
    steps = 4

    def scenario(e):
        env = problems.StubEnv(specs[e], x0s[e])
        return make_solver(kind, specs[e], e, env)

    seq = []
    for e in range(len(specs)):
        solver, env = scenario(e)
        seq.append(do_rollout(env, steps, solver=solver))
    pairs = [scenario(e) for e in range(len(specs))]
    solvers, envs = [p[0] for p in pairs], [p[1] for p in pairs]
    res = do_rollout_batch(envs, steps, solvers)
    assert solvers[0]._multi is not None and solvers[0]._multi[1].per_model_solves == 0
    for e, (r, (xx, yy, cc, codes, failed)) in enumerate(zip(res, seq)):
        assert r.safety_failure == failed and r.xx.shape == xx.shape, e
        np.testing.assert_allclose(r.xx, xx, rtol=0, atol=1e-9, err_msg=f'scenario {e}')
        np.testing.assert_allclose(r.yy, yy, rtol=0, atol=1e-9, err_msg=f'scenario {e}')
        np.testing.assert_array_equal(r.exit_codes, codes)
    if kind == 'nn':   # (the briefly trained ensembles here are too uncertain for a certified plan: the ladder's fallbacks)
        assert any(MpcResult.FOUND_SOLUTION in r.mpc_results for r in res), [r.mpc_results for r in res]
