"""GPU: the fused rollout of JunkDimensionsSSM over feature-space GPs ('linear', 'nn') and MC-dropout models
(sx_cem_rollout_feat_junk / sx_cem_rollout_mlp_junk, kernel_family 'feature_junk' / 'mlp_junk') against the step-by-step
rollout through the wrapper; the kept-column model against the padded one; which entry points CemSafeMPC.get_action calls,
and its action against the same solve step by step.  The MC-dropout cases run on the matrix-core kernels and with
SX_MLP_PATH=valu on the one-particle-per-lane kernels."""
import collections
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


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
    mc_dropout_training_iterations = 25
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
# with the log-std head (one hidden layer, fewer members than waves); 'gal': GalConcreteDropoutSSM (mc_dropout_predict_std)
KINDS = {'linear': dict(exact_gp_kernel='linear'), 'nn': dict(exact_gp_kernel='nn'),
         'mc_dropout': dict(),
         'mc_dropout_std': dict(mc_dropout_type='concrete', mc_dropout_predict_std=True, mc_dropout_hidden_features=[24],
                                mc_dropout_num_samples=6),
         'gal': dict(mc_dropout_type='concrete', mc_dropout_predict_std=True, mc_dropout_hidden_features=[16, 12])}
MLP_KINDS = ('mc_dropout', 'mc_dropout_std', 'gal')


def constructor(kind):
    from safe_exploration_amd.ssm_cem.dropout_ssm_cem import McDropoutSSM
    from safe_exploration_amd.ssm_cem.gal_concrete_dropout import GalConcreteDropoutSSM
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    conf = type('C', (Conf,), KINDS[kind])()
    cls = GpCemSSM if kind in ('linear', 'nn') else GalConcreteDropoutSSM if kind == 'gal' else McDropoutSSM
    return functools.partial(cls, conf)


def base_spec(n_s, n_u, n_train, seed=0):
    """The pendulum; a stable synthetic system for (2, 2)."""
    from safe_exploration_amd import problems
    if (n_s, n_u) == (2, 1):
        return problems.pendulum(n_train=n_train, seed=seed)
    rng = np.random.default_rng(100 + 10 * n_s + n_u)
    X, Y = problems.synthetic_training_set(n_train, n_s, n_u, seed=seed)
    return problems.ProblemSpec('synthetic', n_s, n_u, X, Y, rng.uniform(0.6, 1.4, size=(n_s, n_s + n_u)),
                                np.full(n_s, 0.05), np.full(n_s, 1e-4), 0.95 * np.eye(n_s),
                                rng.uniform(-0.1, 0.1, size=(n_s, n_u)), rng.uniform(-0.3, 0.0, size=(n_u, n_s)),
                                np.full(n_s, 0.05), np.full(n_s, 0.05), 2.0, np.vstack((np.eye(n_s), -np.eye(n_s))),
                                np.ones((2 * n_s, 1)), np.full(n_u, -1.0), np.full(n_u, 1.0))


def model_case(kind, n_s, n_u, js, ja, n_train=60, seed=0):
    """(wrapper over the inner model with data, sx_env, spec)"""
    from safe_exploration_amd import problems
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    spec = base_spec(n_s, n_u, n_train, seed)
    ssm = JunkDimensionsSSM(constructor(kind), state_dimen=n_s, action_dimen=n_u, junk_states=js, junk_actions=ja)
    if kind in ('linear', 'nn'):
        rng = np.random.default_rng(7 + js + 3 * ja)
        ssm._ssm.set_hyperparameters(kernel_scale=rng.uniform(0.3, 0.8, size=n_s + js),
                                     noise=rng.uniform(1e-3, 4e-3, size=n_s + js))
    ssm.update_model(T(spec.X), T(spec.Y), replace_old=True)
    _, env = problems.build(spec, device=DEV)
    return ssm, env, spec


def stepwise_through_wrapper(ssm, env, x0, acts):
    """The rollout of one problem step by step through the wrapper (its predict_* + sx_onestep_reach), recording
    centres, shapes and the variances: the path cem_rollout_stepwise takes."""
    import ctypes

    from safe_exploration_amd import _lib
    P, H, _ = acts.shape
    n_s = ssm.num_states
    p, q = x0.reshape(1, n_s).expand(P, n_s).contiguous(), None
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ps, qs, sigmas = [], [], []
    for t in range(H):
        u = acts[:, t].contiguous()
        if q is None:
            (mean, var), jac = ssm.predict_without_jacobians(p, u), None
        else:
            mean, var, jac = ssm.predict_with_jacobians(p, u)
            jac = jac.contiguous()
        mean, var = mean.contiguous(), var.contiguous()
        p1, q1, sig = torch.empty_like(p), torch.empty((P, n_s, n_s), dtype=torch.float64, device=DEV), torch.empty_like(p)
        _lib.check(_lib.lib().sx_onestep_reach(ctypes.byref(env), P, _lib.ptr(p), _lib.ptr(q), _lib.ptr(u),
                                               _lib.ptr(mean), _lib.ptr(var), _lib.ptr(jac),
                                               _lib.ptr(p1), _lib.ptr(q1), _lib.ptr(sig), _lib.ptr(status),
                                               _lib.stream_ptr(torch.device(DEV))), 'sx_onestep_reach')
        ps.append(p1), qs.append(q1), sigmas.append(sig)
        p, q = p1, q1
    return torch.stack(ps, 1), torch.stack(qs, 1), torch.stack(sigmas, 1), int(status.item())


def close(a, b, rtol=1e-10, atol=1e-12):
    np.testing.assert_allclose(a.cpu().numpy() if torch.is_tensor(a) else a, b.cpu().numpy() if torch.is_tensor(b) else b,
                               rtol=rtol, atol=atol)


# (n_s, n_u, J_s, J_a): the pendulum with junk states (and a junk action), and (2, 2) with the largest query shift.
# ((2, 1, 1, 1) pads to (3, 2), for which the inner model has no sx_*_predict: there is no step-by-step rollout to compare.)
SHAPES = [(2, 1, 1, 0), (2, 1, 2, 0), (2, 1, 2, 1), (2, 2, 2, 0)]


def _check_fused_against_stepwise(kind, n_s, n_u, js, ja):
    from safe_exploration_amd.cem_mpc import cem_rollout, cem_rollout_stepwise
    ssm, env, spec = model_case(kind, n_s, n_u, js, ja)
    family = 'feature_junk' if kind in ('linear', 'nn') else 'mlp_junk'
    assert ssm.kernel_family == family and ssm.query_shift == min(js, n_u)
    H = 5
    rng = np.random.default_rng(n_s + 10 * js + 100 * ja)
    # E = 2; P = 37 is no multiple of the 16-particle tile or the 64-lane wave; 2 x 8250 particles need more than one
    # workgroup per CU on either kernel (258 one-wave workgroups, 1032 matrix-core tiles)
    for E, P in ((2, 37), (2, 8250)):
        x0 = rng.normal(0, 0.05, size=(E, n_s))
        acts = rng.normal(0, 0.3, size=(E, P, H, n_u))
        r = cem_rollout(ssm, env, T(x0), H, actions=T(acts), want_traj=True, want_sigma=True)
        S = n_s + n_s * n_s
        st_fused = int(r['status'].item())
        for e in range(E):
            p, q, sig, st = stepwise_through_wrapper(ssm, env, T(x0[e]), T(acts[e]))
            assert st == st_fused == 0
            traj = r['traj'][e].view(P, H, S)
            close(traj[..., :n_s], p)
            close(traj[..., n_s:].reshape(P, H, n_s, n_s), q)
            close(r['sigma'][e], sig)
            ref = cem_rollout_stepwise(ssm, env, T(x0[e]), T(acts[e]), status=torch.zeros(1, dtype=torch.int32, device=DEV))
            close(r['obj_cost'][e], ref['obj_cost'])
            if P < 100:
                close(r['con_cost'][e], ref['con_cost'], rtol=0, atol=0)
            else:   # (a centre within rounding of a polytope face may land on either side of it; none is expected)
                assert int((r['con_cost'][e] != ref['con_cost']).sum()) <= 2


@pytest.mark.parametrize('kind', ['linear', 'nn'])
@pytest.mark.parametrize('n_s,n_u,js,ja', SHAPES)
def test_fused_feature_junk_rollout_matches_the_step_by_step_rollout(kind, n_s, n_u, js, ja):
    _check_fused_against_stepwise(kind, n_s, n_u, js, ja)


@pytest.mark.parametrize('kind', MLP_KINDS)
@pytest.mark.parametrize('n_s,n_u,js,ja', SHAPES)
def test_fused_mlp_junk_rollout_matches_the_step_by_step_rollout(kind, n_s, n_u, js, ja, mlp_path):
    _check_fused_against_stepwise(kind, n_s, n_u, js, ja)


# views whose shape sx_*_predict is instantiated for: (2, 2) -- the pendulum's (n_s, n_u + s)
VIEW_SHAPES = [(2, 1, 1, 0), (2, 1, 2, 0), (2, 1, 2, 1)]


def _check_view(kind, n_s, n_u, js, ja):
    """The view's posterior at [x, 0_s, u] is the wrapper's at (x, u); its Jacobian's leading n_s + n_u columns are the
    wrapper's Jacobian.  (Views of a shape sx_*_predict is instantiated for; the others serve the fused rollout alone.)"""
    ssm, _, _ = model_case(kind, n_s, n_u, js, ja)
    view = ssm.real_output_view()
    s = ssm.query_shift
    rng = np.random.default_rng(4)
    for P in (1, 37, 300):
        x, u = T(rng.normal(0, 0.3, size=(P, n_s))), T(rng.normal(0, 0.5, size=(P, n_u)))
        m, v, j = ssm.predict_with_jacobians(x, u)
        mv, vv, jv = view.predict_with_jacobians(x, torch.cat((torch.zeros_like(u[:, :1]).expand(P, s), u), 1))
        close(mv, m, rtol=1e-12, atol=1e-12)
        close(vv, v, rtol=1e-12, atol=1e-12)
        close(jv[:, :, :n_s + n_u], j, rtol=1e-12, atol=1e-12)
    # new data is a new device model: the view follows
    x_new, y_new = T(rng.normal(0, 0.3, size=(5, n_s + n_u))), T(rng.normal(0, 0.01, size=(5, n_s)))
    ssm.update_model(x_new, y_new)
    assert ssm.real_output_view() is not view


@pytest.mark.parametrize('kind', ['linear', 'nn'])
@pytest.mark.parametrize('n_s,n_u,js,ja', VIEW_SHAPES)
def test_kept_column_feature_view_equals_the_padded_model(kind, n_s, n_u, js, ja):
    _check_view(kind, n_s, n_u, js, ja)


@pytest.mark.parametrize('kind', MLP_KINDS)
@pytest.mark.parametrize('n_s,n_u,js,ja', VIEW_SHAPES)
def test_kept_column_mlp_view_equals_the_padded_model(kind, n_s, n_u, js, ja, mlp_path):
    _check_view(kind, n_s, n_u, js, ja)


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


@pytest.mark.parametrize('kind,n_u,js,ja', [('linear', 1, 2, 1), ('nn', 1, 1, 0), ('mc_dropout', 1, 2, 0),
                                            ('gal', 1, 1, 0), ('nn', 2, 2, 0), ('mc_dropout_std', 2, 2, 0)])
def test_get_action_through_junk_dimensions_is_fused_and_matches_step_by_step(kind, n_u, js, ja, monkeypatch):
    """CemSafeMPC.get_action over the wrapper: one sx_cem_rollout_*_junk launch per CEM iteration and no
    sx_feat_predict / sx_mlp_predict / sx_onestep_reach; the selected action plan equals the same solve step by step with
    the same noise."""
    from safe_exploration_amd import _lib, problems
    from safe_exploration_amd.safempc_cem import CemSafeMPC, MpcResult, construct_constraints
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    n_s = 2
    spec = base_spec(n_s, n_u, 90, seed=5)
    env = problems.StubEnv(spec, np.zeros(n_s))
    ssm = JunkDimensionsSSM(constructor(kind), state_dimen=n_s, action_dimen=n_u, junk_states=js, junk_actions=ja)
    if kind in ('linear', 'nn'):
        ssm._ssm.set_hyperparameters(kernel_scale=0.05, noise=1e-4)
    c = Conf
    solver = CemSafeMPC(ssm, construct_constraints(c(), env), env, c(), {'lin_model': (spec.a, spec.b)},
                        wx_feedback_cost=np.diag([1.0, 2.0]), wu_feedback_cost=25.0 * np.eye(n_u), beta_safety=spec.beta,
                        safe_policy=lambda x: spec.k_fb @ x)
    y = spec.Y + spec.X[:, :n_s] @ spec.a.T + spec.X[:, n_s:] @ spec.b.T
    solver.update_model(spec.X, y, opt_hyp=False, replace_old=True)
    family = 'feature_junk' if kind in ('linear', 'nn') else 'mlp_junk'
    assert ssm.kernel_family == family
    rng = np.random.default_rng(8 + js)
    noise = rng.normal(size=(c.cem_num_iterations, c.cem_num_rollouts, c.mpc_time_horizon, n_u))
    x0 = np.full(n_s, 0.01)
    mpc = solver._solver()
    it = iter(noise)
    mpc.sample_noise = lambda episodes=1: T(next(it)[None])
    ssm.real_output_view()          # (built before counting: its fit is not part of the solve's path)
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: counting)
    _, result = solver.get_action(x0)
    torch.cuda.synchronize()
    monkeypatch.undo()
    calls = counting.calls
    entry = 'sx_cem_rollout_feat_junk' if family == 'feature_junk' else 'sx_cem_rollout_mlp_junk'
    assert calls[entry] == c.cem_num_iterations, dict(calls)
    for name in ('sx_feat_predict', 'sx_mlp_predict', 'sx_onestep_reach', 'sx_cem_rollout_feat', 'sx_cem_rollout_mlp'):
        assert calls[name] == 0, (name, dict(calls))
    assert mpc.stepwise_fallbacks == 0
    best, ok, _, status = mpc.solve(T(x0[None]), noise=T(noise[:, None]), stepwise=True)
    assert int(status.item()) == 0
    assert bool(ok[0].item()) == (result == MpcResult.FOUND_SOLUTION)
    if result == MpcResult.FOUND_SOLUTION:
        np.testing.assert_allclose(solver._last_mpc_actions, best[0].cpu().numpy(), rtol=0, atol=1e-9)
