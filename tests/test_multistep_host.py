"""CPU: multi-step reachability under a feedback gain per rollout and step, host side -- the chained numpy oracle
(tests/multistep_oracle.py) against the reference's own multistep_reachability (tests/golden/multistep_*.npz);
sx_cem_rollout_gains and its form query declared, exported, bound, checking their arguments before any device access and
answering the form sx_cem_rollout_starts_form answers; the new translation unit named in build.sh;
`multistep_reachability`'s shape handling over a fake library; and `run_uncertainty_propagation` over a scripted linear
environment with `multistep_reachability` replaced by the oracle: draw order, dictionary, shapes, closed-loop law, inside
test.

Tolerance of the golden comparison: 1e-12 relative to max(1, max |Q_t|) (measured on the build machine: 9e-17 at the
pendulum, 5e-16 at the cart-pole)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import multistep_oracle as mo
from safe_exploration_amd import _lib, cem_mpc, gp_reachability_pytorch as grp
from safe_exploration_amd import uncertainty_propagation_runner as upr
from test_static_explore_host import _env, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
ENTRIES = ['sx_cem_rollout_gains', 'sx_cem_rollout_gains_form']


# ---- the oracle against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n_s', [('pendulum', 2), ('cartpole', 4)])
def test_chained_oracle_equals_the_reference(name, n_s):
    g, gp = mo.load_golden(os.path.join(GOLDEN, f'multistep_{name}.npz'))
    R, n = g['k_ff'].shape[:2]
    assert R >= 8 and n == 4 and g['p_0'].shape == (R, n_s) and g['k_fb'].shape == (R, n - 1, 1, n_s)
    p_all, q_all, _, status = mo.multistep(gp, g['p_0'], g['k_fb'], g['k_ff'], g['l_mu'], g['l_sigma'], float(g['c_safety']),
                                           g['a'], g['b'])
    ep, eq = mo.rel_err(p_all, g['p_all'], g['q_all']), mo.rel_err(q_all, g['q_all'], g['q_all'])
    print(f'{name}: {R} rollouts, max |Q| {np.abs(g["q_all"]).max():.3g}, centres {ep:.2e}, shapes {eq:.2e}')
    assert not status.any()
    assert ep <= 1e-12 and eq <= 1e-12
    # the gains matter: with every gain zero the shapes differ
    q_zero = mo.multistep(gp, g['p_0'], 0.0 * g['k_fb'], g['k_ff'], g['l_mu'], g['l_sigma'], float(g['c_safety']), g['a'],
                          g['b'])[1]
    assert mo.rel_err(q_zero, g['q_all'], g['q_all']) > 1e-6


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ENTRIES)
def test_entries_are_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    assert re.search(r'\bint ' + name + r'\(', header)
    assert name in _lib.SIGNATURES
    fn = getattr(_lib.lib(), name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert len(fn.argtypes) == (16 if name == 'sx_cem_rollout_gains' else 2)


def test_header_comment_names_what_the_entry_replaces():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    comment = header[:header.index('int sx_cem_rollout_gains(')].rsplit('/*', 1)[1]
    assert 'Replaces:' in comment and 'gp_reachability.py:168-221' in comment
    assert 'uncertainty_propagation_runner.py:28-41' in comment and 'env->k_fb is NOT read' in comment


def _call(*, model=(), env=(), no_model=False, no_env=False, E=2, P=4, H=5, mean=16, std=16, noise=16, rows=16, gains=16,
          obj=16, con=16, status=16):
    """sx_cem_rollout_gains over pointers that are never dereferenced: every call is answered before any device access."""
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    m, e = _model(*model), _env(*env)
    return _lib.lib().sx_cem_rollout_gains(None if no_model else ctypes.byref(m), None if no_env else ctypes.byref(e), E, P, H,
                                           p(mean), p(std), p(noise), p(rows), p(gains), None, None, p(obj), p(con),
                                           p(status), None)


REFUSALS = [
    ('gains null with H > 1', dict(gains=None), ARG),
    ('gains null with H = 2', dict(gains=None, H=2), ARG),
    ('model and env disagree on n_u', dict(model=(2, 2)), ARG),
    ('model and env disagree on n_s', dict(env=(4, 1)), ARG),
    # the cases of sx_cem_rollout_starts
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
    ('n_train = 0', dict(model=(2, 1, 0)), ARG),
    ('a null pointer before an uncompiled shape', dict(model=(3, 2), env=(3, 2), gains=None), ARG),
    ('a shape without a rollout kernel', dict(model=(3, 2), env=(3, 2)), UNSUPPORTED),
    ('m > SX_MAX_M', dict(env=(2, 1, 17)), UNSUPPORTED),
    ('m = 0', dict(env=(2, 1, 0)), UNSUPPORTED),
    ('a training set on the workspace path', dict(model=(2, 1, 2000)), UNSUPPORTED),
    ('n_s = 1 has no output-by-output form', dict(model=(1, 1, 1000), env=(1, 1), H=600), UNSUPPORTED),
    # H = 1 reads no gain: the NULL pointer passes the argument check and the call reaches the next one
    ('gains null with H = 1 is no argument error', dict(gains=None, H=1, env=(2, 1, 0)), UNSUPPORTED),
]


@pytest.mark.parametrize('what,kw,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_without_a_gpu(what, kw, code):
    assert _call(**kw) == code


@pytest.mark.parametrize('n_s,n_u', [(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2), (3, 2)])
def test_form_query_is_the_starts_form(n_s, n_u):
    lib = _lib.lib()
    seen = set()
    for H in (1, 3, 15, 400):
        for N in list(range(1, 1200, 13)) + [2000]:
            m = _model(n_s, n_u, N)
            got = int(lib.sx_cem_rollout_gains_form(ctypes.byref(m), H))
            assert got == int(lib.sx_cem_rollout_starts_form(ctypes.byref(m), H)), (N, H)
            seen.add(got)
    assert seen == ({-1} if (n_s, n_u) == (3, 2) else {0, -1} if n_s == 1 else {0, 3, -1})
    assert int(lib.sx_cem_rollout_gains_form(None, 3)) < 0 and int(lib.sx_cem_rollout_gains_form(ctypes.byref(m), 0)) < 0


def test_the_translation_unit_is_built():
    csrc = os.path.join(ROOT, 'safe_exploration_amd', 'csrc')
    assert re.search(r'\bsx_stream_gains\.hip\b', open(os.path.join(csrc, 'build.sh')).read())
    unit = open(os.path.join(csrc, 'sx_stream_gains.hip')).read()
    assert 'StreamGains' in unit and 'SX_ROLLOUT_SHAPES' in unit


# ---- multistep_reachability over a fake library --------------------------------------------------------------------------
class _Ssm:
    kernel_family = 'rbf'
    num_states, num_actions = 2, 1
    device_model = _lib.SxGpModel()


def _fake_library(monkeypatch, form=0):
    calls = []

    class Lib:
        def sx_cem_rollout_gains_form(self, model, H):
            return form

        def sx_cem_rollout_gains(self, model, env, E, P, H, mean, std, noise, rows, gains, traj, sigma, obj, con, status,
                                 stream):
            calls.append(dict(E=E, P=P, H=H, mean=mean, noise=noise, rows=rows, gains=gains, traj=traj, sigma=sigma,
                              beta=env._obj.beta, k_fb=list(env._obj.k_fb), m=env._obj.m))
            return 0

    monkeypatch.setattr(_lib, 'lib', lambda: Lib())
    monkeypatch.setattr(_lib, 'stream_ptr', lambda dev: None)
    monkeypatch.setattr(_lib, 'require_gpu', lambda t, name: None)
    monkeypatch.setattr(torch, 'empty', torch.zeros)      # the fake writes nothing: the outputs are zeros
    return calls


def test_multistep_reachability_batched_shapes(monkeypatch):
    calls = _fake_library(monkeypatch)
    R, n = 5, 4
    t = lambda *s: torch.ones(s, dtype=torch.float64)
    p_new, q_new, p_all, q_all = grp.multistep_reachability(t(R, 2), _Ssm(), t(R, n - 1, 1, 2), t(R, n, 1), t(2), t(2),
                                                            c_safety=2.5, verbose=0)
    assert tuple(p_new.shape) == (R, 2) and tuple(q_new.shape) == (R, 2, 2)
    assert tuple(p_all.shape) == (R, n, 2) and tuple(q_all.shape) == (R, n, 2, 2)
    assert len(calls) == 1                                              # all rollouts in ONE launch
    c = calls[0]
    assert (c['E'], c['P'], c['H']) == (1, R, n) and c['beta'] == 2.5 and c['m'] == 1
    assert c['rows'] is not None and c['gains'] is not None and c['traj'] is not None
    assert c['noise'] is None and c['mean'] is None and c['sigma'] is None
    assert not any(c['k_fb'])                                           # no gain goes through the environment


def test_multistep_reachability_reference_shapes(monkeypatch):
    calls = _fake_library(monkeypatch)
    n = 3
    t = lambda *s: torch.ones(s, dtype=torch.float64)
    p_new, q_new, p_all, q_all = grp.multistep_reachability(t(2, 1), _Ssm(), t(n - 1, 1, 2), t(n, 1), t(2), t(2), verbose=0)
    assert tuple(p_new.shape) == (2, 1) and tuple(q_new.shape) == (2, 2)
    assert tuple(p_all.shape) == (n, 2) and tuple(q_all.shape) == (n, 2, 2)
    assert len(calls) == 1 and (calls[0]['E'], calls[0]['P'], calls[0]['H']) == (1, 1, n)
    # one step: no gain to hand over
    grp.multistep_reachability(t(2, 1), _Ssm(), t(0, 1, 2), t(1, 1), t(2), t(2), verbose=0)
    assert calls[1]['H'] == 1 and calls[1]['gains'] is None


def test_multistep_reachability_refuses_what_it_does_not_build(monkeypatch):
    calls = _fake_library(monkeypatch)
    t = lambda *s: torch.ones(s, dtype=torch.float64)
    args = (t(3, 2), _Ssm(), t(3, 2, 1, 2), t(3, 3, 1), t(2), t(2))
    with pytest.raises(NotImplementedError, match='initial ellipsoid'):
        grp.multistep_reachability(*args, q_0=t(3, 2, 2))
    with pytest.raises(NotImplementedError, match='initial ellipsoid'):
        grp.multistep_reachability(*args, k_fb_init=t(1, 2))
    with pytest.raises(Exception):
        grp.multistep_reachability(t(3, 2), _Ssm(), t(3, 1, 1, 2), t(3, 3, 1), t(2), t(2))      # n - 1 gains wanted
    assert not calls


def test_models_without_the_fused_form_go_step_by_step(monkeypatch):
    calls = _fake_library(monkeypatch, form=-1)
    steps = []
    monkeypatch.setattr(grp, 'onestep_reachability', lambda p, ssm, k_ff, l_mu, l_sigma, q, k_fb, *a: steps.append(
        (tuple(p.shape), tuple(k_ff.shape), q is None, None if k_fb is None else k_fb.clone())) or (
        p + 1.0, torch.eye(2, dtype=torch.float64)[None], p))
    R, n = 2, 3
    k_fb = torch.arange(R * (n - 1) * 2, dtype=torch.float64).reshape(R, n - 1, 1, 2)
    t = lambda *s: torch.zeros(s, dtype=torch.float64)
    _, _, p_all, q_all = grp.multistep_reachability(t(R, 2), _Ssm(), k_fb, t(R, n, 1), t(2), t(2), verbose=0)
    assert not calls and len(steps) == R * n
    for i in range(R):
        for s in range(n):
            shape_p, shape_u, point, gain = steps[i * n + s]
            assert shape_p == (1, 2) and shape_u == (1, 1) and point == (s == 0)
            assert gain is None if s == 0 else torch.equal(gain, k_fb[i, s - 1])
    assert torch.equal(p_all[:, :, 0], torch.tensor([[1.0, 2.0, 3.0]] * R, dtype=torch.float64))
    feature = type('F', (_Ssm,), dict(kernel_family='feature'))()
    assert grp.fused_gains_form(feature, 3) == -1 and grp.fused_gains_form(_Ssm(), 3) == -1


def test_cem_rollout_gains_checks_the_gains(monkeypatch):
    rows = torch.zeros((1, 4, 2 + 3), dtype=torch.float64)
    monkeypatch.setattr(_lib, 'require_gpu', lambda t, name: None)
    for gains in (None, torch.zeros((1, 4, 3, 1, 2), dtype=torch.float64), torch.zeros((1, 4, 2, 1, 2), dtype=torch.float32)):
        with pytest.raises(ValueError, match='gains must be'):
            cem_mpc.cem_rollout_gains(_Ssm(), _env(), 3, rows=rows, gains=gains)


# ---- the runner over a scripted linear environment --------------------------------------------------------------------------
class LinearEnv:
    """x' = A x + B u, starts scripted: reset() draws from numpy's global generator, as the reference's does."""
    n_s, n_u = 2, 1
    l_mu, l_sigm = np.array([0.05, 0.05]), np.array([0.05, 0.05])
    A, B = np.array([[0.9, 0.1], [-0.05, 0.95]]), np.array([[0.0], [0.2]])

    def __init__(self):
        self.actions = []

    def reset(self):
        return 0.1 * np.random.rand(self.n_s)

    def simulate_onestep(self, state, action):
        u = np.asarray(action, dtype=np.float64).reshape(-1)
        self.actions.append((np.array(state, dtype=np.float64), u.copy()))
        nxt = self.A @ np.asarray(state) + self.B @ u
        return nxt, nxt


class LinearGp:
    """A 'GP' with a linear mean and a constant variance, in the oracle's predict form."""

    def predict(self, z, jacobians=True):
        M = np.array([[0.02, -0.01, 0.03], [0.01, 0.02, -0.02]])
        m = z @ M.T
        return m, np.full((len(z), 2), 4e-4), (np.broadcast_to(M, (len(z), 2, 3)).copy() if jacobians else None)


def _oracle_multistep(gp):
    def fake(p_0, ssm, k_fb, k_ff, l_mu, l_sigma, q_0=None, c_safety=1., verbose=1, a=None, b=None, k_fb_init=None):
        h = lambda x: None if x is None else x.detach().cpu().numpy()
        p_all, q_all, _, status = mo.multistep(gp, h(p_0), h(k_fb), h(k_ff), h(l_mu), h(l_sigma), c_safety, h(a), h(b))
        assert not status.any()
        fake.seen = dict(p_0=h(p_0), k_fb=h(k_fb), k_ff=h(k_ff), c_safety=c_safety, a=h(a), b=h(b), ssm=ssm)
        return p_all[:, -1], q_all[:, -1], p_all, q_all
    return fake


def _runner_conf(tmp_path=None, n_rollouts=6, n_safe=3):
    return types.SimpleNamespace(n_rollouts=n_rollouts, n_safe=n_safe, beta_safety=2.0, verbosity=1,
                                 save_results=tmp_path is not None, save_path=str(tmp_path), device='cpu')


def test_runner_over_a_scripted_linear_environment(monkeypatch, tmp_path, capsys):
    env, gp = LinearEnv(), LinearGp()
    safempc = types.SimpleNamespace(ssm=types.SimpleNamespace(x_train=None), lin_model=(env.A, env.B), n_safe=3)
    fake = _oracle_multistep(gp)
    monkeypatch.setattr(grp, 'multistep_reachability', fake)
    conf = _runner_conf(tmp_path)
    R, n = conf.n_rollouts, conf.n_safe
    np.random.seed(12)
    res = upr.run_uncertainty_propagation(env, safempc, conf)
    # the reference's draw order, per rollout: gains, feed-forward terms, start
    np.random.seed(12)
    for i in range(R):
        k_fb = .1 * np.random.randn(n - 1, 1, 2)
        k_ff = .1 * np.random.randn(n, 1)
        x_0 = 0.1 * np.random.rand(2)
        np.testing.assert_array_equal(fake.seen['k_fb'][i], k_fb)
        np.testing.assert_array_equal(fake.seen['k_ff'][i], k_ff)
        np.testing.assert_array_equal(fake.seen['p_0'][i], x_0)
    assert fake.seen['c_safety'] == 2.0 and fake.seen['ssm'] is safempc.ssm
    np.testing.assert_array_equal(fake.seen['a'], env.A)
    np.testing.assert_array_equal(fake.seen['b'], env.B)
    # the reference's dictionary and shapes
    assert list(res) == ['inside_ellipsoid_per_step', 'inside_ellipsoid_all', 'x_all', 'p_all', 'q_all']
    assert res['inside_ellipsoid_per_step'].shape == (R, n) and res['inside_ellipsoid_all'].shape == (R,)
    assert res['x_all'].shape == (R, n + 1, 2) and res['p_all'].shape == (R, n, 2) and res['q_all'].shape == (R, n, 2, 2)
    saved = np.load(os.path.join(str(tmp_path), 'res_data.npy'), allow_pickle=True).item()
    assert list(saved) == list(res) and all(np.array_equal(saved[k], res[k]) for k in res)
    # the closed-loop law on the true system: u_0 = k_ff_0, u_i = K_{i-1} (x_i - p_{i-1}) + k_ff_i
    assert len(env.actions) == R * n
    for i in range(R):
        np.testing.assert_array_equal(res['x_all'][i, 0], fake.seen['p_0'][i])
        x = res['x_all'][i, 0]
        for s in range(n):
            u = fake.seen['k_ff'][i, s] if s == 0 else \
                fake.seen['k_fb'][i, s - 1] @ (x - res['p_all'][i, s - 1]) + fake.seen['k_ff'][i, s]
            state, action = env.actions[i * n + s]
            np.testing.assert_array_equal(state, x)
            np.testing.assert_allclose(action, u, rtol=0, atol=1e-15)
            x = env.A @ x + env.B @ action
            np.testing.assert_allclose(res['x_all'][i, s + 1], x, rtol=0, atol=1e-15)
    # the inside flags, recomputed
    for i in range(R):
        for s in range(n):
            d = res['x_all'][i, s + 1] - res['p_all'][i, s]
            inside = d @ np.linalg.inv(res['q_all'][i, s]) @ d < 1.0
            assert bool(res['inside_ellipsoid_per_step'][i, s]) == bool(inside)
        assert bool(res['inside_ellipsoid_all'][i]) == bool(res['inside_ellipsoid_per_step'][i].all())
    out = capsys.readouterr().out
    assert 'Uncertainty propagation' in out and 'Trajectory safety percentage' in out


def test_inside_test_at_the_centre_and_two_semi_axes_out():
    class Still:
        def simulate_onestep(self, state, action):
            return np.asarray(state, dtype=np.float64), None

    q = np.diag([0.04, 0.25])                        # semi-axes 0.2 and 0.5
    k_ff, k_fb = np.zeros((2, 1)), np.zeros((1, 1, 2))
    centre = np.array([0.3, -0.1])
    p_all, q_all = np.stack((centre, centre)), np.stack((q, q))
    assert upr.trajectory_inside_ellipsoid(Still(), centre, p_all, q_all, k_fb, k_ff).tolist() == [True, True]
    out = centre + np.array([0.0, 2 * 0.5])
    assert upr.trajectory_inside_ellipsoid(Still(), out, p_all, q_all, k_fb, k_ff).tolist() == [False, False]
    assert upr.trajectory_inside_ellipsoid(Still(), centre + np.array([0.19, 0.0]), p_all, q_all.reshape(2, 4), k_fb,
                                           k_ff).tolist() == [True, True]
    assert upr.inside_ellipsoid(centre + np.array([0.2, 0.0]), centre, q) is False        # the boundary is outside: d < 1
