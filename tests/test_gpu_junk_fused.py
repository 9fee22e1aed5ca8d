"""GPU: the fused rollout of JunkDimensionsSSM over the exact RBF GP (sx_cem_rollout_junk / sx_cem_rollout_elites_junk,
kernel_family 'rbf_junk') against the step-by-step rollout through the wrapper and against the oracle's CEM over the
reference's padded GP; which entry points a solve calls; the step-by-step fall-back for training sets beyond the
single-launch kernel."""
import collections
import functools

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.gp import ExactGP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


class Conf:
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'
    device = DEV


def base_spec(n_s, n_u, n_train, seed=0):
    """The pendulum and the cart-pole; a stable synthetic system for the other shapes."""
    from safe_exploration_amd import problems
    if (n_s, n_u) == (2, 1):
        return problems.pendulum(n_train=n_train, seed=seed)
    if (n_s, n_u) == (4, 1):
        return problems.cartpole(n_train=n_train, seed=seed)
    rng = np.random.default_rng(100 + 10 * n_s + n_u)
    X, Y = problems.synthetic_training_set(n_train, n_s, n_u, seed=seed)
    return problems.ProblemSpec('synthetic', n_s, n_u, X, Y, rng.uniform(0.6, 1.4, size=(n_s, n_s + n_u)),
                                np.full(n_s, 0.05), np.full(n_s, 1e-4), 0.95 * np.eye(n_s),
                                rng.uniform(-0.1, 0.1, size=(n_s, n_u)), rng.uniform(-0.3, 0.0, size=(n_u, n_s)),
                                np.full(n_s, 0.05), np.full(n_s, 0.05), 2.0, np.vstack((np.eye(n_s), -np.eye(n_s))),
                                np.ones((2 * n_s, 1)), np.full(n_u, -1.0), np.full(n_u, 1.0))


def junk_case(n_s, n_u, js, ja, n_train=60, seed=0):
    """(wrapper over GpCemSSM with data, sx_env, spec, padded hyper-parameters (ls, s, noise) of the reference's model)."""
    from safe_exploration_amd import problems
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    spec = base_spec(n_s, n_u, n_train, seed)
    ssm = JunkDimensionsSSM(functools.partial(GpCemSSM, Conf()), state_dimen=n_s, action_dimen=n_u, junk_states=js,
                            junk_actions=ja)
    rng = np.random.default_rng(7 + js + 3 * ja)
    d_pad = n_s + js + n_u + ja
    ls = rng.uniform(0.6, 1.4, size=(n_s + js, d_pad))
    ls[:n_s, :n_s + n_u] = spec.lengthscale
    s_out = np.concatenate((spec.outputscale, np.full(js, 0.01)))
    nz = np.concatenate((spec.noise, np.full(js, 1e-5)))
    if ssm.folded_columns is None:
        ssm._ssm.set_hyperparameters(ls, s_out, nz)
    else:
        ssm._ssm.set_hyperparameters(ls[:n_s][:, list(ssm.folded_columns)], s_out[:n_s], nz[:n_s])
    ssm.update_model(T(spec.X), T(spec.Y), replace_old=True)
    _, env = problems.build(spec, device=DEV)
    return ssm, env, spec, (ls, s_out, nz)


class PaddedGP:
    """The oracle's exact GP behind the reference's padding: training rows [z, junk], queries [x, junk, u, junk], outputs
    and Jacobian cut to their leading entries."""

    def __init__(self, spec, js, ja, hyp):
        n = spec.X.shape[0]
        self.n_s, self.n_u, self.js, self.ja = spec.n_s, spec.n_u, js, ja
        self.gp = ExactGP(np.concatenate((spec.X, np.zeros((n, js + ja))), 1),
                          np.concatenate((spec.Y, np.zeros((n, js))), 1), *hyp)

    def predict(self, z, jacobians=True):
        n_s, n_u, js = self.n_s, self.n_u, self.js
        zq = np.zeros((z.shape[0], n_s + js + n_u + self.ja))
        zq[:, :n_s], zq[:, n_s + js:n_s + js + n_u] = z[:, :n_s], z[:, n_s:]
        m, v, j = self.gp.predict(zq, jacobians)
        return m[:, :n_s], v[:, :n_s], (j[:, :n_s, :n_s + n_u] if jacobians else None)


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
        mean, var = mean.contiguous(), var.contiguous()   # (held: a temporary's block could be handed to the next one)
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


# (n_s, n_u, J_s, J_a): the reference's pendulum and cart-pole with junk, both sides of the fold, and both query shifts
SHAPES = [(2, 1, 1, 0), (2, 1, 2, 1), (2, 1, 5, 0), (2, 1, 0, 2), (4, 1, 1, 0), (4, 1, 3, 2), (2, 2, 2, 0)]


@pytest.mark.parametrize('n_s,n_u,js,ja', SHAPES)
def test_fused_junk_rollout_matches_the_step_by_step_rollout(n_s, n_u, js, ja):
    from safe_exploration_amd.cem_mpc import cem_rollout, cem_rollout_stepwise
    ssm, env, spec, _ = junk_case(n_s, n_u, js, ja)
    assert ssm.kernel_family == 'rbf_junk' and ssm.query_shift == min(js, n_u)
    E, P, H = 2, 37, 5
    rng = np.random.default_rng(n_s + 10 * js + 100 * ja)
    x0 = rng.normal(0, 0.05, size=(E, n_s))
    acts = rng.normal(0, 0.3, size=(E, P, H, n_u))
    r = cem_rollout(ssm, env, T(x0), H, actions=T(acts), want_traj=True, want_sigma=True)
    assert int(r['status'].item()) == 0
    S = n_s + n_s * n_s
    for e in range(E):
        p, q, sig, st = stepwise_through_wrapper(ssm, env, T(x0[e]), T(acts[e]))
        assert st == 0
        traj = r['traj'][e].view(P, H, S)
        close(traj[..., :n_s], p)
        close(traj[..., n_s:].reshape(P, H, n_s, n_s), q)
        close(r['sigma'][e], sig)
        ref = cem_rollout_stepwise(ssm, env, T(x0[e]), T(acts[e]), status=torch.zeros(1, dtype=torch.int32, device=DEV))
        close(r['obj_cost'][e], ref['obj_cost'])
        close(r['con_cost'][e], ref['con_cost'], rtol=0, atol=0)


@pytest.mark.parametrize('n_s,n_u,js,ja', [(2, 2, 1, 0), (3, 2, 1, 0)])
def test_fused_junk_rollout_without_a_step_by_step_counterpart_matches_the_oracle(n_s, n_u, js, ja):
    """(2, 2, 1, 0): a query shift short of n_u, whose padded inner model (3, 2) has no sx_gp_predict instantiation;
    (3, 2, 1, 0): sx_onestep_reach has no (3, 2) instantiation -- checked against the oracle's rollout over the padded GP
    instead (to the tolerance of the other oracle comparisons: the device's blocked Cholesky against LAPACK's)."""
    from safe_exploration_amd import problems
    from safe_exploration_amd.cem_mpc import cem_rollout
    ssm, env, spec, hyp = junk_case(n_s, n_u, js, ja)
    assert ssm.kernel_family == 'rbf_junk' and ssm.query_shift == min(js, n_u)
    P, H = 45, 5
    rng = np.random.default_rng(3)
    x0 = rng.normal(0, 0.05, size=n_s)
    acts = rng.normal(0, 0.3, size=(P, H, n_u))
    r = cem_rollout(ssm, env, T(x0[None]), H, actions=T(acts[None]), want_traj=True, want_sigma=True)
    ref = ocem.rollout(problems.oracle_problem(spec, ocem), PaddedGP(spec, js, ja, hyp), x0, acts)
    traj = r['traj'][0].cpu().numpy()
    close(traj[..., :n_s], ref.traj_p, rtol=1e-8, atol=1e-11)
    close(traj[..., n_s:].reshape(P, H, n_s, n_s), ref.traj_q, rtol=1e-8, atol=1e-11)
    close(r['sigma'][0], ref.sigma, rtol=1e-8, atol=1e-11)
    close(r['obj_cost'][0], ref.obj_cost, rtol=1e-8, atol=1e-11)
    close(r['con_cost'][0], ref.con_cost, rtol=0, atol=0)


@pytest.mark.parametrize('n_s,n_u,js,ja', [(2, 1, 2, 1), (4, 1, 1, 0)])
def test_elites_entry_matches_the_plain_entry_given_the_same_refit(n_s, n_u, js, ja):
    from safe_exploration_amd.cem_mpc import cem_rollout
    ssm, env, _, _ = junk_case(n_s, n_u, js, ja)
    E, P, H, k = 2, 50, 5, 6
    rng = np.random.default_rng(11)
    x0 = T(rng.normal(0, 0.05, size=(E, n_s)))
    rows = T(rng.normal(0, 0.3, size=(E, k, 2 + H * n_u)))
    noise = T(rng.normal(size=(E, P, H, n_u)))
    a = cem_rollout(ssm, env, x0, H, elite_rows=rows, noise=noise, want_traj=True, want_dist=True)
    close(a['mean'].view(E, H * n_u), rows[:, :, 2:].mean(1), rtol=1e-12, atol=1e-15)
    b = cem_rollout(ssm, env, x0, H, mean=a['mean'], std=a['std'], noise=noise, want_traj=True)
    close(a['actions'], b['actions'], rtol=1e-14, atol=1e-16)
    for key in ('traj', 'obj_cost', 'con_cost'):
        close(a[key], b[key], rtol=1e-12, atol=1e-14)


def test_output_by_output_form_for_a_large_training_set():
    """A training set whose Kstar buffers of all outputs do not fit in LDS together: the output-by-output kernel."""
    import ctypes

    from safe_exploration_amd import _lib
    from safe_exploration_amd.cem_mpc import cem_rollout, cem_rollout_stepwise
    ssm, env, _, _ = junk_case(2, 1, 1, 0, n_train=700)
    H = 5
    SX_FORM_BYOUT = 3   # include/sx_amd.h
    assert _lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.real_output_view().device_model), H) == SX_FORM_BYOUT
    P = 40
    rng = np.random.default_rng(5)
    x0 = rng.normal(0, 0.05, size=2)
    acts = rng.normal(0, 0.3, size=(P, H, 1))
    r = cem_rollout(ssm, env, T(x0[None]), H, actions=T(acts[None]), want_traj=True, want_sigma=True)
    p, q, sig, _ = stepwise_through_wrapper(ssm, env, T(x0), T(acts))
    close(r['traj'][0][..., :2], p)
    close(r['sigma'][0], sig)
    ref = cem_rollout_stepwise(ssm, env, T(x0), T(acts), status=torch.zeros(1, dtype=torch.int32, device=DEV))
    close(r['obj_cost'][0], ref['obj_cost'])


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


def _solve(ssm, env, spec, H, P, k, iters, seed, monkeypatch):
    from safe_exploration_amd import _lib
    from safe_exploration_amd.cem_mpc import FusedCemMpc
    mpc = FusedCemMpc(ssm, env, H, P, k, iters, device=DEV, init_std=0.2)
    rng = np.random.default_rng(seed)
    noise = rng.normal(size=(iters, P, H, spec.n_u))
    x0 = rng.normal(0, 0.02, size=spec.n_s)
    ssm.real_output_view()          # (built before counting: its fit is not part of the solve's path)
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: counting)
    best, ok, _, status = mpc.solve(T(x0[None]), noise=T(noise[:, None]))
    torch.cuda.synchronize()
    monkeypatch.undo()
    return best, ok, status, counting.calls, noise, x0, mpc


@pytest.mark.parametrize('n_s,js,ja', [(2, 2, 1), (2, 5, 0), (4, 1, 0)])
def test_solve_through_junk_dimensions_is_fused_and_matches_the_oracle(n_s, js, ja, monkeypatch):
    """FusedCemMpc.solve (CemSafeMPC.get_action's solve) over the wrapper: one fused launch per CEM iteration, no
    sx_gp_predict / sx_onestep_reach, and the selected actions equal the oracle's CEM over the reference's padded GP."""
    from safe_exploration_amd import problems
    ssm, env, spec, hyp = junk_case(n_s, 1, js, ja, n_train=80)
    H, P, k, iters = 5, 200, 20, 4
    best, ok, status, calls, noise, x0, _ = _solve(ssm, env, spec, H, P, k, iters, 9 + js, monkeypatch)
    fused = calls['sx_cem_rollout_junk'] + calls['sx_cem_rollout_elites_junk']
    assert fused == iters and calls['sx_cem_rollout_junk'] >= 1
    assert calls['sx_gp_predict'] == 0 and calls['sx_onestep_reach'] == 0
    assert calls['sx_cem_rollout'] == 0 and calls['sx_cem_rollout_elites'] == 0
    ref_best, _ = ocem.cem_solve(problems.oracle_problem(spec, ocem), PaddedGP(spec, js, ja, hyp), x0, noise, k,
                                 init_std=np.full((H, 1), 0.2))
    assert int(status.item()) == 0
    assert (ref_best is not None) == bool(ok[0].item())
    if ref_best is not None:
        close(best[0], ref_best, rtol=0, atol=1e-9)


def test_training_set_beyond_the_single_launch_kernel_solves_step_by_step(monkeypatch):
    """n_pad > 1024: sx_cem_rollout_junk answers SX_ERR_UNSUPPORTED and the solve goes step by step through the
    wrapper, with the same result as an explicitly step-by-step solve."""
    ssm, env, spec, _ = junk_case(2, 1, 2, 1, n_train=1100)
    H, P, k, iters = 4, 64, 8, 2
    best, ok, status, calls, noise, x0, mpc = _solve(ssm, env, spec, H, P, k, iters, 4, monkeypatch)
    assert calls['sx_cem_rollout_junk'] == 1 and calls['sx_cem_rollout_elites_junk'] == 0
    assert calls['sx_gp_predict'] == H * iters and calls['sx_onestep_reach'] == H * iters
    best2, ok2, _, _ = mpc.solve(T(x0[None]), noise=T(noise[:, None]), stepwise=True)
    assert bool(ok[0].item()) == bool(ok2[0].item())
    close(best, best2, rtol=0, atol=0)
