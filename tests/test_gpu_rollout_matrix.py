"""GPU: every fused rollout entry point against the oracle at every shape of the compiled table (`JUNK_FUSED_SHAPES`,
`JUNK_MODEL_FUSED_SHAPES`), under both constraint modes -- the terminal one (SX_CON_TERMINAL, the reference's
`use_state_constraint = False`) and every state (SX_CON_ALL_STATES) -- and both objectives.

Each case is a synthetic problem of its own shape: a random stable prior with LQR feedback, a general polytope of 1,
2 n_s or 16 rows whose last row cuts the particles (oracle/cases.py), and an action box the particles cross in the last
action dimension only.  The model is one of the families the rollouts serve: the exact RBF GP, the 'linear' and 'nn'
feature GPs, MC-dropout ensembles on the matrix-core and the one-particle-per-lane kernels, and the concrete-dropout
ensemble with the log-std head.  The oracle is oracle.cem.rollout over the same model restated in numpy (over the padded
model for the junk-dimension entries).  Every case also asserts that it can tell a wrong kernel from a right one: the
two constraint modes and the two objectives give different costs, some particles leave the polytope and some do not, and
no ellipsoid lies within 1e-9 of a face, so that `con_cost` is compared exactly."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import cases
from oracle import cem as ocem
from oracle import reachability as oreach
from oracle.gp import DropoutEnsemble, ExactGP, FeatureGP, FeatureNet
from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem.ssm_cem import JUNK_FUSED_SHAPES, JUNK_MODEL_FUSED_SHAPES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CON_MODES = {'terminal': _lib.SX_CON_TERMINAL, 'all_states': _lib.SX_CON_ALL_STATES}
OBJ_MODES = (_lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS)


def T(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


# ---- model families ----------------------------------------------------------------------------------------------------
class Conf:
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'
    nn_kernel_layers = [12]
    nn_kernel_seed = 0
    mc_dropout_training_iterations = 10
    mc_dropout_hidden_features = [64, 16]
    mc_dropout_num_samples = 11
    mc_dropout_predict_std = False
    mc_dropout_reinitialize = False
    mc_dropout_type = 'fixed'
    mc_dropout_concrete_initial_probability = 0.1
    mc_dropout_fixed_probability = 0.1
    mc_dropout_on_input = True
    mc_dropout_lengthscale = 1e-4
    mc_dropout_seed = 3
    device = DEV


# 'nn1' / 'nn3': the 'nn' kernel with one layer and with three up to SX_FEAT_MAX_WIDTH; 'mlp': two hidden layers, one of
# them 64 wide (the matrix-core kernel); 'mlp_lane': three hidden layers, with SX_MLP_PATH=valu (the one-particle-per-lane
# kernel); 'gal': GalConcreteDropoutSSM, concrete dropout with the log-std head
FAMILIES = {'rbf': dict(),
            'linear': dict(exact_gp_kernel='linear'),
            'nn1': dict(exact_gp_kernel='nn', nn_kernel_layers=[12]),
            'nn3': dict(exact_gp_kernel='nn', nn_kernel_layers=[8, 16, _lib.SX_FEAT_MAX_WIDTH]),
            'mlp': dict(),
            'mlp_lane': dict(mc_dropout_hidden_features=[16, 24, 8], mc_dropout_num_samples=9),
            'gal': dict(mc_dropout_type='concrete', mc_dropout_predict_std=True, mc_dropout_hidden_features=[24, 12],
                        mc_dropout_num_samples=6)}
FEATURE, MLP = ('linear', 'nn1', 'nn3'), ('mlp', 'mlp_lane', 'gal')
# (rtol of the centres, rtol of shapes / variances / objective, atol): those of the neighbouring oracle comparisons
TOL = {'rbf': (1e-8, 1e-7, 1e-11), 'feature': (1e-7, 1e-6, 1e-10), 'mlp': (1e-8, 1e-7, 1e-11)}


def group(family):
    return 'rbf' if family == 'rbf' else 'feature' if family in FEATURE else 'mlp'


@pytest.fixture
def lane_path(monkeypatch):
    """The library reads SX_MLP_PATH at every launch: set it for 'mlp_lane' (monkeypatch restores it)."""
    def select(family):
        if family == 'mlp_lane':
            monkeypatch.setenv('SX_MLP_PATH', 'valu')
        else:
            monkeypatch.delenv('SX_MLP_PATH', raising=False)
    return select


def conf(family, e=0):
    return type('C', (Conf,), dict(FAMILIES[family], nn_kernel_seed=10 + e, mc_dropout_seed=3 + 7 * e))()


def constructor(family, e=0):
    from safe_exploration_amd.ssm_cem.dropout_ssm_cem import McDropoutSSM
    from safe_exploration_amd.ssm_cem.gal_concrete_dropout import GalConcreteDropoutSSM
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    cls = GpCemSSM if group(family) != 'mlp' else GalConcreteDropoutSSM if family == 'gal' else McDropoutSSM
    return functools.partial(cls, conf(family, e))


def feature_net(ssm):
    """The oracle's FeatureNet of a FeatureGpCemSSM: its network's layers and PReLU slope (none for 'linear')."""
    from torch import nn
    if ssm._net is None:
        return FeatureNet()
    layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in ssm._net if isinstance(m, nn.Linear)]
    return FeatureNet(layers, prelu=float(ssm._net[-1].weight.detach().reshape(-1)[0]))


def ensemble_oracle(ssm, n_s):
    """DropoutEnsemble of an McDropoutSSM over its first n_s outputs (and, with the log-std head, their log-stds)."""
    layers, masks = ssm.ensemble()
    n_out = ssm.num_states
    rows = list(range(n_s)) + (list(range(n_out, n_out + n_s)) if ssm._predict_std else [])
    W, b = layers[-1]
    return DropoutEnsemble(layers[:-1] + [(W[rows], b[rows])], masks, n_s, predict_std=bool(ssm._predict_std))


class Padded:
    """An oracle model over the reference's padded inputs seen through JunkDimensionsSSM: queries [x, junk, u, junk], the
    outputs and the Jacobian cut to their leading n_s and n_s + n_u entries."""

    def __init__(self, model, n_s, n_u, js, ja):
        self.model, self.n_s, self.n_u, self.js, self.ja = model, n_s, n_u, js, ja

    def predict(self, z, jacobians=True):
        n_s, n_u, js = self.n_s, self.n_u, self.js
        zq = np.zeros((z.shape[0], n_s + js + n_u + self.ja))
        zq[:, :n_s], zq[:, n_s + js:n_s + js + n_u] = z[:, :n_s], z[:, n_s:]
        m, v, j = self.model.predict(zq, jacobians)
        return m[:, :n_s], v[:, :n_s], (j[:, :n_s, :n_s + n_u] if jacobians else None)


def training_set(n_s, n_u, N, seed):
    from safe_exploration_amd import problems
    return problems.synthetic_training_set(N, n_s, n_u, seed=seed, scale=0.6, amp=0.05, noise_std=0.002)


def build_model(family, n_s, n_u, N=60, seed=0, e=0):
    """(ssm with data on the GPU, its oracle) for a plain (shift-0) model."""
    X, Y = training_set(n_s, n_u, N, 31 * seed + 7 * e + n_s + 3 * n_u)
    rng = np.random.default_rng(500 + 10 * n_s + n_u + 97 * e)
    ssm = constructor(family, e)(state_dimen=n_s, action_dimen=n_u)
    if family == 'rbf':
        ls, s, nz = rng.uniform(0.6, 1.4, size=(n_s, n_s + n_u)), rng.uniform(1e-4, 3e-4, size=n_s), rng.uniform(1e-6, 5e-6, size=n_s)
        ssm.set_hyperparameters(ls, s, nz)
        oracle = ExactGP(X, Y, ls, s, nz)
    elif group(family) == 'feature':
        c, nz = rng.uniform(0.01, 0.03, size=n_s), rng.uniform(1e-4, 3e-4, size=n_s)
        ssm.set_hyperparameters(kernel_scale=c, noise=nz)
        oracle = FeatureGP(X, Y, feature_net(ssm), c, nz)
    ssm.update_model(T(X), T(Y), replace_old=True)
    if group(family) == 'mlp':
        oracle = ensemble_oracle(ssm, n_s)
    assert ssm.kernel_family == group(family)
    return ssm, oracle


def junk_sizes(n_s, n_u, shift):
    """(J_s, J_a) of a JunkDimensionsSSM with this query shift: a junk action where n_u = 1, one junk state more than the
    shift for the pendulum's shape (a padded (4, 2) model)."""
    return shift + (1 if (n_s, n_u) == (2, 1) else 0), (1 if n_u == 1 else 0)


def build_junk_model(family, n_s, n_u, shift, N=60):
    """(JunkDimensionsSSM over the family's model with data, the oracle over the padded model)."""
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    js, ja = junk_sizes(n_s, n_u, shift)
    X, Y = training_set(n_s, n_u, N, 11 * n_s + n_u + shift)
    rng = np.random.default_rng(700 + 10 * n_s + n_u + 100 * shift)
    ssm = JunkDimensionsSSM(constructor(family), state_dimen=n_s, action_dimen=n_u, junk_states=js, junk_actions=ja)
    assert ssm.query_shift == shift
    d_pad = n_s + js + n_u + ja
    X_pad = np.concatenate((X, np.zeros((N, js + ja))), 1)
    Y_pad = np.concatenate((Y, np.zeros((N, js))), 1)
    if family == 'rbf':
        ls = rng.uniform(0.6, 1.4, size=(n_s + js, d_pad))
        s = np.concatenate((rng.uniform(1e-4, 3e-4, size=n_s), np.full(js, 1e-4)))
        nz = np.concatenate((rng.uniform(1e-6, 5e-6, size=n_s), np.full(js, 1e-6)))
        if ssm.folded_columns is None:
            ssm._ssm.set_hyperparameters(ls, s, nz)
        else:
            ssm._ssm.set_hyperparameters(ls[:n_s][:, list(ssm.folded_columns)], s[:n_s], nz[:n_s])
        oracle = ExactGP(X_pad, Y_pad, ls, s, nz)
    elif group(family) == 'feature':
        c, nz = rng.uniform(0.01, 0.03, size=n_s + js), rng.uniform(1e-4, 3e-4, size=n_s + js)
        ssm._ssm.set_hyperparameters(kernel_scale=c, noise=nz)
        oracle = FeatureGP(X_pad, Y_pad, feature_net(ssm._ssm), c, nz)
    ssm.update_model(T(X), T(Y), replace_old=True)
    if group(family) == 'mlp':
        oracle = ensemble_oracle(ssm._ssm, n_s)
    assert ssm.kernel_family == {'rbf': 'rbf_junk', 'feature': 'feature_junk', 'mlp': 'mlp_junk'}[group(family)]
    return ssm, Padded(oracle, n_s, n_u, js, ja)


_MODELS = {}


def cached(builder, *key):
    """One model per (builder, arguments) for the module: the tests of both constraint modes share it."""
    if (builder, key) not in _MODELS:
        _MODELS[(builder, key)] = builder(*key)
    return _MODELS[(builder, key)]


# ---- the problem: prior, feedback, objective, polytope, action box -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(n_s, n_u):
    from safe_exploration_amd.utils import dlqr
    rng = np.random.default_rng(1000 + 10 * n_s + n_u)
    a = 0.85 * np.eye(n_s) + 0.05 * rng.normal(size=(n_s, n_s))
    b = 0.5 * rng.normal(size=(n_s, n_u))
    k_fb = -dlqr(a, b, np.eye(n_s), 5.0 * np.eye(n_u))[0]
    return dict(n_s=n_s, n_u=n_u, a=a, b=b, k_fb=k_fb, l_mu=rng.uniform(0.005, 0.02, size=n_s),
                l_sigma=rng.uniform(0.005, 0.02, size=n_s), beta=2.0, w_abs=rng.uniform(0.2, 1.0, size=n_s),
                target=rng.normal(0, 0.1, size=n_s), w_lin=rng.normal(0, 0.2, size=n_s))


class Constraints:
    """The polytope and the action box of one launch, with the oracle's problem and the sx_env per mode."""

    def __init__(self, sysd, h_mat, h_vec, u_min, u_max):
        self.sysd, self.h_mat, self.h_vec, self.u_min, self.u_max = sysd, h_mat, h_vec, u_min, u_max

    def problem(self, obj_mode, con_mode):
        s = self.sysd
        return ocem.Problem(s['n_s'], s['n_u'], s['a'], s['b'], s['k_fb'], s['l_mu'], s['l_sigma'], s['beta'], self.h_mat,
                            self.h_vec, self.u_min, self.u_max, obj_mode=obj_mode, obj_w_abs=s['w_abs'],
                            obj_target=s['target'], obj_w_lin=s['w_lin'], con_mode=con_mode)

    def env(self, obj_mode, con_mode):
        from safe_exploration_amd.gp_reachability_pytorch import make_env
        s = self.sysd
        return make_env(s['n_s'], s['n_u'], a=s['a'], b=s['b'], k_fb=s['k_fb'], l_mu=s['l_mu'], l_sigma=s['l_sigma'],
                        beta=s['beta'], h_mat=self.h_mat, h_vec=self.h_vec, u_min=self.u_min, u_max=self.u_max,
                        obj_mode=obj_mode, obj_w_abs=s['w_abs'], obj_target=s['target'], obj_w_lin=s['w_lin'],
                        con_mode=con_mode)


def constraints_for(sysd, oracles, x0, actions, q0=None, m=_lib.SX_MAX_M, seed=0):
    """A polytope of m rows chosen from the oracle's trajectories of these particles (E problems: oracles[e], x0 [E x n_s],
    actions [E x P x H x n_u], q0 None or [E x n_s x n_s]) and an action box crossed in the last action dimension only."""
    n_s, n_u = sysd['n_s'], sysd['n_u']
    box = Constraints(sysd, np.vstack((np.eye(n_s), -np.eye(n_s))), np.full((2 * n_s, 1), 1e3), np.full(n_u, -1e3),
                      np.full(n_u, 1e3))
    refs = [ocem.rollout(box.problem(0, 1), oracles[e], x0[e], actions[e], None if q0 is None else q0[e])
            for e in range(len(oracles))]
    traj_p = np.concatenate([r.traj_p for r in refs])
    traj_q = np.concatenate([r.traj_q for r in refs])
    start_q = np.zeros((len(x0), n_s, n_s)) if q0 is None else q0
    h_mat, h_vec = cases.active_polytope(np.random.default_rng(seed), traj_p, traj_q, x0, start_q, m=m)
    u = np.abs(actions[..., -1]).ravel()
    bound = np.full(n_u, np.abs(actions).max() + 1.0)
    bound[-1] = np.quantile(u, 0.8) if u.size > 1 else 2.0 * u[0]
    return Constraints(sysd, h_mat, h_vec, -bound, bound.copy())


# ---- the checks ----------------------------------------------------------------------------------------------------------
def close(a, b, rtol, atol, what):
    np.testing.assert_allclose(a.cpu().numpy() if torch.is_tensor(a) else a, b, rtol=rtol, atol=atol, err_msg=what)


def check_problem(r, e, ref, tol, what):
    """Problem e of a launch against the oracle: centres, shapes, variances, objective; constraint cost exactly."""
    n_s = ref.traj_p.shape[-1]
    P, H = ref.traj_p.shape[:2]
    traj = r['traj'][e].cpu().numpy()
    rtol_p, rtol, atol = tol
    close(traj[..., :n_s], ref.traj_p, rtol_p, atol, what + ': centres')
    close(traj[..., n_s:].reshape(P, H, n_s, n_s), ref.traj_q, rtol, atol, what + ': shapes')
    close(r['sigma'][e], ref.sigma, rtol, atol, what + ': sigma')
    close(r['obj_cost'][e], ref.obj_cost, rtol, atol, what + ': obj_cost')
    np.testing.assert_array_equal(r['con_cost'][e].cpu().numpy(), ref.con_cost, err_msg=what + ': con_cost')


def oracle_runs(con, oracle, x0, actions, q0=None):
    """oracle.cem.rollout of one problem under every (objective, constraint) mode: {(obj, con): RolloutResult}."""
    return {(o, c): ocem.rollout(con.problem(o, c), oracle, x0, actions, q0) for o in OBJ_MODES for c in CON_MODES.values()}


def assert_non_vacuous(con, runs, what):
    """The case tells a wrong kernel from a right one (runs: the oracle_runs of the problems of one launch): no ellipsoid
    within 1e-9 of a face (so that con_cost is compared exactly) and the objectives differ; with more than one particle
    also some particles leave the polytope and some do not, every cutting row is the only row some particle crosses (for
    n_s > 1), and
    (H > 1) the two constraint modes give some particle different costs."""
    T_, A_ = _lib.SX_CON_TERMINAL, _lib.SX_CON_ALL_STATES
    o = OBJ_MODES[0]
    for r in runs:
        ref = r[(o, A_)]
        assert cases.min_abs_distance(ref.traj_p, ref.traj_q, con.h_mat, con.h_vec) > 1e-9, what + ': a face is touched'
    assert any(not np.allclose(r[(OBJ_MODES[0], A_)].obj_cost, r[(OBJ_MODES[1], A_)].obj_cost) for r in runs), \
        what + ': objectives agree'
    crossed = np.concatenate([cases.crossings(r[(o, A_)].traj_p, r[(o, A_)].traj_q, con.h_mat, con.h_vec) for r in runs])
    if len(crossed) == 1:     # (one particle: it cannot both leave and stay)
        return
    outside = crossed.any(1)
    assert outside.any() and not outside.all(), what + f': {int(outside.sum())} of {outside.size} particles leave the polytope'
    # (in one dimension the rows are parallel: two rows that cut on the same side nest, so no particle need cross one alone)
    for row in cases.cutting_rows(len(con.h_vec)) if con.h_mat.shape[1] > 1 else ():
        assert (crossed[:, row] & (crossed.sum(1) == 1)).any(), what + f': no particle crosses row {row} alone'
    if runs[0][(o, A_)].traj_p.shape[1] > 1:     # (one step: the terminal state is every state)
        assert any((r[(o, T_)].con_cost != r[(o, A_)].con_cost).any() for r in runs), what + ': modes agree everywhere'


def assert_status(r, runs_by_problem, words):
    """The device's status word(s) against the OR of the oracle's (one word per launch, or per problem)."""
    want = [ref.status for ref in runs_by_problem]
    got = [int(v) for v in r['status'].cpu().numpy().reshape(-1)]
    assert got == ([int(np.bitwise_or.reduce(want))] if words == 1 else want), (got, want)


def given_actions(ssm, oracles, sysd, con_name, x0, acts, tol, what, seed, m, launch=None):
    """Launch the rollout of given actions under the constraint mode `con_name` and both objectives; every problem against
    the oracle; the case's non-vacuity."""
    from safe_exploration_amd.cem_mpc import cem_rollout
    launch = launch or (lambda env, **kw: cem_rollout(ssm, env, T(x0), acts.shape[2], actions=T(acts), want_traj=True,
                                                       want_sigma=True, **kw))
    con = constraints_for(sysd, oracles, x0, acts, m=m, seed=seed)
    runs = [oracle_runs(con, oracles[e], x0[e], acts[e]) for e in range(len(oracles))]
    assert_non_vacuous(con, runs, what)
    c = CON_MODES[con_name]
    for o in OBJ_MODES:
        r = launch(con.env(o, c))
        for e in range(len(oracles)):
            check_problem(r, e, runs[e][(o, c)], tol, f'{what} obj {o} problem {e}')
        assert_status(r, [runs[e][(o, c)] for e in range(len(oracles))], r['status'].numel())


def shapes(table, shift0):
    return sorted((n_s, n_u) if shift0 else (n_s, n_u, s) for n_s, n_u, s in table if (s == 0) == shift0)


PLAIN = [('rbf',) + s for s in shapes(JUNK_FUSED_SHAPES, True)] + \
        [(f,) + s for f in FEATURE + MLP for s in shapes(JUNK_MODEL_FUSED_SHAPES, True)]
JUNK = [('rbf',) + s for s in shapes(JUNK_FUSED_SHAPES, False)] + \
       [(f,) + s for f in FEATURE + MLP for s in shapes(JUNK_MODEL_FUSED_SHAPES, False)]


@pytest.mark.parametrize('con_name', list(CON_MODES))
@pytest.mark.parametrize('family,n_s,n_u', PLAIN)
def test_plain_entry_given_actions_vs_oracle(family, n_s, n_u, con_name, lane_path):
    """sx_cem_rollout / _feat / _mlp, one problem: P = 1, 17, 65 (around the 16-particle tile and the 64-lane wave), H = 1
    and 4, both objectives, against the oracle."""
    lane_path(family)
    ssm, oracle = cached(build_model, family, n_s, n_u)
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(10 * n_s + n_u)
    M = _lib.SX_MAX_M
    for i, (P, H, m) in enumerate([(1, 1, M), (17, 1, 1), (65, 1, 2 * n_s), (1, 4, 2 * n_s), (17, 4, M), (65, 4, 1)]):
        x0 = rng.normal(0, 0.02, size=(1, n_s))
        acts = rng.normal(0, 0.4, size=(1, P, H, n_u))
        given_actions(ssm, [oracle], sysd, con_name, x0, acts, TOL[group(family)], f'{family} P={P} H={H} m={m}', i, m)


@pytest.mark.parametrize('con_name', list(CON_MODES))
@pytest.mark.parametrize('family,n_s,n_u', PLAIN)
def test_plain_entry_sampled_actions_vs_oracle(family, n_s, n_u, con_name, lane_path):
    """E = 2 problems with a start ellipsoid each (step 0 takes the ellipsoid branch), actions sampled in the kernel from
    mean + std noise: the actions, then every problem against the oracle."""
    from safe_exploration_amd.cem_mpc import cem_rollout
    lane_path(family)
    ssm, oracle = cached(build_model, family, n_s, n_u)
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(20 + 10 * n_s + n_u)
    E = 2
    for i, (P, H, m) in enumerate([(17, 1, _lib.SX_MAX_M), (65, 4, 1)]):
        x0 = rng.normal(0, 0.02, size=(E, n_s))
        q0 = np.stack([np.eye(n_s) * 1e-4 * (e + 1) for e in range(E)])
        mean, std = rng.normal(0, 0.1, size=(E, H, n_u)), rng.uniform(0.2, 0.4, size=(E, H, n_u))
        noise = rng.normal(size=(E, P, H, n_u))
        host = mean[:, None] + std[:, None] * noise
        con = constraints_for(sysd, [oracle] * E, x0, host, q0=q0, m=m, seed=i)
        c = CON_MODES[con_name]
        for o in OBJ_MODES:
            r = cem_rollout(ssm, con.env(o, c), T(x0), H, mean=T(mean), std=T(std), noise=T(noise), q0=T(q0),
                            want_traj=True, want_sigma=True)
            acts = r['actions'].cpu().numpy()
            np.testing.assert_allclose(acts, host, rtol=1e-15, atol=1e-16)
            runs = [oracle_runs(con, oracle, x0[e], acts[e], q0[e]) for e in range(E)]
            assert_non_vacuous(con, runs, f'{family} sampled P={P} H={H}')
            for e in range(E):
                check_problem(r, e, runs[e][(o, c)], TOL[group(family)], f'{family} sampled P={P} H={H} obj {o} problem {e}')
            assert_status(r, [runs[e][(o, c)] for e in range(E)], 1)


def elites_vs_oracle(ssm, oracle, n_s, n_u, c, seed, what):
    """The elite-row entry (sx_cem_rollout_elites[_junk]) under constraint mode c: the refit equals ocem.refit, the launch
    equals the plain entry given that refit bit for bit, and every problem matches the oracle."""
    from safe_exploration_amd.cem_mpc import cem_rollout
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(seed)
    E, P, H, k = 2, 65, 4, 9
    x0 = rng.normal(0, 0.02, size=(E, n_s))
    rows = np.concatenate([np.zeros((E, k, 2)), rng.normal(0.0, 0.3, size=(E, k, H * n_u))], axis=2)
    noise = rng.normal(size=(E, P, H, n_u))
    fits = [ocem.refit(rows[e, :, 2:].reshape(k, H, n_u)) for e in range(E)]
    host = np.stack([fits[e][0][None] + fits[e][1][None] * noise[e] for e in range(E)])
    con = constraints_for(sysd, [oracle] * E, x0, host, seed=3)
    o = _lib.SX_OBJ_AFFINE_ABS
    env = con.env(o, c)
    r1 = cem_rollout(ssm, env, T(x0), H, elite_rows=T(rows), noise=T(noise), want_dist=True, want_traj=True, want_sigma=True)
    for e in range(E):
        close(r1['mean'][e], fits[e][0], 1e-12, 1e-15, what + ': mean')
        close(r1['std'][e], fits[e][1], 1e-12, 1e-15, what + ': std')
    r2 = cem_rollout(ssm, env, T(x0), H, mean=r1['mean'], std=r1['std'], noise=T(noise), want_traj=True, want_sigma=True)
    for key in ('actions', 'obj_cost', 'con_cost', 'traj', 'sigma'):
        torch.testing.assert_close(r1[key], r2[key], rtol=0, atol=0, msg=f'{what}: {key}')
    acts = r1['actions'].cpu().numpy()
    runs = [oracle_runs(con, oracle, x0[e], acts[e]) for e in range(E)]
    assert_non_vacuous(con, runs, what)
    for e in range(E):
        check_problem(r1, e, runs[e][(o, c)], TOL['rbf'], f'{what} problem {e}')
    assert_status(r1, [runs[e][(o, c)] for e in range(E)], 1)


@pytest.mark.parametrize('n_s,n_u', shapes(JUNK_FUSED_SHAPES, True))
def test_elites_entry_with_the_terminal_constraint(n_s, n_u):
    """sx_cem_rollout_elites under SX_CON_TERMINAL (elites_vs_oracle)."""
    ssm, oracle = cached(build_model, 'rbf', n_s, n_u)
    elites_vs_oracle(ssm, oracle, n_s, n_u, _lib.SX_CON_TERMINAL, 30 + 10 * n_s + n_u, 'elites')


@pytest.mark.parametrize('con_name', list(CON_MODES))
@pytest.mark.parametrize('n_s,n_u,shift', shapes(JUNK_FUSED_SHAPES, False))
def test_elites_junk_entry_vs_the_padded_oracle(n_s, n_u, shift, con_name):
    """sx_cem_rollout_elites_junk at every query shift > 0 of JUNK_FUSED_SHAPES (elites_vs_oracle against
    sx_cem_rollout_junk and the oracle over the padded exact GP)."""
    ssm, oracle = cached(build_junk_model, 'rbf', n_s, n_u, shift)
    elites_vs_oracle(ssm, oracle, n_s, n_u, CON_MODES[con_name], 35 + 10 * n_s + n_u + 100 * shift, 'elites junk')


@pytest.mark.parametrize('family,n_s,n_u', PLAIN)
def test_multi_model_entries_vs_oracle(family, n_s, n_u, lane_path):
    """sx_cem_rollout_multi (+ _elites_multi for the exact GP), _feat_multi, _mlp_multi: E = 3 problems with a model of the
    family each, SX_CON_TERMINAL and the affine objective; every problem against the oracle over its own model."""
    from safe_exploration_amd.cem_mpc import cem_rollout_multi
    lane_path(family)
    E, P, H = 3, 65, 4
    built = [cached(build_model, family, n_s, n_u, 50 + 10 * e, 1, e) for e in range(E)]
    ssms, oracles = [b[0] for b in built], [b[1] for b in built]
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(40 + 10 * n_s + n_u)
    x0 = rng.normal(0, 0.02, size=(E, n_s))
    acts = rng.normal(0, 0.4, size=(E, P, H, n_u))
    c, o = _lib.SX_CON_TERMINAL, _lib.SX_OBJ_AFFINE_ABS
    con = constraints_for(sysd, oracles, x0, acts, seed=4)
    runs = [oracle_runs(con, oracles[e], x0[e], acts[e]) for e in range(E)]
    assert_non_vacuous(con, runs, f'{family} multi')
    r = cem_rollout_multi(ssms, con.env(o, c), T(x0), H, actions=T(acts), want_traj=True, want_sigma=True)
    for e in range(E):
        check_problem(r, e, runs[e][(o, c)], TOL[group(family)], f'{family} multi problem {e}')
    assert_status(r, [runs[e][(o, c)] for e in range(E)], E)
    if family != 'rbf':
        return
    k = 7
    rows = np.concatenate([np.zeros((E, k, 2)), rng.normal(0.0, 0.3, size=(E, k, H * n_u))], axis=2)
    noise = rng.normal(size=(E, P, H, n_u))
    fits = [ocem.refit(rows[e, :, 2:].reshape(k, H, n_u)) for e in range(E)]
    host = np.stack([fits[e][0][None] + fits[e][1][None] * noise[e] for e in range(E)])
    con = constraints_for(sysd, oracles, x0, host, seed=5)
    r = cem_rollout_multi(ssms, con.env(o, c), T(x0), H, elite_rows=T(rows), noise=T(noise), want_dist=True,
                          want_traj=True, want_sigma=True)
    acts = r['actions'].cpu().numpy()
    runs = [oracle_runs(con, oracles[e], x0[e], acts[e]) for e in range(E)]
    assert_non_vacuous(con, runs, 'elites multi')
    for e in range(E):
        close(r['mean'][e], fits[e][0], 1e-12, 1e-15, 'mean')
        close(r['std'][e], fits[e][1], 1e-12, 1e-15, 'std')
        check_problem(r, e, runs[e][(o, c)], TOL['rbf'], f'elites multi problem {e}')
    assert_status(r, [runs[e][(o, c)] for e in range(E)], E)


@pytest.mark.parametrize('con_name', list(CON_MODES))
@pytest.mark.parametrize('family,n_s,n_u,shift', JUNK)
def test_junk_entries_vs_the_padded_oracle(family, n_s, n_u, shift, con_name, lane_path):
    """sx_cem_rollout_junk / _feat_junk / _mlp_junk at every query shift > 0 of the tables: E = 2 problems against the
    oracle over the reference's padded model."""
    lane_path(family)
    ssm, oracle = cached(build_junk_model, family, n_s, n_u, shift)
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(50 + 10 * n_s + n_u + 100 * shift)
    for i, (P, H, m) in enumerate([(17, 1, 2 * n_s), (65, 4, _lib.SX_MAX_M)]):
        x0 = rng.normal(0, 0.02, size=(2, n_s))
        acts = rng.normal(0, 0.4, size=(2, P, H, n_u))
        given_actions(ssm, [oracle] * 2, sysd, con_name, x0, acts, TOL[group(family)], f'{family} junk P={P} H={H} m={m}',
                      i, m)


# (n_s, n_u, training-set size, form): SX_FORM_BYOUT needs n_s > 1
LARGE = [(1, 1, 1100, 'big'), (3, 1, 500, 'byout'), (3, 1, 1100, 'big'), (2, 2, 700, 'byout'), (2, 2, 1100, 'big'),
         (4, 2, 400, 'byout'), (4, 2, 1100, 'big')]
FORMS = {'byout': 3, 'big': 4}    # SX_FORM_BYOUT, SX_FORM_BIG (include/sx_amd.h)


@pytest.mark.parametrize('n_s,n_u,N,form', LARGE)
def test_large_training_set_forms_with_the_terminal_constraint(n_s, n_u, N, form):
    """The exact GP's output-by-output kernel and three-launch path, SX_CON_TERMINAL, E = 2 problems against the oracle."""
    ssm, oracle = cached(build_model, 'rbf', n_s, n_u, N, 2)
    assert _lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), 4) == FORMS[form]
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(60 + 10 * n_s + n_u)
    x0 = rng.normal(0, 0.02, size=(2, n_s))
    acts = rng.normal(0, 0.4, size=(2, 65, 4, n_u))
    given_actions(ssm, [oracle] * 2, sysd, 'terminal', x0, acts, TOL['rbf'], f'{form} N={N}', 6, _lib.SX_MAX_M)


# ---- the solver with the terminal constraint ------------------------------------------------------------------------------
class SolverConf:
    mpc_time_horizon = 5
    cem_num_rollouts = 200
    cem_num_elites = 20
    cem_num_iterations = 4
    cem_init_std = 0.4
    plot_cem_optimisation = False
    plot_cem_terminal_states = False
    device = DEV
    use_state_constraint = False
    use_prior_model = True


class SolverEnv:
    """The environment attributes CemSafeMPC reads (the affine pendulum objective of environments.py:505-510)."""

    def __init__(self, spec):
        self.spec, self.n_s, self.n_u = spec, spec.n_s, spec.n_u
        self.l_mu, self.l_sigm = spec.l_mu, spec.l_sigma
        self.u_min_norm, self.u_max_norm = spec.u_min, spec.u_max
        self._current_objective = -0.1

    def random_action(self):
        return np.zeros(self.n_u)

    def objective_cost_function(self, ps):
        return torch.abs(torch.full_like(ps[:, 1], self._current_objective) - ps[:, 1])

    def get_safety_constraints(self, normalize=True):
        return self.spec.h_mat, self.spec.h_vec, None, None


def solver_spec():
    """The pendulum with the affine objective and the terminal constraint."""
    from safe_exploration_amd import problems
    spec = problems.pendulum(n_train=120, seed=3, obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    spec.con_mode = _lib.SX_CON_TERMINAL
    return spec


@pytest.mark.parametrize('family', ['rbf', 'mlp'])
def test_get_action_with_the_terminal_constraint_matches_the_oracle(family, lane_path):
    """CemSafeMPC.get_action with use_state_constraint = False (the terminal constraint through construct_constraints and
    the sx_env's con_mode) against ocem.cem_solve with CON_TERMINAL and the same noise; the same solve step by step.  The
    polytope is the smallest of a range of scalings of the pendulum's box under which the oracle's terminal-constrained
    solve finds a solution and picks other elites than the every-state solve (chosen over the trained model, which the
    polytope does not change)."""
    from safe_exploration_amd import problems
    from safe_exploration_amd.safempc_cem import CemSafeMPC, MpcResult, construct_constraints
    lane_path(family)
    spec = solver_spec()
    c = SolverConf
    ssm = constructor(family)(state_dimen=2, action_dimen=1)
    if family == 'rbf':
        ssm.set_hyperparameters(spec.lengthscale, spec.outputscale, spec.noise)

    def make_solver():
        env = SolverEnv(spec)
        return CemSafeMPC(ssm, construct_constraints(c(), env), env, c(), {'lin_model': (spec.a, spec.b)},
                          wx_feedback_cost=np.diag([1.0, 2.0]), wu_feedback_cost=25.0 * np.eye(1), beta_safety=spec.beta,
                          safe_policy=lambda x: spec.k_fb @ x)
    y = spec.Y + spec.X[:, :2] @ spec.a.T + spec.X[:, 2:] @ spec.b.T
    make_solver().update_model(spec.X, y, opt_hyp=False, replace_old=True)      # (trains the model once)
    model = ExactGP(spec.X, ssm.y_train.cpu().numpy(), spec.lengthscale, spec.outputscale, spec.noise) \
        if family == 'rbf' else ensemble_oracle(ssm, 2)
    rng = np.random.default_rng(13)
    noise = rng.normal(size=(c.cem_num_iterations, c.cem_num_rollouts, c.mpc_time_horizon, 1))
    x0 = np.array([0.01, -0.02])
    init_std = np.full((c.mpc_time_horizon, 1), c.cem_init_std)
    tried = []
    for scale in np.geomspace(0.5, 16.0, 31):     # (the pendulum's box, |d_theta| <= 0.8 and |theta| <= 0.35, scaled)
        spec.h_vec = scale * np.array([[0.8], [0.8], [0.35], [0.35]])
        prob = problems.oracle_problem(spec, ocem)
        ref_best, trace = ocem.cem_solve(prob, model, x0, noise, c.cem_num_elites, init_std=init_std)
        prob.con_mode = _lib.SX_CON_ALL_STATES
        _, trace_all = ocem.cem_solve(prob, model, x0, noise, c.cem_num_elites, init_std=init_std)
        # (the modes pick different elites: a solve that ignored the mode would not match)
        differs = any(not np.array_equal(a, b) for a, b in zip(trace.elites, trace_all.elites))
        tried.append((round(float(scale), 3), ref_best is not None, differs))
        if ref_best is not None and differs:
            break
    else:
        pytest.fail(f'no scale of the polytope separates the constraint modes with a solution: {tried}')
    solver = make_solver()
    mpc = solver._solver()
    it = iter(noise)
    mpc.sample_noise = lambda episodes=1: T(next(it)[None])
    action, result = solver.get_action(x0)
    assert result == MpcResult.FOUND_SOLUTION
    np.testing.assert_allclose(solver._last_mpc_actions, ref_best, rtol=0, atol=1e-9)
    np.testing.assert_allclose(action, ref_best[0], rtol=0, atol=1e-9)
    best, ok, _, status = mpc.solve(T(x0[None]), noise=T(noise[:, None]), stepwise=True)
    fused, ok_f, _, _ = mpc.solve(T(x0[None]), noise=T(noise[:, None]))
    assert int(status.item()) == 0 and bool(ok[0]) and bool(ok_f[0])
    np.testing.assert_allclose(best.cpu().numpy(), fused.cpu().numpy(), rtol=0, atol=1e-9)


# ---- the forced forms at the edges of their step loops ----------------------------------------------------------------------
@pytest.mark.parametrize('form', ['rh', 'rw', 'stream'])
def test_forced_forms_at_short_horizons_with_both_constraint_modes(form):
    """The 8-wave, 4-wave and streaming forms (SX_ROLLOUT, read once per process: tools/rw_repro.py runs a child per
    shape) on every (n_s, n_u) each is instantiated for, with H = 1, 2 and 5 -- where the step loops' last-step epilogues
    (finish, finish_polytope, finish_costs) take over --, both constraint modes and a general polytope of SX_MAX_M rows."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shapes = {'rh': ['2,1,77', '1,1,77', '2,2,77'],
              'rw': ['2,1,77', '1,1,77', '3,1,77', '4,1,50', '4,2,40', '2,2,120'],
              'stream': ['2,1,77', '1,1,77', '3,1,77', '4,1,77', '4,2,60', '2,2,77']}[form]
    env = dict(os.environ, SX_ROLLOUT=form, SX_ROLLOUT_STRICT='1')
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'rw_repro.py'), '--horizons=1,2,5', '--con-modes=0,1',
                        f'--rows={_lib.SX_MAX_M}'] + shapes, capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0 and 'Memory access fault' not in r.stdout + r.stderr, r.stdout[-3000:] + r.stderr[-2000:]
    want = {'rh': 'form 2', 'rw': 'form 1', 'stream': 'form 0'}[form]
    assert r.stdout.count('matches the oracle; ' + want) == len(shapes) * 3 * 2, r.stdout[-3000:]
