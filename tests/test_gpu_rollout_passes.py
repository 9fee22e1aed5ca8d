"""GPU: the persistent-grid rollout kernels and the GP predict kernel past the first pass of their grids.

The default exact-GP rollouts, cem_rollout_rh_kernel (8 waves, n_s <= 2) and cem_rollout_rw_kernel (4 waves, n_s = 3, 4 and
n_s = n_u = 2 beyond n_pad = 128), launch min(E ceil(P / 16), compute units) workgroups, each looping over the tiles
`tile = blockIdx.x; tile += gridDim.x` (csrc/sx_rw_impl.hpp, resident_grid).  The batches of tests/test_gpu_rollout_matrix.py
never reach a second trip of that loop.  Here E = 2 problems of P = 16 CU + 37 particles make 2 CU + 6 tiles: every
workgroup runs two tiles and some run three, and problem 1's first tile and both ragged last tiles fall on later trips,
where the kernel re-derives (e, c0) from the tile, reruns the elite refit into the Kstar buffer, reuses the Kstar padding
zeroed once, W, the exp table and the constants, and (rh) starts the state buffers of its step parity again.

Also here: the forms that are not the default at that batch (tools/rw_repro.py, a child process per shape under
SX_ROLLOUT), the refit prologue's scratch at its bound 2 H n_u = 256 (1 + n_s), and gp_predict_kernel past its cap of
4096 workgroups.  The helpers and tolerances are those of the matrix module."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem.ssm_cem import JUNK_FUSED_SHAPES
from test_gpu_rollout_matrix import (CON_MODES, OBJ_MODES, TOL, Constraints, T, assert_non_vacuous, assert_status,
                                     build_model, cached, check_problem, close, constraints_for, oracle_runs, shapes,
                                     system)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM = {'stream': 0, 'rw': 1, 'rh': 2, 'byout': 3}     # SX_FORM_* (include/sx_amd.h)
E = 2
PLAIN = shapes(JUNK_FUSED_SHAPES, True)
# (n_s, n_u, N, the default form): rh where n_pad <= 128 for n_s <= 2, rw for n_s = 3, 4 and for (2, 2) at n_pad = 160
RESIDENT = [(1, 1, 77, 'rh'), (2, 1, 77, 'rh'), (2, 2, 60, 'rh'), (3, 1, 77, 'rw'), (4, 1, 50, 'rw'), (4, 2, 40, 'rw'),
            (2, 2, 150, 'rw')]


@pytest.fixture(autouse=True)
def one_blas_thread():
    """The oracle's per-step solves are tiny: on one BLAS thread a rollout of hundreds of steps takes a second, not ten."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(1):
        yield


def grid():
    """(compute units, P, tiles per problem) of the multi-trip batch: E = 2 problems of P = 16 CU + 37 particles."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = 16 * cu + 37
    tpp = (P + 15) // 16
    assert E * tpp > 2 * cu, (E * tpp, cu)
    return cu, P, tpp


def chosen_tiles(cu, tpp):
    """Whole tiles by global index: the first, one of the second trip, problem 1's first and each problem's ragged last."""
    tiles = sorted({0, cu + 1, tpp, tpp - 1, 2 * tpp - 1})
    assert cu + 1 < tpp - 1 and tpp >= cu and 2 * tpp - 1 >= 2 * cu, 'problem 1 and the ragged tiles on later trips'
    return tiles


def tile_particles(tiles, e, tpp, P):
    """Problem e's particles of these tiles, in order (a ragged tile last, so each keeps its position mod 16)."""
    idx = np.concatenate([np.arange(16 * (t - e * tpp), min(16 * (t - e * tpp + 1), P)) for t in tiles if t // tpp == e])
    assert (idx % 16 == np.arange(idx.size) % 16).all()
    return idx


def subset(run, idx):
    return dataclasses.replace(run, traj_p=run.traj_p[idx], traj_q=run.traj_q[idx], sigma=run.sigma[idx],
                               obj_cost=run.obj_cost[idx], con_cost=run.con_cost[idx])


def polytope(sysd, oracle, x0, acts, q0, seed):
    """constraints_for the first particle of every tile (active_polytope's search grows faster than linearly with the
    particles; the non-vacuity is then asserted over all of them)."""
    return constraints_for(sysd, [oracle] * E, x0, acts[:, ::16], q0=q0, seed=seed)


def form_of(ssm, H):
    return int(_lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), H))


def start_ellipsoids(n_s):
    return np.stack([np.eye(n_s) * 1e-4 * (e + 1) for e in range(E)])


def same_rows_from_a_small_launch(ssm, env, r, x0, q0, acts, tiles, tpp):
    """Each problem's chosen tiles relaunched on their own (one problem, each particle at its position mod 16): the costs,
    trajectories and variances bit for bit those of the big launch."""
    from safe_exploration_amd.cem_mpc import cem_rollout
    H, P = acts.shape[2], acts.shape[1]
    for e in range(E):
        idx = tile_particles(tiles, e, tpp, P)
        s = cem_rollout(ssm, env, T(x0[e:e + 1]), H, actions=T(acts[e:e + 1, idx]), q0=T(q0[e:e + 1]), want_traj=True,
                        want_sigma=True)
        for key in ('obj_cost', 'con_cost', 'traj', 'sigma'):
            torch.testing.assert_close(s[key][0], r[key][e][torch.as_tensor(idx, device=r[key].device)], rtol=0, atol=0,
                                       msg=f'problem {e} tiles {tiles}: {key}')


# ---- 1. the default forms past the first trip ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,N,form', RESIDENT)
def test_given_actions_past_the_first_pass(n_s, n_u, N, form):
    """Given actions, H = 1 (the epilogue alone), 4 and 5 (both step parities of the rh form's state buffers), a start
    ellipsoid per problem, a general polytope of SX_MAX_M rows, both constraint modes and both objectives: every particle
    of both problems against the oracle, the non-vacuity on the particles of the later trips, and the chosen tiles
    relaunched on their own bit for bit."""
    from safe_exploration_amd.cem_mpc import cem_rollout
    ssm, oracle = cached(build_model, 'rbf', n_s, n_u, N, 3)
    cu, P, tpp = grid()
    tiles = chosen_tiles(cu, tpp)
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(70 + 10 * n_s + n_u + N)
    later = [np.flatnonzero(e * tpp + np.arange(P) // 16 >= cu) for e in range(E)]
    for H in (1, 4, 5):
        assert form_of(ssm, H) == FORM[form], (form_of(ssm, H), form)
        x0 = rng.normal(0, 0.02, size=(E, n_s))
        q0 = start_ellipsoids(n_s)
        acts = rng.normal(0, 0.4, size=(E, P, H, n_u))
        con = polytope(sysd, oracle, x0, acts, q0, H)
        runs = [oracle_runs(con, oracle, x0[e], acts[e], q0[e]) for e in range(E)]
        what = f'{form} ({n_s}, {n_u}) N={N} H={H}'
        assert_non_vacuous(con, runs, what)
        assert_non_vacuous(con, [{k: subset(v, later[e]) for k, v in runs[e].items()} for e in range(E)],
                           what + ' later trips')
        for o, c in ((o, c) for o in OBJ_MODES for c in CON_MODES.values()):
            r = cem_rollout(ssm, con.env(o, c), T(x0), H, actions=T(acts), q0=T(q0), want_traj=True, want_sigma=True)
            for e in range(E):
                check_problem(r, e, runs[e][(o, c)], TOL['rbf'], f'{what} obj {o} problem {e}')
            assert_status(r, [runs[e][(o, c)] for e in range(E)], 1)
            same_rows_from_a_small_launch(ssm, con.env(o, c), r, x0, q0, acts, tiles, tpp)


def elites_launch(ssm, env, x0, q0, rows, noise, H, want_traj):
    """sx_cem_rollout_elites: the published refit, the actions against mean + std noise on the host from that refit (every
    tile refits on its own), and the launch bit for bit against the plain entry given that refit."""
    from safe_exploration_amd.cem_mpc import cem_rollout
    r1 = cem_rollout(ssm, env, T(x0), H, elite_rows=T(rows), noise=T(noise), q0=T(q0), want_dist=True,
                     want_traj=want_traj, want_sigma=want_traj)
    k, n_u = rows.shape[1], noise.shape[-1]
    for e in range(E):
        mean, std = ocem.refit(rows[e, :, 2:].reshape(k, H, n_u))
        close(r1['mean'][e], mean, 1e-12, 1e-15, 'mean')
        close(r1['std'][e], std, 1e-12, 1e-15, 'std')
    host = r1['mean'].cpu().numpy()[:, None] + r1['std'].cpu().numpy()[:, None] * noise
    np.testing.assert_allclose(r1['actions'].cpu().numpy(), host, rtol=1e-15, atol=1e-16)
    r2 = cem_rollout(ssm, env, T(x0), H, mean=r1['mean'], std=r1['std'], noise=T(noise), q0=T(q0), want_traj=want_traj,
                     want_sigma=want_traj)
    for key in ('actions', 'obj_cost', 'con_cost', 'status') + (('traj', 'sigma') if want_traj else ()):
        torch.testing.assert_close(r1[key], r2[key], rtol=0, atol=0, msg=f'elites against the plain entry: {key}')
    return r1


@pytest.mark.parametrize('n_s,n_u,N,form', RESIDENT)
def test_elites_past_the_first_pass(n_s, n_u, N, form):
    """sx_cem_rollout_elites at the multi-trip batch (as the matrix module's elites_vs_oracle), H = 5, every state
    constrained, start ellipsoids: the refit, the actions of every particle, the plain entry, every problem's oracle."""
    ssm, oracle = cached(build_model, 'rbf', n_s, n_u, N, 3)
    cu, P, tpp = grid()
    H, k = 5, 9
    assert form_of(ssm, H) == FORM[form]
    sysd = system(n_s, n_u)
    rng = np.random.default_rng(80 + 10 * n_s + n_u + N)
    x0 = rng.normal(0, 0.02, size=(E, n_s))
    q0 = start_ellipsoids(n_s)
    rows = np.concatenate([np.zeros((E, k, 2)), rng.normal(0.0, 0.3, size=(E, k, H * n_u))], axis=2)
    noise = rng.normal(size=(E, P, H, n_u))
    fits = [ocem.refit(rows[e, :, 2:].reshape(k, H, n_u)) for e in range(E)]
    host = np.stack([fits[e][0][None] + fits[e][1][None] * noise[e] for e in range(E)])
    con = polytope(sysd, oracle, x0, host, q0, 7)
    o, c = _lib.SX_OBJ_AFFINE_ABS, _lib.SX_CON_ALL_STATES
    r = elites_launch(ssm, con.env(o, c), x0, q0, rows, noise, H, True)
    acts = r['actions'].cpu().numpy()
    runs = [oracle_runs(con, oracle, x0[e], acts[e], q0[e]) for e in range(E)]
    what = f'elites {form} ({n_s}, {n_u}) N={N}'
    assert_non_vacuous(con, runs, what)
    for e in range(E):
        check_problem(r, e, runs[e][(o, c)], TOL['rbf'], f'{what} problem {e}')
    assert_status(r, [runs[e][(o, c)] for e in range(E)], 1)


# ---- 2. the forms that are not the default, in child processes --------------------------------------------------------------
def rw_repro(form, args, shapes_, timeout):
    env = dict(os.environ, SX_ROLLOUT=form, SX_ROLLOUT_STRICT='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rw_repro.py')] + args + [f'--timeout={timeout}'] +
                       shapes_, capture_output=True, text=True, timeout=len(shapes_) * timeout + 30, env=env)
    assert r.returncode == 0 and 'Memory access fault' not in r.stdout + r.stderr, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize('form,shape', [('rw', '1,1,77'), ('rw', '2,1,77'), ('rw', '2,1,200'), ('stream', '3,1,77')])
def test_forced_form_past_the_first_pass(form, shape):
    """The 4-wave form where the 8-wave one is the default, and the streaming form, at the multi-trip batch with start
    ellipsoids and SX_MAX_M rows: H = 1, 4, 5, both constraint modes, given and sampled from elite rows."""
    cu, P, _ = grid()
    out = rw_repro(form, ['--horizons=1,4,5', '--con-modes=0,1', f'--rows={_lib.SX_MAX_M}', f'--particles={P}',
                          f'--problems={E}', '--q0', '--elites'], [shape], 240)
    assert out.count(f'matches the oracle; form {FORM[form]}') == 3 * 2 * 2, out[-3000:]


# ---- 3. the refit prologue's scratch at its bound ---------------------------------------------------------------------------
def h_max(n_s, n_u):
    return 256 * (1 + n_s) // (2 * n_u)


def contracting(n_s, n_u):
    """The matrix module's system with a contracting prior and small Lipschitz constants: finite ellipsoids over the
    hundreds of steps of the bound."""
    from safe_exploration_amd.utils import dlqr
    sysd = dict(system(n_s, n_u))
    rng = np.random.default_rng(2000 + 10 * n_s + n_u)
    sysd['a'] = 0.6 * np.eye(n_s) + 0.02 * rng.normal(size=(n_s, n_s))
    sysd['k_fb'] = -dlqr(sysd['a'], sysd['b'], np.eye(n_s), 5.0 * np.eye(n_u))[0]
    sysd['l_mu'], sysd['l_sigma'] = rng.uniform(0.001, 0.003, size=n_s), rng.uniform(0.001, 0.003, size=n_s)
    return sysd


def refused_without_a_launch(ssm, env, P, H):
    """sx_cem_rollout_elites at H answers SX_ERR_UNSUPPORTED and writes none of its outputs."""
    n_s, n_u, k = ssm.num_states, ssm.num_actions, 3
    x0 = torch.zeros((E, n_s), dtype=torch.float64, device='cuda:0')
    rows = torch.zeros((E, k, 2 + H * n_u), dtype=torch.float64, device='cuda:0')
    noise = torch.zeros((E, P, H, n_u), dtype=torch.float64, device='cuda:0')
    outs = [torch.full(shape, np.nan, dtype=torch.float64, device='cuda:0')
            for shape in ((E, P, H, n_u), (E, P), (E, P), (E, H, n_u), (E, H, n_u))]
    status = torch.full((1,), -7, dtype=torch.int32, device='cuda:0')
    acts, obj, con, mean, std = outs
    p = _lib.ptr
    rc = _lib.lib().sx_cem_rollout_elites(ctypes.byref(ssm.device_model), ctypes.byref(env), E, P, H, p(x0), None, p(rows),
                                          k, p(noise), p(acts), None, None, p(obj), p(con), p(status), p(mean), p(std),
                                          _lib.stream_ptr(x0.device))
    torch.cuda.synchronize()
    assert rc == _lib.SX_ERR_UNSUPPORTED, rc
    assert all(bool(t.isnan().all()) for t in outs) and int(status.item()) == -7, 'a refused launch wrote its outputs'


@pytest.mark.parametrize('N', [8, 40])
@pytest.mark.parametrize('n_s,n_u', PLAIN)
def test_refit_scratch_at_its_bound(n_s, n_u, N):
    """2 H n_u = 256 (1 + n_s) means and standard deviations in the prologue's scratch (the Kstar buffer and the mean
    rows), on the smallest training set (N = 8: n_pad = 16, one Kstar pair and one padding pair that the scratch
    overwrites) and a mid-sized one, in the default form: fused_refit_applies and the plan draw the line at H_max, and at
    H_max the refit, every action, the plain entry and the costs of the chosen whole tiles match."""
    from safe_exploration_amd.cem_mpc import fused_refit_applies
    ssm, oracle = cached(build_model, 'rbf', n_s, n_u, N, 4)
    if N == 8:
        assert ssm.device_model.n_pad == 16
    cu, P, tpp = grid()
    tiles = chosen_tiles(cu, tpp)
    H, k = h_max(n_s, n_u), 9
    assert fused_refit_applies(ssm, E, P, H) and not fused_refit_applies(ssm, E, P, H + 1)
    assert form_of(ssm, H) in (FORM['stream'], FORM['rw'], FORM['rh'])
    sysd = contracting(n_s, n_u)
    box = Constraints(sysd, np.vstack((np.eye(n_s), -np.eye(n_s))), np.full((2 * n_s, 1), 1.0), np.full(n_u, -1e3),
                      np.full(n_u, 1e3))
    o, c = _lib.SX_OBJ_AFFINE_ABS, _lib.SX_CON_ALL_STATES
    env = box.env(o, c)
    refused_without_a_launch(ssm, env, P, H + 1)
    rng = np.random.default_rng(90 + 10 * n_s + n_u + N)
    x0 = rng.normal(0, 0.02, size=(E, n_s))
    q0 = start_ellipsoids(n_s)
    rows = np.concatenate([np.zeros((E, k, 2)), rng.normal(0.0, 0.3, size=(E, k, H * n_u))], axis=2)
    noise = rng.normal(size=(E, P, H, n_u))
    r = elites_launch(ssm, env, x0, q0, rows, noise, H, False)
    acts = r['actions'].cpu().numpy()
    refs = []
    for e in range(E):
        idx = tile_particles(tiles, e, tpp, P)
        ref = ocem.rollout(box.problem(o, c), oracle, x0[e], acts[e][idx], q0[e])
        assert np.isfinite(ref.traj_q).all() and np.abs(ref.traj_q).max() < 1.0, 'the ellipsoids grow'
        close(r['obj_cost'][e].cpu().numpy()[idx], ref.obj_cost, TOL['rbf'][1], TOL['rbf'][2], f'problem {e}: obj_cost')
        np.testing.assert_array_equal(r['con_cost'][e].cpu().numpy()[idx], ref.con_cost, err_msg=f'problem {e}: con_cost')
        refs.append(ref)
    assert_status(r, refs, 1)


@pytest.mark.parametrize('form', ['rw', 'stream'])
@pytest.mark.parametrize('n_s,n_u', PLAIN)
def test_refit_scratch_at_its_bound_in_forced_forms(form, n_s, n_u):
    """The refit bound of test_refit_scratch_at_its_bound in the 4-wave and the streaming form (tools/rw_repro.py
    --refit-bound in a child process) on the smallest training set, N = 8 (n_pad = 16)."""
    cu, P, _ = grid()
    out = rw_repro(form, ['--refit-bound', f'--particles={P}', f'--problems={E}', '--q0'], [f'{n_s},{n_u},8'], 120)
    assert out.count(f'matches the oracle; form {FORM[form]}') == 1, out[-3000:]
    assert f'H={h_max(n_s, n_u)} at the refit bound, N=8, n_pad=16' in out, out[-3000:]


# ---- 4. GP predict past 4096 workgroups -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,N,n_pad,kernel', [(2, 1, 77, 96, 'all outputs'), (3, 1, 500, 512, 'by output')])
def test_gp_predict_past_4096_workgroups(n_s, n_u, N, n_pad, kernel):
    """sx_gp_predict (predict_with_jacobians, predict_without_jacobians) of P = 4096 16 + 37 points: 4099 tiles on a grid
    capped at 4096 workgroups, so tiles 4096 .. 4098 run on a second trip of the tile loop.  Which kernel runs follows
    from predict_fits (csrc/sx_gp_predict.hip), the LDS of gp_tile_lds_doubles on 8 waves against 160 KiB:
    (2, 1), N = 77, n_pad = 96: 4736 doubles (37 KiB) with every output resident, gp_predict_kernel<2, 1, false>;
    (3, 1), N = 500, n_pad = 512: 28416 doubles (222 KiB) do not fit, 12032 (94 KiB) one output at a time do,
    gp_predict_kernel<3, 1, true>.  The rows of tiles 0, 4095, 4096 and the ragged last tile equal a small launch of those
    tiles (each point at its position mod 16) bit for bit and match ExactGP.predict."""
    ssm, oracle = cached(build_model, 'rbf', n_s, n_u, N, 5)
    assert ssm.device_model.n_pad == n_pad
    P = 4096 * 16 + 37
    tiles = [0, 4095, 4096, (P - 1) // 16]
    rng = np.random.default_rng(10 * n_s + n_u + N)
    z = rng.uniform(-0.5, 0.5, size=(P, n_s + n_u))
    idx = tile_particles(tiles, 0, (P + 15) // 16, P)
    big = ssm.predict_with_jacobians(T(z[:, :n_s]), T(z[:, n_s:]))
    big_nj = ssm.predict_without_jacobians(T(z[:, :n_s]), T(z[:, n_s:]))
    small = ssm.predict_with_jacobians(T(z[idx, :n_s]), T(z[idx, n_s:]))
    small_nj = ssm.predict_without_jacobians(T(z[idx, :n_s]), T(z[idx, n_s:]))
    sel = torch.as_tensor(idx, device=big[0].device)
    for name, b, s in zip(('mean', 'var', 'jac', 'mean (no jac)', 'var (no jac)'), big + big_nj, small + small_nj):
        torch.testing.assert_close(s, b[sel], rtol=0, atol=0, msg=f'{kernel}: {name}')
    mo, vo, jo = oracle.predict(z[idx])
    for m, v in (big[:2], big_nj):
        np.testing.assert_allclose(m[sel].cpu().numpy(), mo, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(v[sel].cpu().numpy(), vo, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(big[2][sel].cpu().numpy(), jo, rtol=1e-9, atol=1e-11)
