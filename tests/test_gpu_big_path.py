"""GPU: the large-N path (csrc/sx_big.hpp: kstar_big_kernel, trmm_reduce_kernel, step_big_kernel /
predict_collect_big_kernel) through sx_gp_predict and sx_cem_rollout, in every tiling the launcher picks by itself and every
A/B setting it offers, against the oracle.

trmm_reduce_kernel runs 128 x 64 or 128 x 128 tiles (PT = 4 | 8) in longest-first (8) or paired (16) order; each test names
the route it means and asserts through sx_gp_big_tiling that the launch takes it (the particle counts are chosen by that
query, not by a restated rule), and prints what the query reported.  Every launch runs over a NaN-filled workspace
(big_path_case.poison): a slot it reads without having written it ends in its outputs.  The tolerances against the oracle
are those of test_gpu_solver.py's test_gp_predict_large_training_set_vs_oracle (predict) and
test_large_training_set_path_vs_oracle (rollouts).

  a  the four default routes and both parities of row_tiles in the paired order: a full batch of distinct particles, a
     sub-sample of it run alone (bit-identical: the partial sums have a fixed order), the sub-sample against the oracle
  b  the mean / Jacobian rows n_train .. n_train + D across a wave-row boundary, across a tile boundary, alone in the last
     tile; the smallest training set of every shape that takes the path
  c  a NaN query point keeps to its own row
  d  SX_TRMM_PT / SX_TRMM_VARIANT / SX_TRMM_ORDER, a child process per setting, bit for bit against the default"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import big_path_case as bp
import test_gpu_rollout_matrix as rm
from big_path_case import H
from oracle import cases
from oracle import cem as ocem
from safe_exploration_amd import _lib
from test_rollout_plan import _model

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(any(os.environ.get(v) for v in bp.SETTINGS), reason='SX_TRMM_* force a tiling')]
SHAPES = rm.shapes(rm.JUNK_FUSED_SHAPES, True)      # the six shift-0 shapes of SX_ROLLOUT_SHAPES
LONGEST, PAIRED = 8, 16
FEW = 37                                            # particles of the longest-first launches of section b


# ---- routes -------------------------------------------------------------------------------------------------------------
def assert_route(ssm, particles, pt, order, what):
    """The tiling sx_gp_big_tiling reports for this launch is the one the test names."""
    t = _lib.big_tiling(ssm.device_model, particles)
    print(f'route: {what}: n_pad {ssm.device_model.n_pad}, {particles} particles -> PT {t["pt"]}, order {t["order"]}, '
          f'variant {t["variant"]}, grid {t["grid"]}')
    assert (t['pt'], t['order'], t['variant']) == (pt, order, 13), (what, t)
    return t


def paired_count(model):
    """The smallest particle count 128 k - 5 (a partial last group, no multiple of 16) that the launcher runs in paired
    order, and its PT, by the query."""
    for k in range(1, 65):
        t = _lib.big_tiling(model, 128 * k - 5)
        if t['order'] == PAIRED:
            return 128 * k - 5, t['pt']
    raise AssertionError('no particle count up to 8192 runs in paired order')


def edge_indices(total, pt):
    """The first and the last particle, and both neighbours of the 16-, 64- and 128-particle boundaries after the start of
    the first, a middle and the last (partial) particle group of 16 pt."""
    width = 16 * pt
    groups = (total + width - 1) // width
    assert total % width, 'the last group is partial'
    idx = {0, total - 1}
    for g in {0, groups // 2, groups - 1}:
        for b in (16, 64, 128):
            idx |= {g * width + b - 1, g * width + b}
    return sorted(i for i in idx if 0 <= i < total)


def subsample(rng, E, P, pt, most=128):
    """[E x n] particles of each problem, E n <= most: edge_indices of the whole batch, both sides of every problem
    boundary, and random others up to n per problem."""
    glob = set(edge_indices(E * P, pt)) | {e * P - 1 for e in range(1, E)} | {e * P for e in range(1, E)}
    n = min(P, most // E)
    out = []
    for e in range(E):
        mine = sorted(g - e * P for g in glob if e * P <= g < (e + 1) * P)
        assert len(mine) <= n
        rest = [i for i in rng.permutation(P) if i not in mine]
        out.append(sorted(mine + rest[:n - len(mine)]))
    return np.array(out)


# ---- models -------------------------------------------------------------------------------------------------------------
def model(n_s, n_u, N):
    """(ssm, oracle) of rm.build_model('rbf', ...), shared with test_gpu_rollout_matrix.py's own large models."""
    return rm.cached(rm.build_model, 'rbf', n_s, n_u, N, 2)


@functools.lru_cache(maxsize=None)
def big_threshold(n_s, n_u, entry):
    """The smallest N whose model takes the large-N path of `entry` ('predict' | 'rollout'), walking N upward on the host."""
    lib = _lib.lib()
    big = {'rollout': lambda m: lib.sx_cem_rollout_form(ctypes.byref(m), H) == bp.SX_FORM_BIG,
           'predict': lambda m: lib.sx_gp_predict_workspace_bytes(ctypes.byref(m), FEW) > 0}[entry]
    for N in range(64, 4096):
        if big(_model(n_s, n_u, N)):
            assert not big(_model(n_s, n_u, N - 1))
            return N
    raise AssertionError('no model takes the large-N path')


# ---- the comparisons ----------------------------------------------------------------------------------------------------
def close(a, b, rtol, atol, what):
    np.testing.assert_allclose(a.cpu().numpy() if torch.is_tensor(a) else a, b, rtol=rtol, atol=atol, err_msg=what)


def predict_vs_oracle(got, oracle, z, what):
    """test_gp_predict_large_training_set_vs_oracle's tolerances."""
    mo, vo, jo = oracle.predict(z)
    close(got[0], mo, 1e-8, 1e-11, what + ': mean')
    close(got[1], vo, 1e-7, 1e-11, what + ': var')
    close(got[2], jo, 1e-8, 1e-10, what + ': jac')


def rollout_vs_oracle(r, con, modes, oracle, x0, acts, q0, what):
    """Every problem of a launch against ocem.rollout with test_large_training_set_path_vs_oracle's tolerances; the
    constraint cost exactly (no ellipsoid within 1e-9 of a face), the status word."""
    E, P = acts.shape[:2]
    n_s = x0.shape[1]
    status = 0
    for e in range(E):
        ref = ocem.rollout(con.problem(*modes), oracle, x0[e], acts[e], q0[e])
        assert cases.min_abs_distance(ref.traj_p, ref.traj_q, con.h_mat, con.h_vec) > 1e-9, what + ': a face is touched'
        traj = r['traj'][e].cpu().numpy()
        close(traj[..., :n_s], ref.traj_p, 1e-8, 1e-11, f'{what} problem {e}: centres')
        close(traj[..., n_s:].reshape(P, H, n_s, n_s), ref.traj_q, 1e-7, 1e-11, f'{what} problem {e}: shapes')
        close(r['sigma'][e], ref.sigma, 1e-7, 1e-12, f'{what} problem {e}: sigma')
        close(r['obj_cost'][e], ref.obj_cost, 1e-7, 1e-12, f'{what} problem {e}: obj_cost')
        np.testing.assert_array_equal(r['con_cost'][e].cpu().numpy(), ref.con_cost, err_msg=f'{what} problem {e}: con_cost')
        status |= ref.status
    assert int(r['status'].item()) == status == 0, what


def rollout_problem(rng, oracle, n_s, n_u, E, acts, seed):
    """Start ellipsoids and a 2 n_s-row polytope that the oracle's trajectories of `acts` ([E x n x H x n_u]) cross."""
    x0, q0 = bp.start_ellipsoids(rng, E, n_s)
    con = rm.constraints_for(rm.system(n_s, n_u), [oracle] * E, x0, acts, q0=q0, m=2 * n_s, seed=seed)
    return x0, q0, con


# ---- a. every default route ---------------------------------------------------------------------------------------------
# (n_s, n_u, N, problems, particles per problem, PT, order): the four routes at (4, 2), N = 1100 (9 row tiles: the paired order
# has an unpaired middle tile), 128 x 128 paired tiles over an even 16 row tiles, 128 x 64 paired tiles over 9
ROUTES = [(4, 2, 1100, 1, 130, 4, LONGEST), (4, 2, 1100, 1, 600, 4, PAIRED), (4, 2, 1100, 1, 5400, 8, PAIRED),
          (4, 2, 1100, 1, 6200, 8, LONGEST), (4, 1, 2000, 1, 4090, 8, PAIRED), (2, 1, 1100, 1, 1107, 4, PAIRED),
          (4, 2, 1100, 2, 299, 4, PAIRED)]      # two problems, the boundary inside a 16-particle tile
ROW_TILES = {1100: 9, 2000: 16}


@pytest.mark.parametrize('n_s,n_u,N,E,P,pt,order', [r for r in ROUTES if r[3] == 1])
def test_predict_full_batch_equals_its_subsample_and_the_oracle(n_s, n_u, N, E, P, pt, order):
    """sx_gp_predict with Jacobians at P distinct points in the route named; at most 128 of them (edge_indices) alone, bit
    for bit the same; those against the oracle."""
    ssm, oracle = model(n_s, n_u, N)
    assert (ssm.device_model.n_pad + 127) // 128 == ROW_TILES[N]
    what = f'predict ({n_s},{n_u}) N={N} P={P}'
    assert_route(ssm, P, pt, order, what)
    rng = np.random.default_rng(100 * n_s + 10 * n_u + P)
    z = rng.uniform(-0.5, 0.5, size=(P, n_s + n_u))
    idx = subsample(rng, 1, P, pt)[0]
    full = bp.predict(ssm, z)
    t = _lib.big_tiling(ssm.device_model, len(idx))
    print(f'route: {what}: its {len(idx)}-particle sub-sample -> PT {t["pt"]}, order {t["order"]}, grid {t["grid"]}')
    small = bp.predict(ssm, z[idx])
    for f, s, name in zip(full, small, ('mean', 'var', 'jac')):
        assert bool(torch.isfinite(f).all()), f'{what}: {name} of the full batch'
        assert torch.equal(f[torch.as_tensor(idx, device=f.device)], s), f'{what}: {name}'
    predict_vs_oracle(small, oracle, z[idx], what)


@pytest.mark.parametrize('n_s,n_u,N,E,P,pt,order', ROUTES)
def test_rollout_full_batch_equals_its_subsample_and_the_oracle(n_s, n_u, N, E, P, pt, order):
    """sx_cem_rollout, H = 2 from an ellipsoid, E P distinct action sequences in the route named; at most 128 of them alone,
    bit for bit the same; those against the oracle."""
    ssm, oracle = model(n_s, n_u, N)
    what = f'rollout ({n_s},{n_u}) N={N} E={E} P={P}'
    assert E == 1 or P % 16
    assert_route(ssm, E * P, pt, order, what)
    rng = np.random.default_rng(200 * n_s + 20 * n_u + E * P)
    acts = rng.normal(0, 0.4, size=(E, P, H, n_u))
    idx = subsample(rng, E, P, pt)
    sub = np.stack([acts[e, idx[e]] for e in range(E)])
    x0, q0, con = rollout_problem(rng, oracle, n_s, n_u, E, sub, P)
    modes = (_lib.SX_OBJ_AFFINE_ABS, _lib.SX_CON_ALL_STATES)
    full = bp.rollout(ssm, con.env(*modes), x0, acts, q0)
    t = _lib.big_tiling(ssm.device_model, sub.shape[0] * sub.shape[1])
    print(f'route: {what}: its {E} x {sub.shape[1]}-particle sub-sample -> PT {t["pt"]}, order {t["order"]}, grid {t["grid"]}')
    small = bp.rollout(ssm, con.env(*modes), x0, sub, q0)
    for key in ('obj_cost', 'con_cost', 'traj', 'sigma'):
        assert bool(torch.isfinite(full[key]).all()), f'{what}: {key} of the full batch'
        for e in range(E):
            assert torch.equal(full[key][e][torch.as_tensor(idx[e], device=rm.DEV)], small[key][e]), f'{what}: {key}'
    rollout_vs_oracle(small, con, modes, oracle, x0, sub, q0, what)


# ---- b. row edges -------------------------------------------------------------------------------------------------------
# (2, 1), D = 3: where the mean / Jacobian rows N .. N + 3 of the padded W fall in trmm_reduce_kernel's 128-row tiles and
# 64-row wave rows
ROW_EDGES = {1086: 'rows 1086 .. 1089 cross the wave-row boundary 1088 inside tile 8',
             1149: 'rows 1149 .. 1152 cross the tile boundary 1152: tile 9 holds the last Jacobian row only',
             1151: 'the mean row 1151 ends tile 8, every Jacobian row is in tile 9',
             1152: 'training rows fill nine tiles exactly'}


# (n_s, n_u, N) of section b; N = None: the shape's smallest N on the path (big_threshold)
EDGE_SIZES = [(2, 1, N) for N in ROW_EDGES] + [(n_s, n_u, None) for n_s, n_u in SHAPES]


def both_orders(ssm, what):
    """(particles, order) of a longest-first launch of few particles and of a paired one, by the query."""
    assert_route(ssm, FEW, 4, LONGEST, what)
    P, pt = paired_count(ssm.device_model)
    assert_route(ssm, P, pt, PAIRED, what)
    return [FEW, P]


@pytest.mark.parametrize('n_s,n_u,N', EDGE_SIZES)
def test_predict_at_the_row_edges_vs_oracle(n_s, n_u, N):
    """sx_gp_predict with Jacobians on the large-N path at the row edges of trmm_reduce_kernel's epilogue (ROW_EDGES; the
    smallest N of the shape on the path, where N is None), in longest-first and in paired order: every point against the
    oracle."""
    N = N or big_threshold(n_s, n_u, 'predict')
    ssm, oracle = model(n_s, n_u, N)
    assert _lib.lib().sx_gp_predict_workspace_bytes(ctypes.byref(ssm.device_model), FEW) > 0
    what = f'predict ({n_s},{n_u}) N={N}'
    rng = np.random.default_rng(300 + N)
    for P in both_orders(ssm, what):
        z = rng.uniform(-0.5, 0.5, size=(P, n_s + n_u))
        predict_vs_oracle(bp.predict(ssm, z), oracle, z, f'{what} P={P}')


@pytest.mark.parametrize('n_s,n_u,N', EDGE_SIZES)
def test_rollout_at_the_row_edges_vs_oracle(n_s, n_u, N):
    """sx_cem_rollout, H = 2 from an ellipsoid, in the three-launch form at the same row edges, in longest-first and in paired
    order: every particle against the oracle (the polytope is chosen from the first 64)."""
    N = N or big_threshold(n_s, n_u, 'rollout')
    ssm, oracle = model(n_s, n_u, N)
    assert _lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), H) == bp.SX_FORM_BIG
    what = f'rollout ({n_s},{n_u}) N={N}'
    rng = np.random.default_rng(400 + N)
    modes = (_lib.SX_OBJ_NEG_VARIANCE, _lib.SX_CON_ALL_STATES)
    for P in both_orders(ssm, what):
        acts = rng.normal(0, 0.4, size=(1, P, H, n_u))
        x0, q0, con = rollout_problem(rng, oracle, n_s, n_u, 1, acts[:, :64], N + P)
        r = bp.rollout(ssm, con.env(*modes), x0, acts, q0)
        rollout_vs_oracle(r, con, modes, oracle, x0, acts, q0, f'{what} P={P}')


# ---- c. a NaN query ------------------------------------------------------------------------------------------------------
def test_a_nan_query_point_keeps_to_its_row():
    """One NaN coordinate in one query point in the middle of a 16-particle tile, paired order: that point's mean, variance
    and Jacobian are NaN, every other point's are bit for bit those of the run without it."""
    n_s, n_u, N, P = 2, 1, 1100, 1107
    ssm, _ = model(n_s, n_u, N)
    assert_route(ssm, P, 4, PAIRED, 'predict with a NaN query')
    z = np.random.default_rng(5).uniform(-0.5, 0.5, size=(P, n_s + n_u))
    clean = bp.predict(ssm, z)
    bad = 16 * 34 + 7
    z[bad, 1] = np.nan
    dirty = bp.predict(ssm, z)
    others = torch.arange(P, device=rm.DEV) != bad
    for c, d, name in zip(clean, dirty, ('mean', 'var', 'jac')):
        assert bool(torch.isfinite(c).all()), name
        assert bool(torch.isnan(d[bad]).all()), name
        assert torch.equal(c[others], d[others]), name


# ---- d. the A/B settings -------------------------------------------------------------------------------------------------
AB_SETTINGS = [dict(SX_TRMM_PT=8, SX_TRMM_VARIANT=v) for v in (12, 22, 23)] + \
              [dict(SX_TRMM_PT=4, SX_TRMM_ORDER=o) for o in (0, 1, 8, 16)] + \
              [dict(SX_TRMM_PT=8, SX_TRMM_ORDER=o) for o in (1, 16)]
_child_died = False      # a child ended on a signal or a timeout: nothing more is started on the card


@functools.lru_cache(maxsize=None)
def ab_default():
    return bp.ab_case()


@pytest.mark.parametrize('setting', AB_SETTINGS, ids=lambda s: '-'.join(f'{k[8:]}{v}' for k, v in s.items()))
def test_ab_setting_equals_the_default_bit_for_bit(setting, tmp_path):
    """big_path_case.py's fixed case in a child process under one setting of SX_TRMM_*: the child's own query reports the
    setting, and its predict and rollout outputs are bit for bit those of this process without any."""
    global _child_died
    if _child_died:
        pytest.skip('an earlier child ended on a signal or a timeout')
    want = ab_default()
    assert tuple(want['tiling'][:3]) == (4, PAIRED, 13)
    out = tmp_path / 'ab.npz'
    env = {k: v for k, v in os.environ.items() if k not in bp.SETTINGS}
    env.update({k: str(v) for k, v in setting.items()})
    try:
        p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'big_path_case.py'),
                            str(out)], capture_output=True, text=True, env=env, timeout=300)
    except subprocess.TimeoutExpired:
        _child_died = True
        raise
    _child_died = p.returncode < 0
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    got = np.load(out)
    pt, order, variant, grid = (int(v) for v in got['tiling'])
    print(f'route: A/B {setting}: {bp.AB_P} particles -> PT {pt}, order {order}, variant {variant}, grid {grid}')
    assert pt == setting['SX_TRMM_PT'] and variant == setting.get('SX_TRMM_VARIANT', 13)
    if 'SX_TRMM_ORDER' in setting:
        assert order == setting['SX_TRMM_ORDER']
        assert order != 1 or grid % 8 == 0, 'order 1 would fall back to the plain order'
    for key in want:
        if key != 'tiling':
            assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), (setting, key)
