"""GPU: the SafeMPC constraint set of the CEM rollout -- sx_conset_eval against the numpy oracle
(tests/conset_oracle.py); sx_cem_rollout_cons / sx_cem_rollout_elites_cons (cem_rollout_kernel<StreamCons<SAT>>) with the empty
set against the streaming parent, bit for bit, and with a full set against the empty-set launch plus the oracle's extra cost of the
kernel's own trajectory; the fused rollout against the step-by-step one; the solve of tests/conset_oracle.py through
FusedCemMpc(con_set=...); and CemSafeMPC through its two conf settings.

Shapes: P = 37 (three tiles, the last one partial), E = 2; (n_s, n_u, N) in {(2,1,7), (2,1,200), (4,1,200), (4,1,590: output
by output), (2,2,200), (3,1,200), (1,1,200), (4,2,200)}; H = 3 and 15; the given, drawn and elite-row forms; cost = NULL and a
SaturatingCost (cost_of of tests/test_gpu_safety_sat.py; a full-rank cost with the angle at 0 for n_s = 1); one case at
P = 4149, one with a q0, and the main case of the oracle (the pendulum, P = 256, H = 5), where every signal is mixed.

Comparisons.  The constraint cost is a sum of 3s and 10s decided by the sign of distances: it is compared EXACTLY, which is
sound because no distance of the inputs sits within 1e-6 of the boundary (asserted on the oracle's numbers in every case; the
kernel's distances and the oracle's are the same few products in another order, within 1e-12).  The empty set: every output,
con_cost and obj_cost included, is bit-equal to the streaming kernel of the parent entry (sx_cem_rollout[_elites] under
SX_ROLLOUT=stream, in one child process) and within TOL['rbf'] of the parent where it takes a resident form; with a cost it is
bit-equal to sx_cem_rollout[_elites]_sat, which tests/test_gpu_safety_sat.py holds to the oracle.  A full set: everything but
con_cost is bit-equal to the empty-set launch.  Fused against step by step: constraint costs exactly, the saturating objective
within LOSS_TOL per step as tests/test_gpu_safety_sat.py holds it, env's objective within TOL['rbf']'s objective tolerance.  A
solve: constraint costs exactly, equal elite sets, best row within 1e-9.  Every case prints its figures before it asserts."""
import ctypes
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # (this file is also the child process of the bit-equality check)
    sys.path.insert(0, ROOT)

import conset_oracle as co
import sat_cost_oracle as so
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc, problems
from safe_exploration_amd.costs import SaturatingCost
from safe_exploration_amd.gp_reachability_pytorch import make_env
from test_gpu_junk_fused import CountingLib
from test_gpu_perf_var import ABS, DEV, N_, T, case, worst
from test_gpu_rollout_matrix import TOL
from test_gpu_safety_sat import (E, KINDS, LARGE, SMALL, STEPS, assert_close_to_parent, cost_of, inputs, names_of,
                                 seed_of, split)
from test_gpu_sat_cost import LOSS_TOL
from test_sat_cost_host import random_weight

pytestmark = pytest.mark.gpu
CASES = [(2, 1, 7), (2, 1, 200), (4, 1, 200), (4, 1, 590), (2, 2, 200), (3, 1, 200), (1, 1, 200), (4, 2, 200)]
RTOL_P, RTOL, ATOL = TOL['rbf']
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3


def cost_for(n_s):
    """(SaturatingCost, its oracle twin) of a case."""
    if n_s > 1:
        return cost_of(n_s)
    z, w = np.array([0.1, 0.9]), random_weight(np.random.default_rng(79), 2, 2) * 0.4
    return SaturatingCost(z, w, 0), so.Cost(z, w, 0)


def set_for(n_s):
    """The full set of the synthetic cases (tests/test_gpu_perf_var.case: |u| <= 1, x0 ~ 0.05, states that reach ~0.2 after
    three steps and ~0.5 after fifteen): the feedback bounds, and as the obstacle the slab -0.3 <= x_0 <= 0.15."""
    e0 = np.eye(n_s)[:1]
    return co.ConSet(np.vstack((e0, -e0)), np.array([0.15, 0.3]), True)


def launch(ssm, env, inp, H, kind, con=None, cost=None, q0=None):
    """One rollout through cem_rollout: the parent entry, _sat (cost), or _cons (con: a conset_oracle.ConSet)."""
    kw = dict(want_traj=True, want_sigma=True, **({} if cost is None else dict(cost=cost)),
              **({} if con is None else dict(con_set=con.struct(ssm.num_states))), **({} if q0 is None else dict(q0=T(q0))))
    if kind == 'given':
        kw.update(actions=T(inp['actions']))
    elif kind == 'drawn':
        kw.update(mean=T(inp['mean']), std=T(inp['std']), noise=T(inp['noise']))
    else:
        kw.update(elite_rows=T(inp['elite']), noise=T(inp['noise']), want_dist=True)
    out = cem_mpc.cem_rollout(ssm, env, T(inp['x0']), H, **kw)
    torch.cuda.synchronize()
    return out


def check_full_set(label, prob, con, empty, full, kind, n_s, q0=None):
    """Everything but con_cost is the empty-set launch's bits; con_cost is the empty-set launch's plus the oracle's extra cost
    of the kernel's own trajectory, exactly.  Returns the signals per problem."""
    for name in names_of(kind) + ('obj_cost',):
        if name != 'con_cost':
            assert torch.equal(full[name], empty[name]), f'{label}: {name} differs from the empty-set launch'
    out = []
    for e in range(full['con_cost'].size(0)):
        tp, tq = split(full['traj'][e], n_s)
        s = co.signals(prob, con, tp, tq, N_(full['actions'][e]), None if q0 is None else q0[e])
        got, want = N_(full['con_cost'][e]), N_(empty['con_cost'][e]) + s.extra
        print(f'{label} e={e}: con_cost differs from empty + oracle at {int((got != want).sum())} of {len(got)} rows (worst '
              f'{np.abs(got - want).max():.1f}); steps box-violated {int(s.box.sum())}, ellipsoid-violated with the box '
              f'satisfied {int((s.ell & ~s.box).sum())}, obstacle-violated {int(s.obs.sum())}; smallest |d| {s.min_abs_d:.2e}')
        assert s.min_abs_d >= co.MARGIN, f'{label}: a distance sits at the boundary: the exact comparison is not sound'
        np.testing.assert_array_equal(got, want, err_msg=label)
        out.append(s)
    return out


# ---- 1: sx_conset_eval against the oracle -------------------------------------------------------------------------------------------
def eval_inputs(n_s, n_u, P=SMALL):
    """The inputs of the sx_conset_eval case (numpy only): sx_env, the oracle's Problem, u, q_start, p_next, q_next, the sets."""
    rng = np.random.default_rng(300 + 10 * n_s + n_u)
    k_fb = rng.uniform(-6.0, 6.0, size=(n_u, n_s))
    u_min, u_max = -rng.uniform(0.8, 1.2, size=n_u), rng.uniform(0.8, 1.2, size=n_u)
    env = make_env(n_s, n_u, k_fb=k_fb, u_min=u_min, u_max=u_max, h_mat=np.eye(n_s), h_vec=np.ones(n_s))
    prob = ocem.Problem(n_s, n_u, np.eye(n_s), np.zeros((n_s, n_u)), k_fb, np.zeros(n_s), np.zeros(n_s), 1.0, np.eye(n_s),
                        np.ones((n_s, 1)), u_min, u_max)

    def spd(scale):
        a = rng.normal(size=(P, n_s, n_s)) * scale
        return a @ a.transpose(0, 2, 1) + 1e-6 * np.eye(n_s)

    u = rng.normal(0, 0.7, size=(P, n_u))
    q_start, p_next, q_next = spd(0.05), rng.normal(0, 0.4, size=(P, n_s)), spd(0.15)
    # the edge rows: a NaN in Q (not a violation: the box alone decides), and an all-zero Q with u == u_max (d = 0: violates)
    q_start[0, 0, n_s - 1] = np.nan
    u[0] = 0.5 * u_max
    q_start[1] = 0.0
    u[1] = u_max
    q_next[2, 0, 0] = np.nan
    rows = lambda m: rng.normal(size=(m, n_s)) * rng.choice([-1.0, 1.0], size=(m, 1))
    sets = {'two rows': co.ConSet(np.vstack((np.eye(n_s)[:1], -np.eye(n_s)[:1])), np.array([0.3, 0.4]), True),
            'SX_MAX_M rows': co.ConSet(rows(_lib.SX_MAX_M), rng.uniform(0.8, 2.0, size=_lib.SX_MAX_M), True),
            'no rows': co.ConSet(np.zeros((0, n_s)), np.zeros(0), True),
            'rows without the feedback bounds': co.ConSet(rows(3), rng.uniform(0.3, 0.8, size=3), False),
            'empty': co.empty(n_s)}
    return env, prob, u, q_start, p_next, q_next, sets


@pytest.mark.parametrize('n_s,n_u', [(1, 1), (2, 1), (4, 1), (2, 2), (4, 2)])
def test_conset_eval_against_the_oracle(n_s, n_u):
    P = SMALL
    env, prob, u, q_start, p_next, q_next, sets = eval_inputs(n_s, n_u)
    smallest = np.inf
    for name, con in sets.items():
        for q0 in (q_start, None):
            for check in (True, False):
                got = N_(cem_mpc.conset_eval(env, con.struct(n_s), T(u), None if q0 is None else T(q0), T(p_next), T(q_next),
                                             check))
                want = co.step_cost(prob, con, u, q0, p_next, q_next, check)
                d = [co.ctrl_distances(prob, u, q_start)] + ([co.obstacle_distances(con, p_next, q_next)] if len(con.h_obs) else [])
                smallest = min(smallest, min(float(np.nanmin(np.abs(x[2:]))) for x in d))
                print(f'({n_s},{n_u}) {name}, q_start {"given" if q0 is not None else "NULL"}, check_obstacle {int(check)}: '
                      f'differs at {int((got != want).sum())} of {P}; costs {sorted(set(want.tolist()))}')
                np.testing.assert_array_equal(got, want)
                if q0 is not None and con.ctrl_ellipsoid:
                    # d = 0 violates; a NaN distance does not
                    assert got[1] % 10.0 == 3.0 and got[0] % 10.0 == 0.0
                if q0 is None or not con.ctrl_ellipsoid:
                    assert got[1] % 10.0 == 0.0      # u == u_max passes the strict box test
                if not check or not len(con.h_obs):
                    assert set(got.tolist()) <= {0.0, 3.0}
        # p_next / q_next may be NULL where no obstacle row is read
        if not len(con.h_obs):
            free = N_(cem_mpc.conset_eval(env, con.struct(n_s), T(u), T(q_start), None, None, True))
            np.testing.assert_array_equal(free, co.step_cost(prob, con, u, q_start, p_next, q_next, True))
    print(f'({n_s},{n_u}): smallest |d| of the rows without an edge {smallest:.2e}')
    assert smallest >= co.MARGIN
    both = co.step_cost(prob, sets['two rows'], u, q_start, p_next, q_next, True)
    assert {3.0, 10.0, 13.0} <= set(both.tolist()) <= {0.0, 3.0, 10.0, 13.0}, 'the signals of the inputs are not mixed'
    none = co.step_cost(prob, sets['empty'], u, q_start, p_next, q_next, True)
    assert set(none.tolist()) == {0.0, 3.0}


# ---- 2: the empty set is the parent -------------------------------------------------------------------------------------------------
_STREAM_DIR = []


@pytest.fixture(scope='module')
def streaming_parents(tmp_path_factory):
    """sx_cem_rollout / sx_cem_rollout_elites forced to the streaming form on every case's inputs, in ONE fresh child process
    (the override is read when the library plans its first rollout).  The child is this file's __main__."""
    if not _STREAM_DIR:
        d = tmp_path_factory.mktemp('stream_cons')
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(d)], env=dict(os.environ, SX_ROLLOUT='stream'),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        _STREAM_DIR.append(d)
    return _STREAM_DIR[0]


def _streaming_child(d):
    """The parent entries (this process has SX_ROLLOUT=stream) on the inputs of every case, every output saved."""
    for n_s, n_u, N in CASES:
        ssm, envs = case(n_s, n_u, N)[:2]
        for H in STEPS:
            inp = inputs(n_s, n_u, SMALL, H, seed_of(n_s, n_u, N, H))
            form = int(_lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), H))
            for kind in KINDS:
                r = launch(ssm, envs[ABS], inp, H, kind)
                np.savez(os.path.join(d, f'{n_s}_{n_u}_{N}_{H}_{kind}.npz'), form=form,
                         **{name: N_(r[name]) for name in names_of(kind) + ('obj_cost',)})


@pytest.mark.parametrize('H', STEPS)
@pytest.mark.parametrize('n_s,n_u,N', CASES)
def test_the_empty_set_is_the_parent(streaming_parents, n_s, n_u, N, H):
    ssm, envs = case(n_s, n_u, N)[:2]
    cost, _ = cost_for(n_s)
    inp = inputs(n_s, n_u, SMALL, H, seed_of(n_s, n_u, N, H))
    lib = _lib.lib()
    form = int(lib.sx_cem_rollout_form(ctypes.byref(ssm.device_model), H))
    cons_form = int(lib.sx_cem_rollout_cons_form(ctypes.byref(ssm.device_model), H))
    assert cons_form == (SX_FORM_BYOUT if N == 590 else SX_FORM_STREAM)
    for kind in KINDS:
        label = f'({n_s},{n_u}) N={N} H={H} {kind} (parent form {form}, cons form {cons_form})'
        got = launch(ssm, envs[ABS], inp, H, kind, co.empty(n_s))
        assert int(got['status'].item()) == 0
        # the streaming parent, bit for bit, obj_cost and con_cost included
        parent = dict(np.load(os.path.join(streaming_parents, f'{n_s}_{n_u}_{N}_{H}_{kind}.npz')))
        assert int(parent['form']) == cons_form
        differ = [name for name in names_of(kind) + ('obj_cost',) if not np.array_equal(N_(got[name]), parent[name])]
        print(f'{label}: outputs that differ from the streaming parent: {differ}')
        assert not differ, label
        # the parent as this process runs it (a resident form where there is one)
        here = launch(ssm, envs[ABS], inp, H, kind)
        exact = form in (SX_FORM_STREAM, SX_FORM_BYOUT)
        assert_close_to_parent(label, here, got, kind, n_s, exact)
        print(f'{label}: obj_cost against the parent in its default form '
              f'{worst(got["obj_cost"], here["obj_cost"], rtol=RTOL, atol=ATOL):.3e} of the tolerance')
        np.testing.assert_allclose(N_(got['obj_cost']), N_(here['obj_cost']), rtol=RTOL, atol=ATOL)
        # with a cost: sx_cem_rollout[_elites]_sat, bit for bit
        sat, got = launch(ssm, envs[ABS], inp, H, kind, cost=cost), launch(ssm, envs[ABS], inp, H, kind, co.empty(n_s), cost)
        for name in names_of(kind) + ('obj_cost',):
            assert torch.equal(got[name], sat[name]), f'{label} with a cost: {name} differs from the _sat entry'


# ---- 3: a full set ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', STEPS)
@pytest.mark.parametrize('n_s,n_u,N', CASES)
def test_a_full_set_adds_the_oracles_cost_and_nothing_else(n_s, n_u, N, H):
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    cost, _ = cost_for(n_s)
    con = set_for(n_s)
    inp = inputs(n_s, n_u, SMALL, H, seed_of(n_s, n_u, N, H))
    fired = np.zeros(3, dtype=int)
    for use_cost in (None, cost):
        for kind in KINDS:
            label = f'({n_s},{n_u}) N={N} H={H} {kind} cost={"NULL" if use_cost is None else "sat"}'
            empty = launch(ssm, envs[ABS], inp, H, kind, co.empty(n_s), use_cost)
            full = launch(ssm, envs[ABS], inp, H, kind, con, use_cost)
            assert int(full['status'].item()) == 0
            for s in check_full_set(label, probs[ABS], con, empty, full, kind, n_s):
                fired += [int(s.box.sum()), int((s.ell & ~s.box).sum()), int(s.obs.sum())]
            # each half of the set alone
            for half in (co.ConSet(con.h_mat_obs, con.h_obs, False), co.ConSet(np.zeros((0, n_s)), np.zeros(0), True)):
                check_full_set(label + (' rows only' if len(half.h_obs) else ' feedback bounds only'), probs[ABS], half, empty,
                               launch(ssm, envs[ABS], inp, H, kind, half, use_cost), kind, n_s)
    print(f'({n_s},{n_u}) N={N} H={H}: violated steps over all launches: box {fired[0]}, ellipsoid only {fired[1]}, obstacle '
          f'{fired[2]}')
    assert fired[2] > 0 and (H < 15 or fired[1] > 0)


def test_the_main_case_through_the_kernel():
    """The oracle's main case (every signal fires for some particle and stays silent for another: tests/test_conset_host.py),
    as one given launch: con_cost is the parent's plus the oracle's extra cost, on the kernel's trajectory and on the oracle's."""
    spec, con, x0, rows, ref, sig = co.main_case()
    ssm, env = problems.build(spec, device=DEV)
    inp = dict(x0=x0[None], actions=rows[None])
    empty, full = launch(ssm, env, inp, co.H, 'given', co.empty(2)), launch(ssm, env, inp, co.H, 'given', con)
    s = check_full_set('pendulum main case', problems.oracle_problem(spec, ocem), con, empty, full, 'given', 2)[0]
    for name, fires in (('box', s.box.any(axis=1)), ('ellipsoid with the box satisfied', (s.ell & ~s.box).any(axis=1)),
                        ('obstacle', s.obs.any(axis=1))):
        print(f'pendulum main case: {name}: fires for {int(fires.sum())} of {len(fires)} particles')
        assert fires.any() and not fires.all(), name
    np.testing.assert_array_equal(N_(full['con_cost'][0]), ref.con_cost + sig.extra)
    np.testing.assert_array_equal(N_(empty['con_cost'][0]), ref.con_cost)


def test_a_full_set_at_4149_particles():
    n_s, n_u, N, H = 2, 1, 200, 3
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    con = set_for(n_s)
    inp = inputs(n_s, n_u, LARGE, H, seed_of(n_s, n_u, N, H))
    for kind in ('drawn', 'elites'):
        empty, full = launch(ssm, envs[ABS], inp, H, kind, co.empty(n_s)), launch(ssm, envs[ABS], inp, H, kind, con)
        check_full_set(f'P={LARGE} {kind}', probs[ABS], con, empty, full, kind, n_s)
    # a tile does not depend on the grid: the first 37 particles alone
    sub = dict(inp, noise=np.ascontiguousarray(inp['noise'][:, :SMALL]), actions=np.ascontiguousarray(inp['actions'][:, :SMALL]))
    small = launch(ssm, envs[ABS], sub, H, 'drawn', con)
    full = launch(ssm, envs[ABS], inp, H, 'drawn', con)
    for name in ('actions', 'traj', 'sigma', 'obj_cost', 'con_cost'):
        assert torch.equal(small[name], full[name][:, :SMALL]), name


@pytest.mark.parametrize('n_s,n_u,N,H', [(2, 1, 200, 3), (4, 1, 590, 3), (2, 2, 200, 15)])
def test_a_full_set_from_an_ellipsoid(n_s, n_u, N, H):
    """With a q0 the first step starts from an ellipsoid too: its control ellipsoid is checked."""
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    con = set_for(n_s)
    inp = inputs(n_s, n_u, SMALL, H, seed_of(n_s, n_u, N, H))
    a = np.random.default_rng(41 + n_s).normal(size=(E, n_s, n_s)) * 0.6
    q0 = a @ a.transpose(0, 2, 1) + 1e-4 * np.eye(n_s)
    first = 0
    for kind in KINDS:
        empty = launch(ssm, envs[ABS], inp, H, kind, co.empty(n_s), q0=q0)
        full = launch(ssm, envs[ABS], inp, H, kind, con, q0=q0)
        plain = launch(ssm, envs[ABS], inp, H, kind, q0=q0)
        assert torch.equal(empty['con_cost'], plain['con_cost'])
        for s in check_full_set(f'q0 ({n_s},{n_u}) N={N} H={H} {kind}', probs[ABS], con, empty, full, kind, n_s, q0):
            first += int((s.ell[:, 0] & ~s.box[:, 0]).sum())
    print(f'q0 ({n_s},{n_u}) N={N} H={H}: first steps ellipsoid-violated with the box satisfied: {first}')
    assert first > 0


# ---- 4: fused against step by step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', STEPS)
@pytest.mark.parametrize('n_s,n_u,N', CASES)
def test_fused_equals_stepwise(n_s, n_u, N, H):
    ssm, envs = case(n_s, n_u, N)[:2]
    cost, _ = cost_for(n_s)
    con = set_for(n_s)
    inp = inputs(n_s, n_u, SMALL, H, seed_of(n_s, n_u, N, H))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for use_cost in (None, cost):
        fused = launch(ssm, envs[ABS], inp, H, 'given', con, use_cost)
        plain = launch(ssm, envs[ABS], inp, H, 'given', co.empty(n_s), use_cost)
        for e in range(E):
            s = cem_mpc.cem_rollout_stepwise(ssm, envs[ABS], T(inp['x0'][e]), T(inp['actions'][e]), status=status,
                                             con_set=con.struct(n_s), **({} if use_cost is None else dict(cost=use_cost)))
            differ = int((s['con_cost'] != fused['con_cost'][e]).sum())
            added = int((fused['con_cost'][e] != plain['con_cost'][e]).sum())
            if use_cost is None:
                err = worst(s['obj_cost'], fused['obj_cost'][e], rtol=RTOL, atol=ATOL)
                print(f'({n_s},{n_u}) N={N} H={H} e={e}: fused against step by step, env objective {err:.3e} of the tolerance, '
                      f'constraint costs differ at {differ}; the set changes {added} of {SMALL} rows')
                np.testing.assert_allclose(N_(s['obj_cost']), N_(fused['obj_cost'][e]), rtol=RTOL, atol=ATOL)
            else:
                err = float((s['obj_cost'] - fused['obj_cost'][e]).abs().max())
                print(f'({n_s},{n_u}) N={N} H={H} e={e}: fused against step by step, saturating objective {err:.3e} '
                      f'(tolerance {LOSS_TOL * H:.1e}), constraint costs differ at {differ}')
                assert err <= LOSS_TOL * H
            assert torch.equal(s['con_cost'], fused['con_cost'][e])
            assert added > 0
    assert int(status.item()) == 0


# ---- 5: a solve -------------------------------------------------------------------------------------------------------------------------
def _rollout_entries(counting):
    return {k: v for k, v in counting.calls.items() if k.startswith('sx_cem_rollout') and not k.endswith(('_form', '_bytes'))}


def _elites(history, k):
    return [set(ocem.rank(N_(h.constraint_costs), N_(h.objective_costs), k)) for h in history]


def test_solve_matches_the_numpy_cem_and_differs_from_the_solve_without_the_set():
    """The inputs are those tests/test_conset_host.py checks on the CPU: every elite set is decided by more than 1e-6 and no
    distance sits within 1e-6 of the boundary.  This test fails without the feature: the same solve without the set selects
    other elites."""
    spec, con, H, x0, init_std, noise, ref_best, trace, plain_best, plain_trace = co.solve()
    ssm, env = problems.build(spec, device=DEV)
    mpc = cem_mpc.FusedCemMpc(ssm, env, H, co.P, co.K, co.ITERS, device=DEV, init_std=init_std, record_rollouts=True,
                              con_set=con.struct(2))
    counting = CountingLib(_lib.lib())
    with mock.patch.object(_lib, 'lib', lambda: counting):
        best, ok, history, status = mpc.solve(T(x0[None]), noise=T(noise[:, None]))
        torch.cuda.synchronize()
    print(f'rollout entries {_rollout_entries(counting)}')
    assert set(_rollout_entries(counting)) <= {'sx_cem_rollout_cons', 'sx_cem_rollout_elites_cons'}
    assert sum(_rollout_entries(counting).values()) == co.ITERS
    assert int(status.item()) == 0 and bool(ok[0].item())
    assert len(history) == len(trace)
    for it, (h, (cost, obj, idx, _)) in enumerate(zip(history, trace)):
        print(f'iteration {it}: objective {worst(h.objective_costs, obj, rtol=RTOL, atol=ATOL):.3e} of the tolerance, constraint '
              f'costs differ at {int((N_(h.constraint_costs) != cost).sum())}, {int((cost > 0).sum())} of {len(cost)} rows violate')
        np.testing.assert_array_equal(N_(h.constraint_costs), cost)
        np.testing.assert_allclose(N_(h.objective_costs), obj, rtol=RTOL, atol=ATOL)
        assert set(ocem.rank(N_(h.constraint_costs), N_(h.objective_costs), co.K)) == set(idx)
    print(f'best row: max |device - numpy CEM| = {float(np.abs(N_(best[0]) - ref_best).max()):.3e}')
    np.testing.assert_allclose(N_(best[0]), ref_best, rtol=0, atol=1e-9)
    # the same solve without the set: the numpy CEM without it, and another elite set in at least one iteration
    plain = cem_mpc.FusedCemMpc(ssm, env, H, co.P, co.K, co.ITERS, device=DEV, init_std=init_std, record_rollouts=True)
    pbest, pok, phistory, pstatus = plain.solve(T(x0[None]), noise=T(noise[:, None]))
    torch.cuda.synchronize()
    differ = [a != b for a, b in zip(_elites(history, co.K), _elites(phistory, co.K))]
    print(f'iterations whose elite set differs from the solve without the set: {differ}; best row without the set against its '
          f'numpy CEM {float(np.abs(N_(pbest[0]) - plain_best).max()):.3e}')
    assert any(differ)
    np.testing.assert_allclose(N_(pbest[0]), plain_best, rtol=0, atol=1e-9)
    # the step-by-step path carries the set: the same solve through it ends at the same row
    sbest, sok, _, sstatus = mpc.solve(T(x0[None]), noise=T(noise[:, None]), stepwise=True)
    torch.cuda.synchronize()
    print(f'step by step: best row against the numpy CEM {float(np.abs(N_(sbest[0]) - ref_best).max()):.3e}')
    assert int(sstatus.item()) == 0 and bool(sok[0].item())
    np.testing.assert_allclose(N_(sbest[0]), ref_best, rtol=0, atol=1e-9)


# ---- 6: CemSafeMPC through conf -----------------------------------------------------------------------------------------------------------
class Conf:
    mpc_time_horizon = co.H
    cem_num_rollouts = co.P
    cem_num_elites = co.K
    cem_num_iterations = co.ITERS
    cem_init_std = co.INIT_STD
    plot_cem_optimisation = False
    plot_cem_terminal_states = False
    device = DEV
    use_state_constraint = True
    use_prior_model = True
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'


def test_safempc_get_action_with_and_without_the_settings():
    from safe_exploration_amd.safempc_cem import MpcResult
    spec, con, H, x0, init_std, noise, ref_best, trace, plain_best, plain_trace = co.solve()
    opt_env = {'h_mat_obs': con.h_mat_obs, 'h_obs': con.h_obs[:, None]}
    target = float(spec.obj_target[1])

    def act(conf):
        env = problems.StubEnv(spec, np.zeros(2), objective_target=target)
        solver, _ = problems.make_solver(spec, conf, env, device=DEV, opt_env=opt_env)
        mpc = solver._solver()
        mpc._next_noise = lambda episodes: T(noise[:, None])      # the oracle's draws
        counting = CountingLib(_lib.lib())
        with mock.patch.object(_lib, 'lib', lambda: counting):
            action, result = solver.get_action(x0)
        return mpc, counting, np.asarray(action).reshape(-1), result

    on = type('C', (Conf,), dict(cem_ctrl_ellipsoid_constraint=True, cem_obstacle_constraint=True))()
    mpc, counting, action, result = act(on)
    rollouts = _rollout_entries(counting)
    print(f'settings on: rollout entries {rollouts}; action {action}, the numpy CEM\'s {ref_best[0]}')
    assert set(rollouts) <= {'sx_cem_rollout_cons', 'sx_cem_rollout_elites_cons'} and sum(rollouts.values()) == co.ITERS
    assert 'sx_conset_eval' not in counting.calls and 'sx_onestep_reach' not in counting.calls
    assert (mpc._con_set.m_obs, mpc._con_set.ctrl_ellipsoid) == (2, 1)
    assert result == MpcResult.FOUND_SOLUTION and mpc.last_status == 0
    np.testing.assert_allclose(action, ref_best[0], rtol=0, atol=1e-9)
    # with the settings absent it calls exactly what it calls today, whatever opt_env holds
    mpc, counting, action, result = act(Conf())
    rollouts = _rollout_entries(counting)
    print(f'settings absent: rollout entries {rollouts}; action {action}, the numpy CEM\'s {plain_best[0]}')
    assert set(rollouts) <= {'sx_cem_rollout', 'sx_cem_rollout_elites'} and sum(rollouts.values()) == co.ITERS
    assert mpc._con_set is None and 'sx_conset_eval' not in counting.calls
    assert result == MpcResult.FOUND_SOLUTION
    np.testing.assert_allclose(action, plain_best[0], rtol=0, atol=1e-9)


if __name__ == '__main__':
    _streaming_child(sys.argv[1])
