"""GPU: the SafeMPC constraint set in multi-model CEM solves ("the multi-model form") --
sx_cem_rollout_cons_multi / sx_cem_rollout_elites_cons_multi (cem_rollout_kernel<StreamCons<SAT, true>>) against the
single-model entries problem by problem, with the empty set against the multi-model parents, with a full set against the
empty-set launch plus the numpy oracle's extra cost of the kernel's own trajectory (tests/conset_oracle.py), with a NaN start
in one problem; the solve of tests/conset_multi_oracle.py through MultiModelConsCemMpc; and get_actions_multi over CemSafeMPCs
with the two conf settings.

Shapes: E = 3 problems with a GP each, P = 37 (three tiles per problem, the last one partial; the problem index of a
workgroup is blockIdx.x / 3); training sets of DIFFERENT sizes, so that a wrong table entry shows: (n_s, n_u, sizes) in
{(2,1,(7,200,100)), (4,1,(590,200,33): output by output for all because of the first), (2,2,(200,100,7)),
(4,2,(200,100,33))} at H = 3 and 15, (3,1,(200,100,7)) and (1,1,(200,100,7)) at H = 3; the given, drawn and elite-row
forms; cost = NULL and a SaturatingCost (cost_for of tests/test_gpu_conset.py).  The full set is set_for of that file.

Comparisons.  Problem e of a launch against sx_cem_rollout[_elites]_cons of model e alone: every output bit for bit where
sx_cem_rollout_cons_form(model e) is the launch's form; where the launch is output by output and the model alone is not, within
TOL['rbf'] of tests/test_gpu_rollout_matrix.py (the bound the two forms of one model are held to there), con_cost exactly.  The
empty set: bit-equal to sx_cem_rollout[_elites]_multi, with a cost to the _sat_multi entries.  A full set: check_full_set of
tests/test_gpu_conset.py per problem -- everything but con_cost carries the empty-set launch's bits, con_cost is the empty-set
launch's plus the oracle's extra cost, exactly, after asserting that no distance of the oracle sits within MARGIN = 1e-6 of the
boundary.  The solve: constraint costs exactly, equal elite sets in every iteration, best row within 1e-9 of the numpy CEM (the
single-model solve test's tolerance, where 8e-17 was measured); against FusedCemMpc(con_set=...).solve of each model alone bit
for bit where the forms agree.  The public surface: actions within 1e-12 of two get_action calls.
Every case prints its figures before it asserts."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import conset_multi_oracle as cmo
import conset_oracle as co
import test_gpu_perf_multi as multi
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc, problems
from test_gpu_conset import Conf, _rollout_entries, check_full_set, cost_for, set_for
from test_gpu_junk_fused import CountingLib
from test_gpu_perf_var import ABS, DEV, N_, T, worst
from test_gpu_rollout_matrix import TOL
from test_gpu_safety_sat import KINDS, K_ELITES, assert_close_to_parent, names_of, seed_of

pytestmark = pytest.mark.gpu
E, SMALL = 3, 37
CASES = [(2, 1, (7, 200, 100)), (4, 1, (590, 200, 33)), (2, 2, (200, 100, 7)), (4, 2, (200, 100, 33))]
SHORT_CASES = [(3, 1, (200, 100, 7)), (1, 1, (200, 100, 7))]          # H = 3 only
CASES_STEPS = [(n_s, n_u, sizes, H) for n_s, n_u, sizes in CASES for H in (3, 15)] + [c + (3,) for c in SHORT_CASES]
RTOL_P, RTOL, ATOL = TOL['rbf']
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
MULTI_ENTRIES = ('sx_cem_rollout_cons_multi', 'sx_cem_rollout_elites_cons_multi')
_INPUTS = {}


def inputs(n_s, n_u, H, seed, P=SMALL):
    """x0 [E x n_s], the distribution, the draws and the rows they give, and elite rows [E x k x (2 + H n_u)]; computed once."""
    key = (n_s, n_u, H, seed, P)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        x0 = rng.normal(0, 0.05, size=(E, n_s))
        mean, std = rng.normal(0, 0.2, size=(E, H, n_u)), rng.uniform(0.3, 0.8, size=(E, H, n_u))
        noise = rng.normal(size=(E, P, H, n_u))
        elite = np.concatenate((np.zeros((E, K_ELITES, 2)), rng.normal(0, 0.5, size=(E, K_ELITES, H * n_u))), axis=2)
        _INPUTS[key] = dict(x0=x0, mean=mean, std=std, noise=noise, actions=mean[:, None] + std[:, None] * noise, elite=elite)
    return _INPUTS[key]


def seed_for(n_s, n_u, sizes, H):
    """The seed of a case's inputs.  (The offset is chosen on the oracle alone, oracle.cem.rollout of these inputs over the
    cases' GPs: no control or obstacle distance of any case then sits within 1e-5 of the boundary -- ten times MARGIN, which
    check_full_set asserts on the kernel's own trajectory; smallest 1.7e-5.  Without the offset the (4,1) H = 15 elite-row
    case has one at 5.8e-7.)"""
    return seed_of(n_s, n_u, sizes, H) + 5000


def only(inp, e):
    """The inputs of problem e alone."""
    return {name: np.ascontiguousarray(v[e:e + 1]) for name, v in inp.items()}


def launch(models, env, inp, H, kind, con=None, cost=None, q0=None):
    """One rollout: `models` a list of GpCemSSMs (the _multi entries, a status word per problem) or one (the single-model
    entries); `con` a conset_oracle.ConSet or None (the parent entry)."""
    many = isinstance(models, (list, tuple))
    fn = cem_mpc.cem_rollout_multi if many else cem_mpc.cem_rollout
    n_s = (models[0] if many else models).num_states
    kw = dict(want_traj=True, want_sigma=True, **({} if cost is None else dict(cost=cost)),
              **({} if con is None else dict(con_set=con.struct(n_s))), **({} if q0 is None else dict(q0=T(q0))))
    if many:
        kw.update(status=torch.zeros(len(models), dtype=torch.int32, device=DEV))
    if kind == 'given':
        kw.update(actions=T(inp['actions']))
    elif kind == 'drawn':
        kw.update(mean=T(inp['mean']), std=T(inp['std']), noise=T(inp['noise']))
    else:
        kw.update(elite_rows=T(inp['elite']), noise=T(inp['noise']), want_dist=True)
    out = fn(models, env, T(inp['x0']), H, **kw)
    torch.cuda.synchronize()
    return out


def forms(ssms, H):
    """(the form of the multi-model launch, the form of every model alone)."""
    lib = _lib.lib()
    models = cem_mpc.model_array(ssms, 'rbf')
    return (int(lib.sx_cem_rollout_cons_multi_form(models, len(ssms), H)),
            [int(lib.sx_cem_rollout_cons_form(ctypes.byref(s.device_model), H)) for s in ssms])


def problem_of(out, e):
    """Problem e of a multi-model launch, shaped like a single-model launch of it."""
    return {name: None if v is None else v[e:e + 1] for name, v in out.items()}


# ---- 1: against the single-model kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,sizes,H', CASES_STEPS)
def test_problem_e_is_the_single_model_launch_of_model_e(n_s, n_u, sizes, H):
    ssms, envs = multi.case(n_s, n_u, sizes)[:2]
    cost, _ = cost_for(n_s)
    con = set_for(n_s)
    inp = inputs(n_s, n_u, H, seed_for(n_s, n_u, sizes, H))
    form, alone = forms(ssms, H)
    want_form = SX_FORM_BYOUT if max(sizes) == 590 else SX_FORM_STREAM
    print(f'({n_s},{n_u}) N={sizes} H={H}: the launch has form {form}, the models alone {alone}')
    assert form == want_form and alone == [SX_FORM_BYOUT if N == 590 else SX_FORM_STREAM for N in sizes]
    for use_cost in (None, cost):
        for kind in KINDS:
            got = launch(ssms, envs[ABS], inp, H, kind, con, use_cost)
            assert got['status'].tolist() == [0] * E
            for e in range(E):
                label = f'({n_s},{n_u}) N={sizes} H={H} {kind} cost={"NULL" if use_cost is None else "sat"} e={e}'
                one, mine = launch(ssms[e], envs[ABS], only(inp, e), H, kind, con, use_cost), problem_of(got, e)
                exact = alone[e] == form
                differ = [name for name in names_of(kind) + ('obj_cost',) if not torch.equal(mine[name], one[name])]
                print(f'{label}: forms {"agree" if exact else "differ"}; outputs that differ from the model alone: {differ}; '
                      f'obj_cost {worst(mine["obj_cost"], one["obj_cost"], rtol=RTOL, atol=ATOL):.3e} of the tolerance, con_cost '
                      f'differs at {int((mine["con_cost"] != one["con_cost"]).sum())} of {SMALL} rows')
                if exact:
                    assert not differ, label
                else:
                    assert_close_to_parent(label, one, mine, kind, n_s, False)      # con_cost and status exactly
                    np.testing.assert_allclose(N_(mine['obj_cost']), N_(one['obj_cost']), rtol=RTOL, atol=ATOL, err_msg=label)


# ---- 2: the empty set is the multi-model parent ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,sizes,H', CASES_STEPS)
def test_the_empty_set_is_the_multi_model_parent(n_s, n_u, sizes, H):
    ssms, envs = multi.case(n_s, n_u, sizes)[:2]
    cost, _ = cost_for(n_s)
    inp = inputs(n_s, n_u, H, seed_for(n_s, n_u, sizes, H))
    for use_cost in (None, cost):
        for kind in KINDS:
            label = f'({n_s},{n_u}) N={sizes} H={H} {kind} cost={"NULL" if use_cost is None else "sat"}'
            parent = launch(ssms, envs[ABS], inp, H, kind, None, use_cost)
            got = launch(ssms, envs[ABS], inp, H, kind, co.empty(n_s), use_cost)
            differ = [name for name in names_of(kind) + ('obj_cost',) if not torch.equal(got[name], parent[name])]
            print(f'{label}: outputs that differ from sx_cem_rollout{"_elites" if kind == "elites" else ""}'
                  f'{"_sat" if use_cost is not None else ""}_multi: {differ}')
            assert got['status'].tolist() == [0] * E
            assert not differ, label


# ---- 3: a full set against the oracle ------------------------------------------------------------------------------------------------------
def start_shapes(n_s):
    """A different q0 per problem."""
    a = np.random.default_rng(43 + n_s).normal(size=(E, n_s, n_s)) * np.array([0.3, 0.6, 0.9])[:, None, None]
    return a @ a.transpose(0, 2, 1) + 1e-4 * np.eye(n_s)


@pytest.mark.parametrize('n_s,n_u,sizes,H', CASES_STEPS)
def test_a_full_set_adds_the_oracles_cost_per_problem_and_nothing_else(n_s, n_u, sizes, H):
    ssms, envs, gps, probs = multi.case(n_s, n_u, sizes)
    cost, _ = cost_for(n_s)
    con = set_for(n_s)
    inp = inputs(n_s, n_u, H, seed_for(n_s, n_u, sizes, H))
    # (from points, and for the cases of one horizon from an ellipsoid of its own per problem)
    starts = [None] + ([start_shapes(n_s)] if H == 3 else [])
    fired = np.zeros(3, dtype=int)
    first = 0
    for q0 in starts:
        for use_cost in (None, cost):
            for kind in KINDS:
                label = (f'({n_s},{n_u}) N={sizes} H={H} {kind} cost={"NULL" if use_cost is None else "sat"} '
                         f'{"from points" if q0 is None else "q0 per problem"}')
                empty = launch(ssms, envs[ABS], inp, H, kind, co.empty(n_s), use_cost, q0)
                full = launch(ssms, envs[ABS], inp, H, kind, con, use_cost, q0)
                assert full['status'].tolist() == [0] * E
                for s in check_full_set(label, probs[ABS], con, empty, full, kind, n_s, q0):
                    fired += [int(s.box.sum()), int((s.ell & ~s.box).sum()), int(s.obs.sum())]
                    if q0 is not None:
                        first += int((s.ell[:, 0] & ~s.box[:, 0]).sum())
    print(f'({n_s},{n_u}) N={sizes} H={H}: violated steps over all launches: box {fired[0]}, ellipsoid only {fired[1]}, obstacle '
          f'{fired[2]}; first steps ellipsoid-violated with the box satisfied (q0 given) {first}')
    assert fired[2] > 0 and (H < 15 or fired[1] > 0)
    # (the q0 launches exercise the first step's control ellipsoid; at (1,1) the given rows of these inputs have no such step)
    assert H != 3 or n_s == 1 or first > 0


# ---- 4: one problem's trouble is its own -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,sizes,H', [(2, 1, (7, 200, 100), 3), (4, 1, (590, 200, 33), 3)])
def test_a_nan_start_is_its_problems_alone(n_s, n_u, sizes, H):
    ssms, envs = multi.case(n_s, n_u, sizes)[:2]
    cost, _ = cost_for(n_s)
    con = set_for(n_s)
    inp = inputs(n_s, n_u, H, seed_for(n_s, n_u, sizes, H))
    bad = dict(inp, x0=inp['x0'].copy())
    bad['x0'][1, n_s - 1] = np.nan
    for use_cost in (None, cost):
        for kind in ('drawn', 'elites'):
            good, nan = launch(ssms, envs[ABS], inp, H, kind, con, use_cost), launch(ssms, envs[ABS], bad, H, kind, con, use_cost)
            print(f'({n_s},{n_u}) N={sizes} {kind} cost={"NULL" if use_cost is None else "sat"}: status words {nan["status"].tolist()} '
                  f'(clean launch {good["status"].tolist()})')
            assert good['status'].tolist() == [0] * E
            assert nan['status'][1].item() & _lib.SX_STATUS_NAN
            assert nan['status'][0].item() == 0 and nan['status'][2].item() == 0
            for e in (0, 2):
                for name in ('actions', 'traj', 'sigma', 'obj_cost', 'con_cost'):
                    assert torch.equal(nan[name][e], good[name][e]), (name, e)
            if use_cost is not None:
                assert bool(torch.isnan(nan['obj_cost'][1]).all())


# ---- 5: the multi solve ------------------------------------------------------------------------------------------------------------------------
def _recording_rank(record):
    """cem_rank_refit_any, keeping the costs it was handed."""
    real = cem_mpc.cem_rank_refit_any

    def rank(con, obj, actions, k, **kw):
        record.append((N_(con).copy(), N_(obj).copy()))
        return real(con, obj, actions, k, **kw)
    return rank


def _elite_sets(record, e):
    return [set(ocem.rank(con[e], obj[e], co.K)) for con, obj in record]


def test_multi_solve_matches_the_numpy_cems_and_the_solves_of_each_model_alone():
    """The inputs are those tests/test_conset_multi_host.py checks on the CPU: per problem every elite set is decided by more
    than 1e-6 (smallest gap 6.65e-5) and no distance sits within 1e-6 of the boundary (smallest |d| 2.41e-5).  This test fails
    without the feature: the same solve without the set selects other elites."""
    solves = cmo.solves()
    H, init_std, con = solves[0][2], solves[0][4], solves[0][1]
    built = [problems.build(s[0], device=DEV) for s in solves]
    assert all(bytes(b[1]) == bytes(built[0][1]) for b in built)
    ssms, env = [b[0] for b in built], built[0][1]
    mk = lambda e, **kw: cem_mpc.FusedCemMpc(ssms[e], env, H, co.P, co.K, co.ITERS, device=DEV, init_std=init_std, seed=e, **kw)
    mpc = cem_mpc.MultiModelConsCemMpc.from_solvers([mk(e, con_set=con.struct(2)) for e in range(cmo.E)])
    assert mpc.fused_applies()
    x0 = np.stack([s[3] for s in solves])
    noise = np.stack([s[5] for s in solves], axis=1)
    counting, record = CountingLib(_lib.lib()), []
    with mock.patch.object(_lib, 'lib', lambda: counting), mock.patch.object(cem_mpc, 'cem_rank_refit_any', _recording_rank(record)):
        best, ok, status = mpc.solve(T(x0), noise=T(noise))
        torch.cuda.synchronize()
    rollouts = _rollout_entries(counting)
    print(f'rollout entries {rollouts}')
    assert set(rollouts) <= set(MULTI_ENTRIES) and sum(rollouts.values()) == co.ITERS
    assert status.tolist() == [0] * cmo.E and ok.tolist() == [1] * cmo.E
    assert len(record) == co.ITERS
    for e, s in enumerate(solves):
        ref_best, trace = s[6], s[7]
        for it, ((con_all, obj_all), (cost, obj, idx, _)) in enumerate(zip(record, trace)):
            print(f'problem {e} iteration {it}: objective {worst(obj_all[e], obj, rtol=RTOL, atol=ATOL):.3e} of the tolerance, '
                  f'constraint costs differ at {int((con_all[e] != cost).sum())}, {int((cost > 0).sum())} of {len(cost)} rows violate')
            np.testing.assert_array_equal(con_all[e], cost)
            np.testing.assert_allclose(obj_all[e], obj, rtol=RTOL, atol=ATOL)
            assert set(ocem.rank(con_all[e], obj_all[e], co.K)) == set(idx)
        print(f'problem {e}: best row: max |device - numpy CEM| = {float(np.abs(N_(best[e]) - ref_best).max()):.3e}')
        np.testing.assert_allclose(N_(best[e]), ref_best, rtol=0, atol=1e-9)
    # each model alone, with the same noise: the same bits where the forms agree (they do: streaming for every model)
    form, alone = forms(ssms, H)
    for e in range(cmo.E):
        single = mk(e, con_set=con.struct(2))
        sbest, sok, _, sstatus = single.solve(T(x0[e:e + 1]), noise=T(noise[:, e:e + 1]))
        torch.cuda.synchronize()
        err = float((sbest[0] - best[e]).abs().max())
        print(f'problem {e}: best row against FusedCemMpc(con_set=...).solve of the model alone: {err:.3e} (forms {alone[e]} / {form})')
        assert int(sstatus.item()) == 0 and bool(sok[0].item())
        assert alone[e] == form
        assert torch.equal(sbest[0], best[e])
    # the same multi solve without the set: other elites in at least one iteration of every problem
    plain = cem_mpc.MultiModelCemMpc.from_solvers([mk(e) for e in range(cmo.E)])
    precord = []
    with mock.patch.object(cem_mpc, 'cem_rank_refit_any', _recording_rank(precord)):
        pbest, pok, pstatus = plain.solve(T(x0), noise=T(noise))
        torch.cuda.synchronize()
    for e, s in enumerate(solves):
        differ = [a != b for a, b in zip(_elite_sets(record, e), _elite_sets(precord, e))]
        print(f'problem {e}: iterations whose elite set differs from the solve without the set: {differ}; best row without the '
              f'set against its numpy CEM {float(np.abs(N_(pbest[e]) - s[8]).max()):.3e}')
        assert any(differ)
        np.testing.assert_allclose(N_(pbest[e]), s[8], rtol=0, atol=1e-9)


# ---- 6: through the public surface ---------------------------------------------------------------------------------------------------------------
def test_get_actions_multi_with_and_without_the_settings():
    from safe_exploration_amd.safempc_cem import MpcResult, get_actions_multi
    solves = cmo.solves()[:2]
    con = solves[0][1]
    opt_env = {'h_mat_obs': con.h_mat_obs, 'h_obs': con.h_obs[:, None]}
    target = float(solves[0][0].obj_target[1])
    x0 = np.stack([s[3] for s in solves])

    def solvers(settings):
        out = []
        for e, s in enumerate(solves):
            c = type('C', (Conf,), dict(settings, cem_seed=e))()
            env = problems.StubEnv(s[0], np.zeros(2), objective_target=target)
            out.append(problems.make_solver(s[0], c, env, device=DEV, opt_env=opt_env)[0])
        return out

    def act_together(settings):
        group = solvers(settings)
        counting = CountingLib(_lib.lib())
        with mock.patch.object(_lib, 'lib', lambda: counting):
            actions, results = get_actions_multi(group, x0)
        return group, counting, np.asarray(actions), results

    on = dict(cem_ctrl_ellipsoid_constraint=True, cem_obstacle_constraint=True)
    group, counting, actions, results = act_together(on)
    rollouts = _rollout_entries(counting)
    print(f'settings on: rollout entries {rollouts}; actions {actions.reshape(-1)}')
    assert isinstance(group[0]._multi[1], cem_mpc.MultiModelConsCemMpc) and group[0]._multi[1].per_model_solves == 0
    assert set(rollouts) <= set(MULTI_ENTRIES) and sum(rollouts.values()) == co.ITERS       # one launch per iteration for both
    assert 'sx_conset_eval' not in counting.calls and 'sx_onestep_reach' not in counting.calls
    assert all(r == MpcResult.FOUND_SOLUTION for r in results)
    # two get_action calls on fresh solvers with the same seeds: what a user had to do before
    for e, fresh in enumerate(solvers(on)):
        action, result = fresh.get_action(x0[e])
        err = float(np.abs(np.asarray(action).reshape(-1) - actions[e].reshape(-1)).max())
        print(f'solver {e}: get_actions_multi against get_action on a fresh solver: {err:.3e}')
        assert result == MpcResult.FOUND_SOLUTION
        assert err <= 1e-12
    # the same list with the settings off calls sx_cem_rollout_multi, as before
    group, counting, plain_actions, results = act_together({})
    rollouts = _rollout_entries(counting)
    print(f'settings off: rollout entries {rollouts}; actions {plain_actions.reshape(-1)}')
    assert type(group[0]._multi[1]) is cem_mpc.MultiModelCemMpc
    assert set(rollouts) <= {'sx_cem_rollout_multi', 'sx_cem_rollout_elites_multi'} and sum(rollouts.values()) == co.ITERS
    assert all(s._con_set is None for s in group) and 'sx_conset_eval' not in counting.calls
