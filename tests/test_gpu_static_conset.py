"""GPU: the SafeMPC constraint set in static exploration ("the constraint set") --
sx_cem_rollout_starts_cons (cem_rollout_kernel<StreamStartsCons>) with the empty set against sx_cem_rollout_starts, bit for bit;
with a full set against the empty-set launch plus the oracle's extra cost of the kernel's own trajectory and starts
(tests/static_conset_oracle.py); against the oracle's rollout from every row's own start; its independence of the particle
count; the fused rollout against StaticCemMpc._rollout_stepwise; the solve of the oracle file through
StaticCemMpc(con_set=...); and StaticSafeMPCExploration over a CemSafeMPC with the two static settings.

Shapes: those of tests/test_gpu_static_explore.py and its inputs -- every (n_s, n_u) of {(1,1), (2,1), (2,2), (3,1), (4,1),
(4,2)} with N = 33, P = 37 (three tiles, the last one partial), E = 2 with a distribution each, H = 3 -- plus a (4,1) model
with N = 590 (output by output), and at (2,1) one case with H = 1 (only the start test and the box apply), one with H = 15 and
one with P = 4149.  The set of a case: the feedback bounds, and two obstacle rows +-e_0 cut through the oracle's starts and
intermediate ellipsoids of the very rows that are checked, half-way between two support values at least 4e-6 apart; the
bound of the last action component is moved so that some step is ellipsoid-violated with the box satisfied (the synthetic
models' ellipsoids are small: sqrt(K Q K^T) ~ 1e-3).

Tolerances: TOL['rbf'] of tests/test_gpu_rollout_matrix.py on objectives; rtol 1e-8 / atol 1e-11 on trajectories against the
oracle; constraint costs exactly, which is sound because no distance of the inputs sits within 1e-6 of the boundary (asserted
on the oracle's numbers in every case); 1e-9 absolute on a solve's best row.  Every figure is printed before it is asserted."""
import ctypes
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import conset_oracle as co
import static_conset_oracle as sco
import static_explore_oracle as seo
import test_gpu_rollout_matrix as rm
import test_gpu_static_explore as gse
from oracle import cases
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc, problems
from test_gpu_junk_fused import CountingLib
from test_gpu_rollout_matrix import DEV, TOL, T

pytestmark = pytest.mark.gpu
E, P, H = gse.E, gse.P, gse.H
LARGE = 4149
VAR, ALL_STATES = gse.VAR, gse.ALL_STATES
RTOL_P, RTOL, ATOL = TOL['rbf']
SX_FORM_BYOUT = 3
gse.SHAPES.setdefault('byout590', (4, 1, 590))      # the output-by-output model of tests/test_gpu_conset.py
# name -> (the model and system of this case of tests/test_gpu_static_explore.py, H, P)
CASES = {'1x1': ('1x1', H, P), '2x1': ('2x1', H, P), '2x2': ('2x2', H, P), '3x1': ('3x1', H, P), '4x1': ('4x1', H, P),
         '4x2': ('4x2', H, P), 'byout590': ('byout590', H, P), 'H1': ('2x1', 1, P), 'H15': ('2x1', 15, P),
         'P4149': ('2x1', H, LARGE)}
NAMES = list(CASES)
N_ = lambda t: t.detach().cpu().numpy()


class Inputs:
    """One case, computed once on the CPU and left unchanged: the model's name, H, P, the constraints of the parent case, the
    distribution and the draws, the rows, the set, and per problem the oracle's rollout with the set."""


def _cut(values, crossing, quantile):
    """An offset half-way between two adjacent values at least 4e-6 apart, as close as there is to `quantile` of `crossing`."""
    v = np.unique(values[np.isfinite(values)])
    mid, gap = 0.5 * (v[:-1] + v[1:]), v[1:] - v[:-1]
    mid = mid[gap > 4e-6 * (1.0 + np.abs(mid))]
    return float(mid[np.argmin(np.abs(mid - np.quantile(crossing, quantile)))])


def obstacle_rows(n_s, starts, traj_p, traj_q):
    """The obstacle slab of a case: +e_0 cut at the 0.8 quantile of the starts' supports, -e_0 at the 0.85 quantile of the
    intermediate ellipsoids' (of the starts' for H = 1), both clear of every support value of a start or such an ellipsoid."""
    e0 = np.eye(n_s)[0]
    h_obs = []
    for sign, quantile, of_starts in ((1.0, 0.8, True), (-1.0, 0.85, False)):
        s0 = starts @ (sign * e0)
        s1 = cases.support(traj_p, traj_q, sign * e0).ravel() if traj_p.shape[1] else s0
        h_obs.append(_cut(np.concatenate((s0, s1)), s0 if of_starts else s1, quantile))
    return co.ConSet(np.vstack((e0, -e0)), np.array(h_obs), True)


def action_bound(prob, rows, plain, bound):
    """The action box of a case: that of the parent case with the bound of the last action component moved, as little as can
    be, to |u| + sqrt(Q_u) / 2 of some step t >= 1 of some row (Q_u = K Q_t K^T in that component), so that this step is
    ellipsoid-violated with the box satisfied, with every |u| and every |u| + sqrt(Q_u) at least 2e-6 away from the bound.
    (The trajectories do not depend on the box.)"""
    k_fb = np.asarray(prob.k_fb, dtype=np.float64).reshape(prob.n_u, prob.n_s)
    a, r = [], []
    for e, res in enumerate(plain):
        u = np.abs(seo.split(prob, rows[e])[1][:, 1:, -1])                                          # [P x (H - 1)]
        a.append(u.ravel())
        r.append(np.sqrt(np.einsum('i,ptij,j->pt', k_fb[-1], res.traj_q[:, :-1], k_fb[-1])).ravel())
    a, r = np.concatenate(a), np.concatenate(r)
    first = np.concatenate([np.abs(seo.split(prob, rows[e])[1][:, 0, -1]) for e in range(len(plain))])
    edges = np.concatenate((a, a + r, first))
    for j in np.argsort(np.abs(a + 0.5 * r - bound[-1])):
        b = a[j] + 0.5 * r[j]
        if np.isfinite(b) and r[j] > 1e-5 and np.abs(edges - b).min() > 2e-6:
            out = bound.copy()
            out[-1] = b
            return out
    raise AssertionError('no step can be made ellipsoid-violated with the box satisfied')


@functools.lru_cache(maxsize=None)
def inputs(name):
    model, Hn, Pn = CASES[name]
    c = gse.case(model)
    i = Inputs()
    i.model, i.H, i.P, i.n_s, i.n_u, i.gp, i.con = model, Hn, Pn, c.n_s, c.n_u, c.gp, c.con
    L = c.n_s + Hn * c.n_u
    if Hn == H:
        i.mean, i.std, i.noise = c.mean, c.std, c.noise
        if Pn > P:
            extra = np.random.default_rng(3).normal(size=(E, Pn - P, L))
            i.noise = np.concatenate((c.noise, extra), axis=1)
    else:
        rng = np.random.default_rng(70 + Hn)
        i.mean = np.concatenate((rng.normal(0, 0.05, size=(E, c.n_s)), rng.normal(0, 0.1, size=(E, Hn * c.n_u))), axis=1)
        i.std = np.concatenate((rng.uniform(0.1, 0.25, size=(E, c.n_s)), rng.uniform(0.2, 0.5, size=(E, Hn * c.n_u))), axis=1)
        i.noise = rng.normal(size=(E, Pn, L))
    i.rows = i.mean[:, None] + i.std[:, None] * i.noise
    plain = [seo.rollout(c.con.problem(VAR, ALL_STATES), c.gp, i.rows[e]) for e in range(E)]
    if Hn > 1:
        bound = action_bound(c.con.problem(VAR, ALL_STATES), i.rows, plain, c.con.u_max)
        i.con = rm.Constraints(c.sysd, c.con.h_mat, c.con.h_vec, -bound, bound.copy())
    i.prob = i.con.problem(VAR, ALL_STATES)
    plain = [seo.rollout(i.prob, c.gp, i.rows[e]) for e in range(E)]
    i.set = obstacle_rows(c.n_s, i.rows[:, :, :c.n_s].reshape(E * Pn, c.n_s),
                          np.concatenate([r.traj_p[:, :Hn - 1] for r in plain]),
                          np.concatenate([r.traj_q[:, :Hn - 1] for r in plain]))
    i.refs = [sco.rollout(i.prob, i.set, c.gp, i.rows[e]) for e in range(E)]
    i.plain = plain
    return i


def env_of(i):
    return i.con.env(VAR, ALL_STATES)


def launch(i, con=None, kind='drawn', rows=None, first=None):
    """sx_cem_rollout_starts (con None) or sx_cem_rollout_starts_cons on the case's draws (`first`: of its first particles
    only) or on given rows."""
    kw = dict(want_traj=True, want_sigma=True, **({} if con is None else dict(con_set=con.struct(i.n_s))))
    if kind == 'drawn':
        noise = i.noise if first is None else np.ascontiguousarray(i.noise[:, :first])
        kw.update(mean=T(i.mean), std=T(i.std), noise=T(noise))
    else:
        kw.update(rows=rows.clone())
    out = cem_mpc.cem_rollout_starts(gse.device_model(i.model), env_of(i), i.H, **kw)
    torch.cuda.synchronize()
    return out


KEYS = ('rows', 'traj', 'sigma', 'obj_cost', 'con_cost', 'status')


def differing(a, b, keys=KEYS, first=None):
    cut = lambda t: t if first is None or t.dim() < 2 else t[:, :first]
    return [k for k in keys if not torch.equal(cut(a[k]), cut(b[k]))]


def counts(i):
    """(starts that violate the obstacle rows inside the safe polytope, rows with a step ellipsoid-violated with the box
    satisfied, rows with an obstacle-violated ellipsoid, feasible rows, smallest |d| to the set, to the safe polytope), on the
    oracle's numbers."""
    start = ell = obs = feasible = 0
    margin = poly = np.inf
    for e in range(E):
        r, s = i.refs[e], i.refs[e].signals
        start += int((r.start_obs & (i.plain[e].start_cost == 0)).sum())
        ell += int((s.ell & ~s.box).any(axis=1).sum())
        obs += int(s.obs.any(axis=1).sum())
        feasible += int((r.con_cost == 0).sum())
        margin, poly = min(margin, r.min_abs_d), min(poly, sco.polytope_margin(i.prob, i.rows[e], r))
    return start, ell, obs, feasible, margin, poly


def assert_sound(name, i):
    start, ell, obs, feasible, margin, poly = counts(i)
    print(f'{name}: oracle: starts obstacle-violated inside the safe polytope {start}, rows ellipsoid-violated with the box '
          f'satisfied {ell}, obstacle-violated {obs}, feasible {feasible} of {E * i.P}; smallest |d| {margin:.2e}, to the safe '
          f'polytope {poly:.2e}')
    assert margin >= sco.MARGIN and poly >= sco.MARGIN, 'a distance sits at the boundary: the exact comparison is not sound'
    assert start > 0 and (feasible > 0 or i.H == 15)
    assert obs > 0 or i.H == 1
    assert ell > 0 or i.H == 1


# ---- 1: the empty set is the parent ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_the_empty_set_is_the_parent(name):
    i = inputs(name)
    form = int(_lib.lib().sx_cem_rollout_starts_form(ctypes.byref(gse.device_model(i.model).device_model), i.H))
    assert form == (SX_FORM_BYOUT if name == 'byout590' else 0)
    parent = launch(i)
    got = launch(i, co.empty(i.n_s))
    differ = differing(got, parent)
    print(f'{name} (form {form}) drawn: outputs that differ from sx_cem_rollout_starts: {differ}')
    assert not differ
    given_parent = launch(i, kind='given', rows=parent['rows'])
    given = launch(i, co.empty(i.n_s), kind='given', rows=parent['rows'])
    differ = differing(given, given_parent) + differing(given, parent)
    print(f'{name} (form {form}) given rows: outputs that differ from sx_cem_rollout_starts, or from the drawn form: {differ}')
    assert not differ


# ---- 2: a full set adds the oracle's cost and nothing else ----------------------------------------------------------------------------
def check_full_set(label, i, con, empty, full):
    differ = differing(full, empty, keys=('rows', 'traj', 'sigma', 'obj_cost', 'status'))
    assert not differ, f'{label}: {differ} differ from the empty-set launch'
    fired = np.zeros(3, dtype=int)
    for e in range(E):
        traj = N_(full['traj'][e])
        tp, tq = traj[..., :i.n_s], traj[..., i.n_s:].reshape(i.P, i.H, i.n_s, i.n_s)
        extra, smallest, s, start_obs = sco.extra_of(i.prob, con, tp, tq, N_(full['rows'][e]))
        got, want = N_(full['con_cost'][e]), N_(empty['con_cost'][e]) + extra
        print(f'{label} e={e}: con_cost differs from empty + oracle at {int((got != want).sum())} of {len(got)} rows; starts '
              f'obstacle-violated {int(start_obs.sum())}, steps ellipsoid-violated with the box satisfied '
              f'{int((s.ell & ~s.box).sum())}, obstacle-violated {int(s.obs.sum())}; smallest |d| {smallest:.2e}')
        assert smallest >= sco.MARGIN, f'{label}: a distance sits at the boundary: the exact comparison is not sound'
        np.testing.assert_array_equal(got, want, err_msg=label)
        fired += [int(start_obs.sum()), int((s.ell & ~s.box).sum()), int(s.obs.sum())]
    return fired


@pytest.mark.parametrize('name', NAMES)
def test_a_full_set_adds_the_oracles_cost_and_nothing_else(name):
    i = inputs(name)
    assert_sound(name, i)
    empty = launch(i, co.empty(i.n_s))
    fired = check_full_set(name, i, i.set, empty, launch(i, i.set))
    assert fired[0] > 0 and (i.H == 1 or (fired[1] > 0 and fired[2] > 0))
    # each half of the set alone
    rows_only, bounds_only = co.ConSet(i.set.h_mat_obs, i.set.h_obs, False), co.ConSet(np.zeros((0, i.n_s)), np.zeros(0), True)
    half = check_full_set(name + ' rows only', i, rows_only, empty, launch(i, rows_only))
    assert half[1] == 0 and half[0] == fired[0] and half[2] == fired[2]
    half = check_full_set(name + ' feedback bounds only', i, bounds_only, empty, launch(i, bounds_only))
    assert half[0] == 0 and half[2] == 0 and half[1] == fired[1]
    if i.H == 1:
        # only the start test and the box: the set adds 10 per violating start and nothing else
        added = launch(i, i.set)['con_cost'] - empty['con_cost']
        assert set(N_(added).ravel().tolist()) == {0.0, 10.0}


def test_the_main_case_through_the_kernel():
    """The oracle's main case (tests/test_static_conset_host.py: every signal fires for some row and stays silent for another,
    and one start is outside both the safe polytope and the obstacle slab: 20) as one given launch."""
    spec, con, rows, ref = sco.main_case()
    ssm, env = problems.build(spec, device=DEV)
    env.obj_mode = VAR
    out = {}
    for label, c in (('empty', co.empty(2)), ('full', con)):
        out[label] = cem_mpc.cem_rollout_starts(ssm, env, sco.H, rows=T(rows[None]), want_traj=True, con_set=c.struct(2))
    prob = problems.oracle_problem(spec, ocem)
    plain = seo.rollout(prob, sco.gp_of(spec), rows)
    got, empty = N_(out['full']['con_cost'][0]), N_(out['empty']['con_cost'][0])
    both = ref.start_obs & (plain.start_cost > 0)
    print(f'main case: con_cost differs from the oracle at {int((got != ref.con_cost).sum())} of {len(got)} rows, the empty set '
          f'from the plain oracle at {int((empty != plain.con_cost).sum())}; starts outside both: {int(both.sum())}, their start '
          f'costs {sorted(set((got - ref.signals.extra - (plain.con_cost - plain.start_cost))[both].tolist()))}')
    assert ref.min_abs_d >= sco.MARGIN and both.any()
    np.testing.assert_array_equal(empty, plain.con_cost)
    np.testing.assert_array_equal(got, ref.con_cost)
    np.testing.assert_array_equal((got - empty)[both] - ref.signals.extra[both], 10.0)
    np.testing.assert_allclose(N_(out['full']['obj_cost'][0]), ref.obj_cost, rtol=RTOL, atol=ATOL)


# ---- 3: against the oracle's rollout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_rollout_matches_the_oracle(name):
    i = inputs(name)
    assert_sound(name, i)
    r = launch(i, i.set)
    rows = N_(r['rows'])
    print(f'{name}: rows rel {gse.max_rel(rows, i.rows):.2e}')
    np.testing.assert_allclose(rows, i.rows, rtol=1e-13, atol=1e-16)
    status = 0
    for e in range(E):
        # (the kernel may fuse mean + std * eps into one fma: the oracle rolls out exactly the rows the kernel used)
        ref = sco.rollout(i.prob, i.set, i.gp, rows[e])
        np.testing.assert_array_equal(ref.con_cost, i.refs[e].con_cost)        # (the conditions above hold on these rows too)
        traj = N_(r['traj'][e])
        tp, tq = traj[..., :i.n_s], traj[..., i.n_s:].reshape(i.P, i.H, i.n_s, i.n_s)
        sig, obj, con = N_(r['sigma'][e]), N_(r['obj_cost'][e]), N_(r['con_cost'][e])
        print(f'  problem {e}: centres {gse.max_rel(tp, ref.traj_p):.2e} shapes {gse.max_rel(tq, ref.traj_q):.2e} sigma '
              f'{gse.max_rel(sig, ref.sigma):.2e} obj {gse.max_rel(obj, ref.obj_cost):.2e} con differs at '
              f'{int((con != ref.con_cost).sum())}; costs {sorted(set(ref.con_cost.tolist()))[:8]}')
        np.testing.assert_allclose(tp, ref.traj_p, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(tq, ref.traj_q, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(sig, ref.sigma, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(obj, ref.obj_cost, rtol=RTOL, atol=ATOL)
        np.testing.assert_array_equal(con, ref.con_cost)
        status |= ref.status
    assert int(r['status'].item()) == status


# ---- 4: independence of the particle count ----------------------------------------------------------------------------------------------
def test_particles_do_not_depend_on_the_particle_count():
    big = inputs('P4149')
    full = launch(big, big.set)
    small = launch(big, big.set, first=P)
    differ = differing(small, full, keys=('rows', 'traj', 'sigma', 'obj_cost', 'con_cost'), first=P)
    added = int((full['con_cost'] != launch(big, co.empty(2))['con_cost']).sum())
    print(f'{P} particles alone and as the first of {LARGE}: outputs that differ {differ}; the set changes {added} of '
          f'{E * LARGE} rows')
    assert not differ and added > 0
    assert bool(torch.isfinite(full['obj_cost']).all())


# ---- 5: fused = step by step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in NAMES if n != 'P4149'])
def test_fused_equals_stepwise(name):
    i = inputs(name)
    con = i.set.struct(i.n_s)
    mpc = cem_mpc.StaticCemMpc(gse.device_model(i.model), env_of(i), i.H, i.P, 4, 1, start_mean=i.mean[0, :i.n_s],
                               start_std=i.std[0, :i.n_s], n_restarts=E, device=DEV, con_set=con)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = mpc._rollout_stepwise(T(i.mean), T(i.std), T(i.noise), status)
    fused = launch(i, i.set)
    plain = launch(i, co.empty(i.n_s))
    torch.cuda.synchronize()
    for e in range(E):
        differ = int((s['con_cost'][e] != fused['con_cost'][e]).sum())
        added = int((fused['con_cost'][e] != plain['con_cost'][e]).sum())
        err = gse.max_rel(N_(s['obj_cost'][e]), N_(fused['obj_cost'][e]))
        print(f'{name} e={e}: fused against step by step: objective rel {err:.2e}, constraint costs differ at {differ}; the set '
              f'changes {added} of {i.P} rows')
        np.testing.assert_allclose(N_(s['obj_cost'][e]), N_(fused['obj_cost'][e]), rtol=RTOL, atol=ATOL)
        assert torch.equal(s['con_cost'][e], fused['con_cost'][e])
        assert added > 0
    assert int(status.item()) == int(fused['status'].item())


# ---- 6: the solve of the oracle file ----------------------------------------------------------------------------------------------------
def _rollout_entries(counting):
    return {k: v for k, v in counting.calls.items() if k.startswith('sx_cem_rollout') and not k.endswith(('_form', '_bytes'))}


def _check_solve(label, mpc, noise, per, answer, chosen, stepwise=False):
    best, costs, ok, history, status = mpc.solve(noise=T(noise), stepwise=stepwise)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    for e, (ref_best, ref_costs, ref_ok, trace) in enumerate(per):
        err = float(np.abs(N_(best[e]) - ref_best).max())
        print(f'{label} restart {e}: best row differs by {err:.2e}; (con, obj) {costs[e].tolist()} oracle {ref_costs}')
        assert err < 1e-9
        assert bool(ok[e].item()) == ref_ok and float(costs[e, 0]) == ref_costs[0]
        np.testing.assert_allclose(float(costs[e, 1]), ref_costs[1], rtol=RTOL, atol=ATOL)
    return history


def test_solve_matches_the_numpy_cem_and_differs_from_the_solve_without_the_set():
    """The inputs are those tests/test_static_conset_host.py checks on the CPU.  This test fails without the feature: the same
    solve without the set ends at the oracle's other answer."""
    d = sco.solve()
    spec, con, noise = d['spec'], d['con'], d['noise']
    ssm, env = problems.build(spec, device=DEV)
    kw = dict(start_mean=sco.START_MEAN, start_std=sco.START_STD, n_restarts=sco.E, init_std=sco.INIT_STD, device=DEV)
    mpc = cem_mpc.StaticCemMpc(ssm, env, sco.H, sco.P, sco.K, sco.ITERS, record_rollouts=True, con_set=con.struct(2), **kw)
    counting = CountingLib(_lib.lib())
    with mock.patch.object(_lib, 'lib', lambda: counting):
        history = _check_solve('with the set', mpc, noise, d['per'], d['answer'], d['chosen'])
    print(f'rollout entries {_rollout_entries(counting)}')
    assert _rollout_entries(counting) == {'sx_cem_rollout_starts_cons': sco.ITERS}
    # per iteration and restart: constraint costs exactly, equal elite sets
    assert len(history) == sco.ITERS * sco.E
    for it in range(sco.ITERS):
        for e in range(sco.E):
            h, (cost, obj, idx, _) = history[it * sco.E + e], d['per'][e][3][it]
            got_con, got_obj = N_(h.constraint_costs), N_(h.objective_costs)
            print(f'iteration {it} restart {e}: objective rel {gse.max_rel(got_obj, obj):.2e}, constraint costs differ at '
                  f'{int((got_con != cost).sum())}, {int((cost > 0).sum())} of {len(cost)} rows violate')
            np.testing.assert_array_equal(got_con, cost)
            np.testing.assert_allclose(got_obj, obj, rtol=RTOL, atol=ATOL)
            assert set(ocem.rank(got_con, got_obj, sco.K)) == set(idx)
    found = mpc.find(noise=T(noise))
    assert found is not None and mpc.last_choice == d['chosen']
    np.testing.assert_allclose(found[0].numpy(), d['answer'][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(found[1].numpy(), d['answer'][1], rtol=0, atol=1e-9)
    # the same solve without the set gives the oracle's other answer
    plain = cem_mpc.StaticCemMpc(ssm, env, sco.H, sco.P, sco.K, sco.ITERS, **kw)
    _check_solve('without the set', plain, noise, d['plain_per'], d['plain_answer'], d['plain_chosen'])
    pfound = plain.find(noise=T(noise))
    assert pfound is not None and plain.last_choice == d['plain_chosen']
    np.testing.assert_allclose(pfound[0].numpy(), d['plain_answer'][0], rtol=0, atol=1e-9)
    moved = float(np.abs(np.concatenate((found[0].numpy(), found[1].numpy().ravel()))
                         - np.concatenate((pfound[0].numpy(), pfound[1].numpy().ravel()))).max())
    print(f'the answers with and without the set differ by {moved:.3f}')
    assert moved > 1e-3
    # the step-by-step path carries the set: the same solve through it ends at the same rows
    _check_solve('step by step', mpc, noise, d['per'], d['answer'], d['chosen'], stepwise=True)


# ---- 7: StaticSafeMPCExploration over a CemSafeMPC ----------------------------------------------------------------------------------------
class Conf:
    mpc_time_horizon = sco.H
    cem_num_rollouts = sco.P
    cem_num_elites = sco.K
    cem_num_iterations = sco.ITERS
    cem_init_std = sco.INIT_STD
    plot_cem_optimisation = False
    plot_cem_terminal_states = False
    device = DEV
    use_state_constraint = True
    use_prior_model = True
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'


class Env(problems.StubEnv):
    """StubEnv with the start distribution StaticSafeMPCExploration reads (un-normalised: inv_norm = 1)."""

    def __init__(self, spec):
        super().__init__(spec, np.zeros(spec.n_s))
        self.init_m, self.init_std = np.array(sco.START_MEAN), np.array(sco.START_STD)
        self.inv_norm = [np.ones(spec.n_s), np.ones(spec.n_u)]


def test_static_exploration_through_the_safe_mpc_with_and_without_the_settings():
    from safe_exploration_amd.safempc_exploration import StaticSafeMPCExploration
    d = sco.solve()
    spec, con, noise = d['spec'], d['con'], d['noise']
    opt_env = {'h_mat_obs': con.h_mat_obs, 'h_obs': con.h_obs[:, None]}

    def explore(conf):
        env = Env(spec)
        solver, _ = problems.make_solver(spec, conf, env, device=DEV, opt_env=opt_env)
        ex = StaticSafeMPCExploration(solver, env, n_restarts_optimizer=sco.E, verbosity=0)
        ex._solver.sample_noise = lambda: T(noise)        # the oracle's draws
        counting = CountingLib(_lib.lib())
        with mock.patch.object(_lib, 'lib', lambda: counting):
            x, u = ex.find_max_variance(None)
        return ex, counting, x, u

    on = type('C', (Conf,), dict(cem_static_ctrl_ellipsoid_constraint=True, cem_static_obstacle_constraint=True))()
    ex, counting, x, u = explore(on)
    print(f'settings on: rollout entries {_rollout_entries(counting)}; x {None if x is None else x.ravel()} u '
          f'{None if u is None else u.ravel()}, the oracle\'s {d["answer"][0]} {d["answer"][1][0]}')
    assert _rollout_entries(counting) == {'sx_cem_rollout_starts_cons': sco.ITERS}
    assert 'sx_conset_eval' not in counting.calls and 'sx_onestep_reach' not in counting.calls
    assert (ex._solver._con_set.m_obs, ex._solver._con_set.ctrl_ellipsoid) == (2, 1) and ex._solver.last_choice == d['chosen']
    assert x.shape == (2, 1) and u.shape == (1, 1)
    np.testing.assert_allclose(x.ravel(), d['answer'][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(u.ravel(), d['answer'][1][0], rtol=0, atol=1e-9)
    # with the settings off it calls what it calls today and returns the plain oracle's answer, whatever opt_env holds
    ex, counting, x, u = explore(Conf())
    print(f'settings off: rollout entries {_rollout_entries(counting)}; x {None if x is None else x.ravel()} u '
          f'{None if u is None else u.ravel()}, the oracle\'s {d["plain_answer"][0]} {d["plain_answer"][1][0]}')
    assert _rollout_entries(counting) == {'sx_cem_rollout_starts': sco.ITERS}
    assert ex._solver._con_set is None and ex._solver.last_choice == d['plain_chosen']
    np.testing.assert_allclose(x.ravel(), d['plain_answer'][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(u.ravel(), d['plain_answer'][1][0], rtol=0, atol=1e-9)
