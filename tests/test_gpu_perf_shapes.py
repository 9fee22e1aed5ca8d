"""GPU: the six performance-trajectory entries -- sx_cem_perf_rollout[_multi] (mean-only), sx_cem_perf_rollout_var[_multi]
(variance), sx_cem_perf_rollout_taylor[_multi] (Taylor) -- at the compiled shapes and the sizes the other files leave out:

  1. every entry at (3, 1) (the odd n_s), (1, 1) (no output-by-output kernel) and (4, 2) (the largest register state and the
     largest PerfTaylorConst): against the numpy oracles, drawn against given tail, mode against mode, Taylor against the
     variance kernel, multi-model against single-model, and past one pass of the grid;
  2. the form's dependence on n_perf: the tile's actions (and the Taylor step constants) share LDS with Kstar, so a model
     goes from all outputs in LDS to output by output as n_perf grows -- both sides of that flip, the last one with the
     allocation all but full;
  3. the largest training set of each of the six shapes that still has a form, and the longest trajectory it admits;
  4. row-block and trip edges: n_pad = 16, 32 and 48 with the last block full and just opened; the mean-only kernel's
     32-point trips at N = 1, 31, 32, 33, 64 and at its own LDS limit;
  5. the terminal-safety polytope with SX_MAX_M rows and with one row; the single-model entries' status word.

The cases, inputs and launchers are those of tests/test_gpu_perf_var.py, test_gpu_perf_traj.py, test_gpu_perf_taylor.py
(case() / inputs(): E = 2, H = 5) and of test_gpu_perf_multi.py, test_gpu_perf_taylor_multi.py (E = 3 GPs over one sx_env).
Every limit and every flip is asked of the _form queries (on host-side models, as tests/test_perf_var_host.py builds them),
never computed here.  Tolerances: MEAN_TOL (rtol 1e-10, atol 1e-12) for rows, means and the affine objective; SIGMA_TOL
(rtol 1e-8, atol 1e-11) for perf_sigma, perf_cov and the variance objective; the con_cost increment exactly.  Every case
prints its worst error as a fraction of the tolerance before it asserts.  Measured figures: DESIGN.md section 3.9, "the
other shapes and the size limits"."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import test_gpu_perf_multi as pm
import test_gpu_perf_taylor_multi as ptm
from oracle import cem as ocem
from perf_taylor_oracle import perf_taylor_rollout
from perf_traj_oracle import perf_rollout
from perf_var_oracle import perf_var_rollout
from safe_exploration_amd import _lib, cem_mpc
from safe_exploration_amd.cem_mpc import GpModelTable, PerfModelTable
from test_gpu_perf_taylor import MEAN_TOL, launch as launch_taylor, tails
from test_gpu_perf_traj import launch as launch_mean
from test_gpu_perf_var import ABS, DEV, H, SIGMA_TOL, VAR, N_, T, case, close, inputs, launch as launch_var, worst
from test_perf_var_host import _model as host_model

pytestmark = pytest.mark.gpu
SMALL, LARGE = 37, 4096 + 53
NEW_SHAPES = [(3, 1), (1, 1), (4, 2)]
ALL_SHAPES = [(2, 1), (3, 1), (4, 1), (2, 2), (4, 2), (1, 1)]
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
KINDS = ('mean', 'var', 'taylor')
ENTRY = {'mean': 'sx_cem_perf_rollout', 'var': 'sx_cem_perf_rollout_var', 'taylor': 'sx_cem_perf_rollout_taylor'}
FIELDS = {'mean': ('rows', 'perf_traj', 'obj_cost', 'con_cost'),
          'var': ('rows', 'perf_traj', 'perf_sigma', 'obj_cost', 'con_cost'),
          'taylor': ('rows', 'perf_traj', 'perf_sigma', 'perf_cov', 'obj_cost', 'con_cost')}
LAUNCH = {'mean': launch_mean, 'var': launch_var, 'taylor': launch_taylor}
MODES_OF = {'mean': (ABS,), 'var': (VAR, ABS), 'taylor': (VAR, ABS)}
# (N, n_perf, r): (2, 1) and (8, 3) everywhere; (40, 3) for the mean-only and variance entries where the oracle stays cheap
CASES = [(N, n_perf, r) for N in (7, 200, 590) for n_perf, r in ((2, 1), (8, 3))]
LONG = [(N, 40, 3) for N in (7, 200)]


# ---- the form queries -------------------------------------------------------------------------------------------------------
def form(kind, model, n_perf):
    """What the single-model form query of `kind` answers for an sx_gp_model (a GpCemSSM's, or a host-side one)."""
    query = {'var': 'sx_cem_perf_rollout_var_form', 'taylor': 'sx_cem_perf_rollout_taylor_form'}[kind]
    return int(getattr(_lib.lib(), query)(ctypes.byref(model), n_perf))


def expect_form(kind, ssm, n_s, n_perf):
    """Asserted before a launch: all outputs in LDS at N = 7 and 200, and at 590 for one output; output by output at 590
    for the other shapes.  (The mean-only kernel has one form.)"""
    if kind == 'mean':
        return None
    N = ssm.device_model.n_train
    got, want = form(kind, ssm.device_model, n_perf), SX_FORM_BYOUT if N == 590 and n_s > 1 else SX_FORM_STREAM
    assert got == want, f'{ENTRY[kind]} ({n_s}, .) N={N} n_perf={n_perf}: form {got}, expected {want}'
    return got


# ---- the oracles ------------------------------------------------------------------------------------------------------------
def oracle(kind, probs, gp, x0, safe, tail, r, **kw):
    if kind == 'mean':
        return perf_rollout(probs[ABS], gp, x0, safe, tail, r)
    if kind == 'var':
        return perf_var_rollout(probs[VAR], gp, x0, safe, tail, r)
    return perf_taylor_rollout(probs[VAR], gp, x0, safe, tail, r, **kw)


def oracle_objective(kind, prob, ref):
    if kind == 'mean':
        return ref.obj_cost
    return sum(ocem.objective_cost(prob, ref.traj[:, t], ref.sigma[:, t]) for t in range(ref.traj.shape[1]))


def oracle_conditions(kind, refs, n_perf, label):
    """On the oracle alone: some tail action leaves the box, and (Taylor, n_perf > 2) the propagated part of diag G is not
    lost below the tolerance of diag G."""
    violations = sum(int(ref.violations.sum()) for ref in refs)
    assert violations > 0, f'{label}: no tail action leaves the box'
    if kind == 'taylor':
        assert all(np.isfinite(ref.cov).all() for ref in refs), f'{label}: the oracle\'s covariance is not finite'
        propagated = max(float((ref.sigma - ref.var).max()) for ref in refs)
        print(f'{label}: oracle: {violations} box violations, largest propagated part of diag G {propagated:.3e}, largest '
              f'covariance entry {max(float(np.abs(ref.cov).max()) for ref in refs):.3e}')
        if n_perf > 2:
            assert propagated > 100 * SIGMA_TOL['atol'], label


_REFS = {}


def single_refs(kind, n_s, n_u, N, P, n_perf, r, seed=None):
    """(inputs, the oracle's rollout of `kind` per problem) of a single-model case: computed once, left unchanged."""
    key = (kind, n_s, n_u, N, P, n_perf, r, seed)
    if key not in _REFS:
        gp, probs = case(n_s, n_u, N)[3:]
        inp = inputs(n_s, n_u, P, n_perf, r, seed=n_s + 7 * n_u + N + P + 100 * n_perf + r if seed is None else seed)
        refs = [oracle(kind, probs, gp, inp['x0'][e], inp['safe'][e], tail, r) for e, tail in enumerate(tails(inp))]
        oracle_conditions(kind, refs, n_perf, f'{ENTRY[kind]} ({n_s},{n_u}) N={N} P={P} n_perf={n_perf} r={r}')
        _REFS[key] = (inp, refs)
    return _REFS[key]


def multi_refs(kind, n_s, n_u, sizes, P, n_perf, r):
    key = (kind, n_s, n_u, sizes, P, n_perf, r)
    if key not in _REFS:
        gps, probs = pm.case(n_s, n_u, sizes)[2:]
        inp = pm.inputs(len(sizes), n_s, n_u, P, n_perf, r, seed=41 + n_s + 7 * n_u + P + 100 * n_perf + r + sum(sizes))
        refs = [oracle(kind, probs, gps[e], inp['x0'][e], inp['safe'][e], ptm.tail_of(inp, e), r) for e in range(len(sizes))]
        oracle_conditions(kind, refs, n_perf, f'{ENTRY[kind]}_multi ({n_s},{n_u}) N={sizes} P={P} n_perf={n_perf} r={r}')
        _REFS[key] = (inp, refs)
    return _REFS[key]


def against_the_oracle(kind, out, e, o, ref, want_obj, obj_tol, con0, label):
    """Problem e of `out` against `ref` (o: its index in `out`): prints the worst errors as fractions of their tolerances,
    then asserts them."""
    parts = [f'rows {worst(out["rows"][o], ref.rows, **MEAN_TOL):.2e}',
             f'traj {worst(out["perf_traj"][o], ref.traj, **MEAN_TOL):.2e}']
    if kind != 'mean':
        parts.append(f'sigma {worst(out["perf_sigma"][o], ref.sigma, **SIGMA_TOL):.2e}')
    if kind == 'taylor':
        parts.append(f'cov {worst(out["perf_cov"][o], ref.cov, **SIGMA_TOL):.2e}')
    parts.append(f'obj {worst(out["obj_cost"][o], want_obj, **obj_tol):.2e}')
    print(f'{label}: of the tolerance: ' + ', '.join(parts))
    close(out['rows'][o], ref.rows, **MEAN_TOL)
    close(out['perf_traj'][o], ref.traj, **MEAN_TOL)
    if kind != 'mean':
        close(out['perf_sigma'][o], ref.sigma, **SIGMA_TOL)
    if kind == 'taylor':
        close(out['perf_cov'][o], ref.cov, **SIGMA_TOL)
    close(out['obj_cost'][o], want_obj, **obj_tol)
    close(out['con_cost'][o] - T(con0[e]), ref.con_cost, rtol=0, atol=0)


def given_rows(drawn):
    rows = drawn['rows'].clone()
    rows[:, :, :H] = float('nan')                 # the safety part of the rows is an output in both forms
    return rows


# ---- 1: every entry at (3, 1), (1, 1), (4, 2) -------------------------------------------------------------------------------
def check_single(kind, n_s, n_u, N, P, n_perf, r, want_form='by N', seed=None):
    """One single-model case in both tail forms and every objective mode of the entry.  Returns (inputs, {mode: drawn})."""
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    inp, refs = single_refs(kind, n_s, n_u, N, P, n_perf, r, seed)
    if want_form == 'by N':
        expect_form(kind, ssm, n_s, n_perf)
    elif kind != 'mean':
        assert form(kind, ssm.device_model, n_perf) == want_form
    outs = {}
    for mode in MODES_OF[kind]:
        obj_tol = SIGMA_TOL if mode == VAR else MEAN_TOL
        drawn = LAUNCH[kind](ssm, envs[mode], inp, n_perf, r)
        given = LAUNCH[kind](ssm, envs[mode], inp, n_perf, r, rows=given_rows(drawn))
        for e, ref in enumerate(refs):
            want_obj = oracle_objective(kind, probs[mode], ref)
            for name, out in (('drawn', drawn), ('given', given)):
                against_the_oracle(kind, out, e, e, ref, want_obj, obj_tol, inp['con0'],
                                   f'{ENTRY[kind]} ({n_s},{n_u}) N={N} P={P} n_perf={n_perf} r={r} e={e} mode={mode} {name}')
            assert torch.equal(drawn['rows'][e, :, :H], T(inp['safe'][e]))           # the shared actions: bit-identical
        for n in FIELDS[kind][1:]:
            assert torch.equal(drawn[n], given[n]), n                               # the two forms see the same tail bits
        if kind == 'taylor':
            assert torch.equal(drawn['perf_cov'], drawn['perf_cov'].transpose(-1, -2))   # symmetric to the bit
        outs[mode] = drawn
    if len(outs) == 2:
        for n in FIELDS[kind]:
            if n != 'obj_cost':
                assert torch.equal(outs[VAR][n], outs[ABS][n]), n                   # the mode changes the objective only
    return inp, outs


def taylor_against_the_variance_kernel(n_s, n_u, N, n_perf, r, inp, tay):
    """The mean recursion is the variance kernel's fma chain, and Sigma_0 = 0 leaves the GP's own variance at step 0: bit
    for bit where the two kernels take the same form.  Between the flips of the two entries (part 2) the Taylor kernel
    already runs output by output and the variance kernel does not yet -- another summation order: within the tolerances."""
    ssm, envs = case(n_s, n_u, N)[:2]
    var = launch_var(ssm, envs[VAR], inp, n_perf, r)
    assert torch.equal(tay['rows'], var['rows']) and torch.equal(tay['con_cost'], var['con_cost'])
    assert torch.equal(tay['perf_cov'][:, :, 0], torch.diag_embed(tay['perf_sigma'][:, :, 0]))
    if form('taylor', ssm.device_model, n_perf) == form('var', ssm.device_model, n_perf):
        assert torch.equal(tay['perf_traj'], var['perf_traj'])
        assert torch.equal(tay['perf_sigma'][:, :, 0], var['perf_sigma'][:, :, 0])
    else:
        print(f'({n_s},{n_u}) N={N} n_perf={n_perf}: Taylor output by output, variance not; of the tolerance: traj '
              f'{worst(tay["perf_traj"], var["perf_traj"], **MEAN_TOL):.2e}, step-0 variance '
              f'{worst(tay["perf_sigma"][:, :, 0], var["perf_sigma"][:, :, 0], **SIGMA_TOL):.2e}')
        close(tay['perf_traj'], var['perf_traj'], **MEAN_TOL)
        close(tay['perf_sigma'][:, :, 0], var['perf_sigma'][:, :, 0], **SIGMA_TOL)


@pytest.mark.parametrize('N,n_perf,r', CASES + LONG)
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_mean_only_entry_matches_the_oracle(n_s, n_u, N, n_perf, r):
    check_single('mean', n_s, n_u, N, SMALL, n_perf, r)


@pytest.mark.parametrize('N,n_perf,r', CASES + LONG)
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_variance_entry_matches_the_oracle(n_s, n_u, N, n_perf, r):
    """(1, 1) keeps Kstar of its one output in LDS at 590 too; (3, 1) and (4, 2) go output by output there."""
    inp, outs = check_single('var', n_s, n_u, N, SMALL, n_perf, r)
    # the means, rows and costs are the mean-only kernel's to the tolerance: it sums k* . alpha in another order
    ssm, envs = case(n_s, n_u, N)[:2]
    mean_only = launch_mean(ssm, envs[ABS], inp, n_perf, r)
    assert torch.equal(outs[ABS]['rows'], mean_only['rows']) and torch.equal(outs[ABS]['con_cost'], mean_only['con_cost'])
    close(outs[ABS]['perf_traj'], mean_only['perf_traj'], **MEAN_TOL)
    close(outs[ABS]['obj_cost'], mean_only['obj_cost'], **MEAN_TOL)


@pytest.mark.parametrize('N,n_perf,r', CASES)
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_taylor_entry_matches_the_oracle(n_s, n_u, N, n_perf, r):
    """No (40, 3): at (4, 2), N = 200 the oracle's propagated covariance reaches 2e1 by step 40 with this case's prior -- a
    test of the oracle's conditioning, not of the kernel."""
    inp, outs = check_single('taylor', n_s, n_u, N, SMALL, n_perf, r)
    taylor_against_the_variance_kernel(n_s, n_u, N, n_perf, r, inp, outs[VAR])


# the multi-model entries: E = 3 GPs of their own over one sx_env
def launch_m(kind, ssms, env, inp, n_perf, r, rows=None, table=None, **kw):
    if kind == 'taylor':
        return ptm.launch_multi(ssms, env, inp, n_perf, r, rows=rows, table=table, **kw)
    return pm.launch_multi(ssms, env, inp, n_perf, r, kind == 'var', rows=rows, table=table, **kw)


def launch_s(kind, ssm, env, inp, e, n_perf, r, rows=None):
    if kind == 'taylor':
        return ptm.launch_single(ssm, env, inp, e, n_perf, r, rows=rows)
    return pm.launch_single(ssm, env, inp, e, n_perf, r, kind == 'var', rows=rows)


def multi_forms(kind, ssms, n_s, sizes, n_perf):
    """(the launch's form, every model's own), asserted: over (7, 200, 590) output by output at (3, 1) and (4, 2), all
    outputs in LDS at (1, 1); over (7, 100, 200) all outputs in LDS.  The mean-only kernel has one form."""
    if kind == 'mean':
        return 0, [0] * len(ssms)
    multi_form, own = (pm if kind == 'var' else ptm).forms(ssms, n_perf)
    want = SX_FORM_BYOUT if 590 in sizes and n_s > 1 else SX_FORM_STREAM
    assert multi_form == want, f'{ENTRY[kind]}_multi N={sizes} n_perf={n_perf}: form {multi_form}, expected {want}'
    assert own == [SX_FORM_BYOUT if N == 590 and n_s > 1 else SX_FORM_STREAM for N in sizes], own
    return multi_form, own


def check_multi(kind, n_s, n_u, sizes, P, n_perf, r):
    ssms, envs, gps, probs = pm.case(n_s, n_u, sizes)
    inp, refs = multi_refs(kind, n_s, n_u, sizes, P, n_perf, r)
    multi_form, own = multi_forms(kind, ssms, n_s, sizes, n_perf)
    table = PerfModelTable() if kind == 'mean' else GpModelTable()
    outs = {}
    for mode in MODES_OF[kind]:
        obj_tol = SIGMA_TOL if mode == VAR else MEAN_TOL
        drawn = launch_m(kind, ssms, envs[mode], inp, n_perf, r, table=table)
        rows = given_rows(drawn)
        given = launch_m(kind, ssms, envs[mode], inp, n_perf, r, rows=rows, table=table)
        for e, ref in enumerate(refs):
            want_obj = oracle_objective(kind, probs[mode], ref)
            label = f'{ENTRY[kind]}_multi ({n_s},{n_u}) N={sizes[e]} of {sizes} P={P} n_perf={n_perf} r={r} mode={mode}'
            for name, out, rows_in in (('drawn', drawn, None), ('given', given, rows)):
                against_the_oracle(kind, out, e, e, ref, want_obj, obj_tol, inp['con0'], f'{label} {name}')
                one = launch_s(kind, ssms[e], envs[mode], inp, e, n_perf, r, rows=rows_in)
                if own[e] == multi_form:          # the launch's form is the model's own: the single-model launch, bit for bit
                    for n in FIELDS[kind]:
                        assert torch.equal(out[n][e], one[n][0]), f'{label} {name} {n}'
                else:                             # output by output only because another model needs it
                    against_the_oracle(kind, one, e, 0, ref, want_obj, obj_tol, inp['con0'], f'{label} {name}, its own launch')
                    for n in FIELDS[kind]:
                        tol = (MEAN_TOL if n in ('rows', 'perf_traj') else
                               SIGMA_TOL if n in ('perf_sigma', 'perf_cov') else obj_tol)
                        if n == 'con_cost':
                            assert torch.equal(out[n][e], one[n][0])
                        else:
                            close(out[n][e], one[n][0], **tol)
            assert torch.equal(drawn['rows'][e, :, :H], T(inp['safe'][e]))
        for n in FIELDS[kind][1:]:
            assert torch.equal(drawn[n], given[n]), n
        if kind == 'taylor':
            assert torch.equal(drawn['perf_cov'], drawn['perf_cov'].transpose(-1, -2))
        outs[mode] = drawn
    assert any(f == multi_form for f in own)      # something is compared bit for bit
    if len(outs) == 2:
        for n in FIELDS[kind]:
            if n != 'obj_cost':
                assert torch.equal(outs[VAR][n], outs[ABS][n]), n
    return inp, outs


MULTI_CASES = [(sizes, n_perf, r) for sizes in (pm.SIZES, pm.SIZES_STREAM) for n_perf, r in ((2, 1), (8, 3))]


@pytest.mark.parametrize('kind', ['mean', 'var'])
@pytest.mark.parametrize('sizes,n_perf,r', MULTI_CASES + [(pm.SIZES_STREAM, 40, 3)])
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_multi_model_entries_match_the_oracle_and_the_single_model_launch(n_s, n_u, sizes, n_perf, r, kind):
    check_multi(kind, n_s, n_u, sizes, SMALL, n_perf, r)


@pytest.mark.parametrize('sizes,n_perf,r', MULTI_CASES)
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_taylor_multi_model_entry_matches_the_oracle_and_the_single_model_launch(n_s, n_u, sizes, n_perf, r):
    check_multi('taylor', n_s, n_u, sizes, SMALL, n_perf, r)


# grid independence: one case per new shape and entry, chosen so that every N and both horizons occur
GRID_CASES = {(3, 1): (590, pm.SIZES, 2, 1), (1, 1): (200, pm.SIZES, 8, 3), (4, 2): (7, pm.SIZES_STREAM, 8, 3)}


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_single_model_tile_does_not_depend_on_the_grid(n_s, n_u, kind):
    """P = 4096 + 53 per problem; the first 37 particles of each problem in a launch of their own are bit-identical."""
    N, _, n_perf, r = GRID_CASES[(n_s, n_u)]
    ssm, envs = case(n_s, n_u, N)[:2]
    expect_form(kind, ssm, n_s, n_perf)
    inp = inputs(n_s, n_u, LARGE, n_perf, r, seed=n_s + N)
    sub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in inp.items()}
    for mode in MODES_OF[kind]:
        big, small = LAUNCH[kind](ssm, envs[mode], inp, n_perf, r), LAUNCH[kind](ssm, envs[mode], sub, n_perf, r)
        for n in FIELDS[kind]:
            assert torch.equal(small[n], big[n][:, :SMALL]), n


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_multi_model_tile_does_not_depend_on_the_grid(n_s, n_u, kind):
    _, sizes, n_perf, r = GRID_CASES[(n_s, n_u)]
    ssms, envs = pm.case(n_s, n_u, sizes)[:2]
    multi_forms(kind, ssms, n_s, sizes, n_perf)
    inp = pm.inputs(len(sizes), n_s, n_u, LARGE, n_perf, r, seed=n_s + sum(sizes))
    sub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in inp.items()}
    for mode in MODES_OF[kind]:
        big, small = launch_m(kind, ssms, envs[mode], inp, n_perf, r), launch_m(kind, ssms, envs[mode], sub, n_perf, r)
        for n in FIELDS[kind]:
            assert torch.equal(small[n], big[n][:, :SMALL]), n


# ---- 2: the form's dependence on n_perf, and the full LDS -------------------------------------------------------------------
# (n_s, n_u, N): {kind: the last n_perf with all outputs in LDS, as the LDS arithmetic gives it}
FLIPS = {(4, 2, 249): dict(var=10, taylor=5), (3, 1, 346): dict(var=24, taylor=17), (2, 1, 500): dict(var=74, taylor=69)}
FLIP_P = 17     # two tiles, the second with one particle: the oracle at n_perf ~ 70 is what these cases cost


def walk_n_perf(kind, model, stop=1 << 12):
    """The form query's answers for n_perf = 2, 3, ... up to the first refusal (exclusive)."""
    seq = []
    for n_perf in range(2, stop):
        f = form(kind, model, n_perf)
        if f < 0:
            return seq
        seq.append(f)
    raise AssertionError(f'a form for every n_perf below {stop}')


@pytest.mark.parametrize('side', ['last with all outputs in LDS', 'first output by output'])
@pytest.mark.parametrize('kind', ['var', 'taylor'])
@pytest.mark.parametrize('n_s,n_u,N', list(FLIPS))
def test_both_sides_of_the_flip_of_the_form_with_n_perf(n_s, n_u, N, kind, side):
    """Walking n_perf upward the query answers SX_FORM_STREAM, then SX_FORM_BYOUT, and changes exactly once; the launch at
    the last STREAM value -- the Taylor constants in the last bytes of a nearly full allocation -- and at the first BYOUT
    value match the oracle.  Where the flip lands is printed beside the derived value, not asserted.
    The (2, 1) flip is at n_perf ~ 70: with this case's prior (a = 0.85 I + noise) the Taylor oracle's covariance stays
    finite and its propagated part above the tolerance floor (asserted on the oracle, as in every case)."""
    ssm = case(n_s, n_u, N)[0]
    seq = walk_n_perf(kind, ssm.device_model)
    assert seq == walk_n_perf(kind, host_model(n_s, n_u, N))                        # the query reads the sizes alone
    changes = [i for i in range(1, len(seq)) if seq[i] != seq[i - 1]]
    assert len(changes) == 1 and seq[0] == SX_FORM_STREAM and seq[-1] == SX_FORM_BYOUT, (changes, seq[0], seq[-1])
    last_stream = 2 + changes[0] - 1
    print(f'{ENTRY[kind]} ({n_s},{n_u}) N={N}: all outputs in LDS up to n_perf = {last_stream} (derived: '
          f'{FLIPS[(n_s, n_u, N)][kind]}), output by output from {last_stream + 1} to {2 + len(seq) - 1}')
    n_perf, want = (last_stream, SX_FORM_STREAM) if side.startswith('last') else (last_stream + 1, SX_FORM_BYOUT)
    inp, outs = check_single(kind, n_s, n_u, N, FLIP_P, n_perf, min(3, n_perf - 1), want_form=want)
    if kind == 'taylor':
        taylor_against_the_variance_kernel(n_s, n_u, N, n_perf, min(3, n_perf - 1), inp, outs[VAR])


# ---- 3: the largest model of each shape -------------------------------------------------------------------------------------
# the largest N with a form at n_perf = 2 as the LDS arithmetic gives it: {(n_s, n_u): (variance, Taylor)}
DERIVED_LIMITS = {(2, 1): (988, 988), (3, 1): (923, 907), (4, 1): (858, 842), (2, 2): (939, 939), (4, 2): (809, 809),
                  (1, 1): (1021, 1021)}
SEARCH_TO = 1200
LIMIT_P = 17


def largest_n(kind, n_s, n_u):
    sizes = [N for N in range(1, SEARCH_TO + 1) if form(kind, host_model(n_s, n_u, N), 2) >= 0]
    assert sizes and sizes[-1] < SEARCH_TO and sizes == list(range(1, sizes[-1] + 1))   # one interval, inside the search
    return sizes[-1]


def refused_without_a_launch(kind, ssm, env, n_s, n_u, n_perf, r):
    """The entry raises SxError 'no form' (SX_ERR_UNSUPPORTED) and has written nothing."""
    inp = inputs(n_s, n_u, SMALL, n_perf, r, seed=1)
    obj = torch.full((2, SMALL), float('nan'), dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    wrapper = {'var': cem_mpc.cem_perf_rollout_var, 'taylor': cem_mpc.cem_perf_rollout_taylor}[kind]
    with pytest.raises(_lib.SxError, match='no form'):
        wrapper(ssm, env, T(inp['x0']), H, n_perf, r, safe_actions=T(inp['safe']), obj_cost=obj, con_cost=T(inp['con0']),
                status=status, tail_mean=T(inp['mean']), tail_std=T(inp['std']), tail_noise=T(inp['noise']))
    torch.cuda.synchronize()
    assert bool(torch.isnan(obj).all()) and int(status.item()) == 0


@pytest.mark.parametrize('which', ['n_perf = 2', 'the last n_perf'])
@pytest.mark.parametrize('kind', ['var', 'taylor'])
@pytest.mark.parametrize('n_s,n_u', ALL_SHAPES)
def test_the_largest_model_of_a_shape(n_s, n_u, kind, which):
    """The largest N the form query accepts at n_perf = 2, built for real, at n_perf = 2 and at the longest trajectory the
    query still accepts, against the oracle; one point more, and one step more, have no form and are refused by the entry
    before any launch.  (1, 1) reaches n_pad = 1024 and the whole LDS with its one output in it; every other shape ends
    output by output below n_pad = 1024, where one output's Kstar and the training inputs fill the LDS."""
    N = largest_n(kind, n_s, n_u)
    ssm, envs = case(n_s, n_u, N)[:2]
    seq = walk_n_perf(kind, ssm.device_model)
    last = 2 + len(seq) - 1
    assert ssm.device_model.n_pad == host_model(n_s, n_u, N).n_pad and seq == walk_n_perf(kind, host_model(n_s, n_u, N))
    derived = DERIVED_LIMITS[(n_s, n_u)][kind == 'taylor']
    print(f'{ENTRY[kind]} ({n_s},{n_u}): the largest N with a form {N} (derived: {derived}), n_pad {ssm.device_model.n_pad}, '
          f'form {seq[0]} at n_perf = 2, the last n_perf {last} (form {seq[-1]})')
    assert form(kind, ssm.device_model, last + 1) == -1 and form(kind, host_model(n_s, n_u, N + 1), 2) == -1
    if which == 'n_perf = 2':
        check_single(kind, n_s, n_u, N, LIMIT_P, 2, 1, want_form=seq[0])
        bigger = case(n_s, n_u, N + 1)
        refused_without_a_launch(kind, bigger[0], bigger[1][VAR], n_s, n_u, 2, 1)
    else:
        check_single(kind, n_s, n_u, N, LIMIT_P, last, min(3, last - 1), want_form=seq[-1])
        refused_without_a_launch(kind, ssm, envs[VAR], n_s, n_u, last + 1, min(3, last - 1))


# ---- 4: block and trip edges ------------------------------------------------------------------------------------------------
def block_edges(n_s, n_u):
    """N = 1, and the N that fill a 16-row block of the packed model exactly (the rows behind the training points hold the
    mean and the Jacobian rows) and open the next one: n_pad = 16 | 16, 32 | 32, 48."""
    k = 1 + n_s + n_u
    return [1, 16 - k, 16 - k + 1, 32 - k, 32 - k + 1]


@pytest.mark.parametrize('kind', ['var', 'taylor'])
@pytest.mark.parametrize('n_s,n_u,N', [(n_s, n_u, N) for n_s, n_u in ((3, 1), (4, 2)) for N in block_edges(n_s, n_u)])
def test_gp_product_entries_at_the_row_block_edges(n_s, n_u, N, kind):
    """n_pad = 32 and 48 give the Kstar phase fewer row pairs than the workgroup has waves."""
    ssm = case(n_s, n_u, N)[0]
    edges = block_edges(n_s, n_u)
    assert ssm.device_model.n_pad == {edges[0]: 16, edges[1]: 16, edges[2]: 32, edges[3]: 32, edges[4]: 48}[N]
    inp, outs = check_single(kind, n_s, n_u, N, SMALL, 8, 3, want_form=SX_FORM_STREAM)
    if kind == 'taylor':
        taylor_against_the_variance_kernel(n_s, n_u, N, 8, 3, inp, outs[VAR])


@pytest.mark.parametrize('N', [1, 31, 32, 33, 64])
@pytest.mark.parametrize('n_s,n_u', NEW_SHAPES)
def test_mean_only_entry_at_the_trip_edges(n_s, n_u, N):
    """The kernel pads to 32 points, a trip of its 16 lanes: one trip with one point, a trip one short, exactly full, one
    more (the prefetch behind the last trip wraps to the first rows), two full trips."""
    check_single('mean', n_s, n_u, N, SMALL, 8, 3)


def call_mean_only(model, alpha, env, bufs, E, P, n_perf, r):
    x0, safe, mean, std, noise, rows, obj, con, status = bufs
    return _lib.lib().sx_cem_perf_rollout(ctypes.byref(model), _lib.ptr(alpha), ctypes.byref(env), E, P, H, n_perf, r,
                                          *[_lib.ptr(b) for b in (x0, safe, mean, std, noise, rows, obj, con)], None,
                                          _lib.ptr(status), _lib.stream_ptr(torch.device(DEV)))


def test_mean_only_entry_at_its_lds_limit():
    """(4, 2): the mean-only form stages the training inputs and alpha in LDS and knows no n_pad <= 1024 rule.  Its largest
    N is found by bisection over the entry's own answer (SX_OK | SX_ERR_UNSUPPORTED), on a model whose training inputs and
    alpha are zeros of the search's largest size, so that an accepted call is a launch within its buffers.  That N, built for
    real, matches the oracle; one more is refused before any launch.  The LDS arithmetic gives 2016."""
    n_s, n_u, top = 4, 2, 4096
    env = case(n_s, n_u, 7)[1][ABS]
    zeros_x = torch.zeros((top, n_s + n_u), dtype=torch.float64, device=DEV)
    zeros_alpha = torch.zeros((n_s, top), dtype=torch.float64, device=DEV)
    inp = inputs(n_s, n_u, 1, 2, 1, seed=1)

    def accepted(N):
        model = host_model(n_s, n_u, N)
        model.x_train = zeros_x.data_ptr()
        obj = torch.full((2, 1), float('nan'), dtype=torch.float64, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        bufs = (T(inp['x0']), T(inp['safe']), T(inp['mean']), T(inp['std']), T(inp['noise']),
                torch.empty((2, 1, H + 1, n_u), dtype=torch.float64, device=DEV), obj, T(inp['con0']), status)
        code = call_mean_only(model, zeros_alpha, env, bufs, 2, 1, 2, 1)
        torch.cuda.synchronize()
        assert code in (_lib.SX_OK, _lib.SX_ERR_UNSUPPORTED), code
        # accepted: a launch over zeros (finite costs, no status bit); refused: nothing written
        assert bool(torch.isfinite(obj).all() if code == _lib.SX_OK else torch.isnan(obj).all()) and int(status.item()) == 0
        return code == _lib.SX_OK

    lo, hi = 1, top
    assert accepted(lo) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    print(f'sx_cem_perf_rollout (4,2): the largest N the entry accepts {lo} (derived: 2016)')
    assert accepted(lo) and not accepted(lo + 1)
    check_single('mean', n_s, n_u, lo, SMALL, 2, 1)


# ---- 5: the polytope's rows, and the single-model status word ---------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,m', [(3, 1, _lib.SX_MAX_M), (1, 1, 1)])
def test_terminal_safety_with_the_most_and_the_fewest_polytope_rows(n_s, n_u, m):
    """The gap construction of tests/test_gpu_perf_taylor.py::test_terminal_safety over a polytope of m rows (SX_MAX_M unit
    normals at (3, 1); the one row x <= h at (1, 1)): the offset comes from the oracle -- every particle's largest row
    distance with h_vec = 0, sorted, and a common h_vec in the widest gap between neighbours inside the middle half."""
    N, n_perf, r = 200, H + 3, 1
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    h_mat = np.random.default_rng(50 + m).normal(size=(m, n_s))
    h_mat /= np.linalg.norm(h_mat, axis=1, keepdims=True)
    if m == 1:
        h_mat = np.ones((1, 1))
    inp = inputs(n_s, n_u, SMALL, n_perf, r, seed=23 + n_s + N)
    zero = dataclasses.replace(probs[VAR], h_mat=h_mat, h_vec=np.zeros((m, 1)))
    d_max = np.concatenate([perf_taylor_rollout(zero, gp, inp['x0'][e], inp['safe'][e], tail, r).distances.max(axis=1)
                            for e, tail in enumerate(tails(inp))])
    order = np.sort(d_max)
    lo, hi = len(order) // 4, 3 * len(order) // 4
    i = lo + int(np.argmax(np.diff(order[lo:hi + 1])))
    gap, offset = order[i + 1] - order[i], 0.5 * (order[i] + order[i + 1])
    print(f'({n_s},{n_u}) N={N} m={m}: offset {offset:.6e}, gap {gap:.3e}, {int((d_max >= offset).sum())} of {len(d_max)} '
          f'violate')
    assert gap > 1e-6
    prob = dataclasses.replace(zero, h_vec=np.full((m, 1), offset))
    env = _lib.SxEnv.from_buffer_copy(envs[VAR])
    env.m = m
    _lib.fill(env.h_mat, h_mat)
    _lib.fill(env.h_vec, np.full(m, offset))
    refs = [perf_taylor_rollout(prob, gp, inp['x0'][e], inp['safe'][e], tail, r, terminal_safety=True)
            for e, tail in enumerate(tails(inp))]
    unsafe = sum(int(ref.unsafe.sum()) for ref in refs)
    assert len(d_max) // 4 <= unsafe <= 3 * len(d_max) // 4 + 1
    assert min(float(np.abs(ref.distances.max(axis=1)).min()) for ref in refs) >= 0.5 * gap * (1 - 1e-9)
    if m > 1:     # the deciding row is not always the same one: the loop over the rows runs to the last
        assert len({int(np.argmax(ref.distances[c])) for ref in refs for c in range(SMALL)}) > 1
    on, off = launch_taylor(ssm, env, inp, n_perf, r, terminal_safety=True), launch_taylor(ssm, env, inp, n_perf, r)
    for e, ref in enumerate(refs):
        close(on['con_cost'][e] - T(inp['con0'][e]), ref.con_cost, rtol=0, atol=0)
        close(off['con_cost'][e] - T(inp['con0'][e]), ocem.ACTION_VIOLATION_COST * ref.violations, rtol=0, atol=0)
    for n in FIELDS['taylor'][:5]:
        assert torch.equal(on[n], off[n]), n


@pytest.mark.parametrize('kind', KINDS)
def test_a_nan_model_sets_the_single_model_status_word(kind):
    """(3, 1), N = 200: a data NaN in what the form reads of the model -- alpha for the mean-only form, the packed operands
    for the GP-product forms (a_pack[0]: the first fragment of output 0's first row-block, which every tile reads) -- sets
    SX_STATUS_NAN and leaves obj_cost NaN; once the value is back, a launch reproduces the clean one."""
    n_s, n_u, N, n_perf, r = 3, 1, 200, 8, 3
    ssm, envs = case(n_s, n_u, N)[:2]
    env = envs[ABS if kind == 'mean' else VAR]
    inp = inputs(n_s, n_u, SMALL, n_perf, r, seed=17)
    clean = LAUNCH[kind](ssm, env, inp, n_perf, r)
    E, P = 2, SMALL
    kw = dict(safe_actions=T(inp['safe']), tail_mean=T(inp['mean']), tail_std=T(inp['std']), tail_noise=T(inp['noise']),
              want_traj=True, **({} if kind == 'mean' else dict(want_sigma=True)))
    wrapper = {'mean': cem_mpc.cem_perf_rollout, 'var': cem_mpc.cem_perf_rollout_var,
               'taylor': cem_mpc.cem_perf_rollout_taylor}
    poisoned = (ssm._alpha if kind == 'mean' else ssm._buffers[1]).view(-1)
    keep = poisoned[0].clone()
    poisoned[0] = float('nan')
    try:
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = wrapper[kind](ssm, env, T(inp['x0']), H, n_perf, r, status=status, con_cost=T(inp['con0']),
                            obj_cost=torch.zeros((E, P), dtype=torch.float64, device=DEV), **kw)
        torch.cuda.synchronize()
    finally:
        poisoned[0] = keep
    assert int(status.item()) & _lib.SX_STATUS_NAN
    assert bool(torch.isnan(out['obj_cost']).all())
    again = LAUNCH[kind](ssm, env, inp, n_perf, r)          # asserts a clean status word
    for n in FIELDS[kind]:
        assert bool(torch.isfinite(clean[n]).all()) and torch.equal(again[n], clean[n]), n
