"""GPU: the cautious and the saturating-cost rollouts -- sx_cem_cautious_rollout[_sat], sx_cem_perf_rollout_taylor_sat[_multi],
sx_cem_rollout[_elites]_sat[_multi] -- at the compiled shapes, forms and sizes the files that came with them leave out:

  1. the cautious rollout at (3, 1) (the odd n_s), (1, 1) (no output-by-output kernel) and (4, 2) (the largest register
     state): against the numpy oracle, its decisions exactly with the bounds placed by the oracle, against the Taylor and the
     variance kernel bit for bit, and past one pass of the grid;
  2. the size limits of the cautious form at all six shapes: both sides of the flip of the form with T (the last one with
     beta in the last bytes of a nearly full allocation), the largest training set of each shape and its longest row, the
     row-block edges, a polytope of SX_MAX_M rows, and the status word;
  3. the saturating cost on the Taylor and the cautious trajectory at the three shapes and, output by output, at (2, 1) and
     (2, 2), with the parameters sat_loss does not otherwise see inside a rollout: (a) no angle, rank 1; (b) the angle first,
     full rank; (c) the angle last, rank 2 (rank 1 at n_s = 1);
  4. the saturating cost on the safety trajectory at (1, 1) and (4, 2), at the other shapes output by output and in one
     row-block, with costs (a) and (b); the streaming parents come from the one child process of
     tests/test_gpu_safety_sat.py.

Cases, inputs, launchers and tolerances are those of tests/test_gpu_perf_var.py (case() / inputs(): E = 2),
test_gpu_cautious.py, test_gpu_sat_cost.py, test_gpu_safety_sat.py and test_gpu_perf_shapes.py; P = 37 (three tiles, the
last one partial) unless stated.  Every limit and every flip is asked of sx_cem_cautious_rollout_form (on host-side models,
as tests/test_perf_var_host.py builds them), never computed here.  Tolerances: MEAN_TOL (rtol 1e-10, atol 1e-12) for rows,
means and the affine objective; SIGMA_TOL (rtol 1e-8, atol 1e-11) for sigma, cov and the variance objective; LOSS_TOL = 1e-12
per step against the oracle's cost of the kernel's own trajectory; TOL['rbf'] where the safety parent takes a resident form;
constraint costs and decisions exactly.  A pre-condition on the inputs is asserted on the oracle alone, before the GPU is
touched.  Every case prints its worst error as a fraction of the tolerance before it asserts.  Measured figures: DESIGN.md
section 3.14."""
import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

import safety_sat_oracle as sso
import sat_cost_oracle as so
import test_gpu_cautious as tc
import test_gpu_perf_multi as pm
import test_gpu_perf_shapes as ps
import test_gpu_perf_taylor_multi as ptm
import test_gpu_safety_sat as ss
import test_gpu_sat_cost as sc
from cautious_oracle import cautious_rollout, distances_at
from oracle import cem as ocem
from perf_taylor_oracle import perf_taylor_rollout
from safe_exploration_amd import _lib, cem_mpc
from safe_exploration_amd.costs import SaturatingCost
from test_gpu_cautious import EDGE, drawn_rows, placed_bounds, rows_inputs, with_bounds
from test_gpu_perf_taylor import MEAN_TOL, OUTPUTS as TAYLOR_OUTPUTS, tails
from test_gpu_perf_var import ABS, DEV, MODES, SIGMA_TOL, VAR, N_, T, case, close, inputs, worst
from test_gpu_safety_sat import streaming_parents  # noqa: F401  (the fixture: the one child process, started once)
from test_perf_var_host import _model as host_model
from test_sat_cost_host import random_weight

pytestmark = pytest.mark.gpu
SMALL, LARGE = 37, 4096 + 53
NEW = [(3, 1), (1, 1), (4, 2)]
ALL_SHAPES = [(2, 1), (3, 1), (4, 1), (2, 2), (4, 2), (1, 1)]
SIZES = [7, 200, 590]
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
LIMIT_P = 17       # two tiles, the second with one particle


def cautious_form(model, steps):
    return int(_lib.lib().sx_cem_cautious_rollout_form(ctypes.byref(model), steps))


def form_by_size(n_s, N):
    """All outputs in LDS at N = 7 and 200, and at 590 for one output; output by output at 590 for the other shapes."""
    return SX_FORM_BYOUT if N == 590 and n_s > 1 else SX_FORM_STREAM


# ---- 1: the cautious rollout at (3, 1), (1, 1), (4, 2) ------------------------------------------------------------------------
def decisions_of(refs):
    return np.concatenate([np.concatenate((ref.state_d.reshape(-1), ref.ctrl_d.reshape(-1))) for ref in refs])


def oracle_conditions(refs, steps, propagate, label):
    """On the oracle alone: some control leaves the box, no decision hangs on the rounding, the covariance is finite and
    (T > 2) the propagated part of diag G is not lost below the tolerance of diag G."""
    violations = sum(int(ref.ctrl_viol.sum()) for ref in refs)
    edge = float(np.abs(decisions_of(refs)).min())
    propagated = max(float((ref.sigma - ref.var).max()) for ref in refs)
    print(f'{label}: oracle: {violations} controls leave the box, decision closest to zero {edge:.3e}, largest propagated '
          f'part of diag G {propagated:.3e}, largest covariance entry {max(float(np.abs(ref.cov).max()) for ref in refs):.3e}')
    assert violations > 0, f'{label}: no control leaves the box'
    assert edge > EDGE, f'{label}: a decision hangs on the rounding'
    assert all(np.isfinite(ref.cov).all() for ref in refs), f'{label}: the oracle\'s covariance is not finite'
    if steps > 2 and propagate:
        assert propagated > 100 * SIGMA_TOL['atol'], label


_REFS = {}


def cautious_refs(n_s, n_u, N, steps, propagate, P=SMALL, seed=None):
    """(inputs, the oracle's cautious rollout per problem): computed once, shared by parts 1 to 3, left unchanged.  The seed
    is that of tests/test_gpu_cautious.py."""
    key = ('cautious', n_s, n_u, N, steps, propagate, P, seed)
    if key not in _REFS:
        gp, probs = case(n_s, n_u, N)[3:]
        inp = rows_inputs(n_s, n_u, P, steps, seed=n_s + 7 * n_u + N + P + 100 * steps if seed is None else seed)
        refs = [cautious_rollout(probs[VAR], gp, inp['x0'][e], rows, propagate) for e, rows in enumerate(drawn_rows(inp))]
        oracle_conditions(refs, steps, propagate, f'cautious ({n_s},{n_u}) N={N} P={P} T={steps} propagate={propagate}')
        _REFS[key] = (inp, refs)
    return _REFS[key]


def check_cautious(label, ssm, envs, probs, inp, refs, steps, propagate, want_form):
    """The body of test_gpu_cautious.test_kernel_matches_the_oracle for {mode: env}, {mode: problem} and the oracle's
    `refs`, after the form query has answered `want_form`.  Returns the drawn launch under the variance objective."""
    got = cautious_form(ssm.device_model, steps)
    assert got == want_form, f'{label}: form {got}, expected {want_form}'
    edge = float(np.abs(decisions_of(refs)).min())
    outs = {}
    for mode_name, mode in MODES.items():
        drawn = tc.launch(ssm, envs[mode], inp, steps, propagate=propagate)
        given = tc.launch(ssm, envs[mode], inp, steps, rows=drawn['rows'].clone(), propagate=propagate)
        for e, ref in enumerate(refs):
            want_obj = tc.oracle_objective(probs[mode], ref)
            obj_tol = SIGMA_TOL if mode == VAR else MEAN_TOL
            own = distances_at(probs[mode], inp['x0'][e], N_(drawn['rows'][e]), N_(drawn['traj'][e]), N_(drawn['cov'][e]))
            for name, out in (('drawn', drawn), ('given', given)):
                vs_oracle = float((np.abs(N_(out['margins'][e]) - ref.margins)
                                   / tc.sqrt_tolerance(ref.margins, **SIGMA_TOL)).max())
                print(f'{label} e={e} {mode_name} {name} (form {got}): of the tolerance: traj '
                      f'{worst(out["traj"][e], ref.traj, **MEAN_TOL):.2e}, diag G '
                      f'{worst(out["sigma"][e], ref.sigma, **SIGMA_TOL):.2e}, cov '
                      f'{worst(out["cov"][e], ref.cov, **SIGMA_TOL):.2e}, obj '
                      f'{worst(out["obj_cost"][e], want_obj, **obj_tol):.2e}, margins at the kernel\'s own outputs '
                      f'{worst(out["margins"][e], own, **MEAN_TOL):.2e}; margins against the oracle\'s: {vs_oracle:.2e} of '
                      f'SIGMA_TOL through the square root; decision closest to zero {edge:.3e}')
                close(out['rows'][e], ref.rows)
                close(out['traj'][e], ref.traj)
                close(out['sigma'][e], ref.sigma, **SIGMA_TOL)
                close(out['cov'][e], ref.cov, **SIGMA_TOL)
                close(out['obj_cost'][e], want_obj, **obj_tol)
                close(out['margins'][e], own)
                close(out['con_cost'][e], ref.con_cost, rtol=0, atol=0)
        for name in tc.OUTPUTS:
            assert torch.equal(drawn[name], given[name]), name                       # the two forms see the same bits
        assert torch.equal(drawn['cov'], drawn['cov'].transpose(-1, -2))              # symmetric to the bit
        if not propagate:
            assert torch.equal(drawn['cov'], torch.diag_embed(drawn['sigma']))
        outs[mode] = drawn
    for name in tc.OUTPUTS[:5] + ('con_cost',):
        assert torch.equal(outs[VAR][name], outs[ABS][name]), name                   # the mode changes the objective only
    return outs[VAR]


def check_default(n_s, n_u, N, steps, propagate, want_form, P=SMALL):
    """check_cautious with the case's own bounds."""
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    inp, refs = cautious_refs(n_s, n_u, N, steps, propagate, P)
    return check_cautious(f'cautious ({n_s},{n_u}) N={N} P={P} T={steps} propagate={propagate}', ssm, envs, probs, inp, refs,
                          steps, propagate, want_form)


@pytest.mark.parametrize('propagate', [True, False])
@pytest.mark.parametrize('steps', [1, 2, 8])
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('n_s,n_u', NEW)
def test_cautious_rollout_matches_the_oracle(n_s, n_u, N, steps, propagate):
    check_default(n_s, n_u, N, steps, propagate, form_by_size(n_s, N))


# (n_s, n_u, N, T, P, seed of the inputs): the first seed of 0, 1, ... for which placed_bounds' pre-conditions hold on the
# oracle, at P = 37 where one of 0 .. 59 does and at P = 149 otherwise (test_gpu_cautious.DECISION_CASES says why T = 2 is the
# hard one).
DECISION_CASES = [(3, 1, 7, 1, 37, 0), (3, 1, 7, 2, 37, 6), (3, 1, 7, 8, 37, 0),
                  (3, 1, 200, 1, 37, 0), (3, 1, 200, 2, 149, 17), (3, 1, 200, 8, 37, 4),
                  (1, 1, 7, 1, 37, 0), (1, 1, 7, 2, 37, 2), (1, 1, 7, 8, 37, 0),
                  (1, 1, 200, 1, 37, 0), (1, 1, 200, 2, 149, 3), (1, 1, 200, 8, 37, 2),
                  (4, 2, 7, 1, 37, 0), (4, 2, 7, 2, 37, 0), (4, 2, 7, 8, 37, 0),
                  (4, 2, 200, 1, 37, 0), (4, 2, 200, 2, 37, 11), (4, 2, 200, 8, 37, 0)]


@pytest.mark.parametrize('n_s,n_u,N,steps,P,seed', DECISION_CASES)
def test_cautious_decisions_exactly(n_s, n_u, N, steps, P, seed):
    """test_gpu_cautious.test_decisions_exactly, with its beta = 0 counter-run."""
    assert cautious_form(case(n_s, n_u, N)[0].device_model, steps) == SX_FORM_STREAM
    tc.test_decisions_exactly(n_s, n_u, N, steps, P, seed)


@pytest.mark.parametrize('steps', [2, 8])
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('n_s,n_u', NEW)
def test_cautious_against_the_taylor_and_the_variance_kernel(n_s, n_u, N, steps):
    """Bit for bit, as it is for the old shapes."""
    model = case(n_s, n_u, N)[0].device_model
    assert cautious_form(model, steps) == ps.form('taylor', model, steps) == form_by_size(n_s, N)
    tc.test_against_the_taylor_and_the_variance_kernel(n_s, n_u, N, steps)


@pytest.mark.parametrize('n_s,n_u,N,steps', [(3, 1, 590, 8), (1, 1, 200, 8), (4, 2, 590, 2)])
def test_cautious_tile_does_not_depend_on_the_grid(n_s, n_u, N, steps):
    assert cautious_form(case(n_s, n_u, N)[0].device_model, steps) == form_by_size(n_s, N)
    tc.test_a_tile_does_not_depend_on_the_grid(n_s, n_u, N, steps)


# ---- 2: the size limits of the cautious form ----------------------------------------------------------------------------------
# (n_s, n_u, N): (the last T with all outputs in LDS, the last T with any form), as the LDS arithmetic gives them
FLIPS = {(4, 2, 249): (5, 389), (3, 1, 346): (17, 721), (2, 1, 500): (69, 581)}


def walk_steps(model, stop=1 << 12):
    """The cautious form query's answers for T = 1, 2, ... up to the first refusal (exclusive)."""
    seq = []
    for steps in range(1, stop):
        f = cautious_form(model, steps)
        if f < 0:
            return seq
        seq.append(f)
    raise AssertionError(f'a form for every T below {stop}')


def placed(n_s, n_u, N, steps, P, seed):
    """The case with its bounds placed by test_gpu_cautious.placed_bounds on the inputs of `seed`:
    (inputs, {mode: problem}, {mode: env}, the oracle's rollouts under them)."""
    key = ('placed', n_s, n_u, N, steps, P, seed)
    if key not in _REFS:
        gp, probs = case(n_s, n_u, N)[3:]
        inp = rows_inputs(n_s, n_u, P, steps, seed=seed)
        prob, refs, h_vec, u = placed_bounds(probs, gp, inp)
        oracle_conditions(refs, steps, True, f'cautious, placed bounds ({n_s},{n_u}) N={N} P={P} T={steps}')
        _REFS[key] = (inp, prob, refs, h_vec, u)
    inp, prob, refs, h_vec, u = _REFS[key]
    envs, probs = case(n_s, n_u, N)[1], case(n_s, n_u, N)[4]
    placed_probs = {mode: dataclasses.replace(probs[mode], h_vec=prob.h_vec, u_min=prob.u_min, u_max=prob.u_max)
                    for mode in probs}
    return inp, placed_probs, {mode: with_bounds(envs[mode], h_vec=h_vec, u=u) for mode in envs}, refs


def decisions_equal(out, refs):
    """The sign of every margin is the oracle's (test_gpu_cautious.test_decisions_exactly)."""
    for e, ref in enumerate(refs):
        got = N_(out['margins'][e])
        assert np.array_equal(got[..., 0] >= 0, ref.state_viol) and np.array_equal(got[:, 1:, 1] >= 0, ref.ctrl_viol[:, 1:])
        assert np.array_equal(got[:, 0, 1] > 0, ref.ctrl_viol[:, 0])                 # the plain box at t = 0


FLIP_SEED = 0       # placed_bounds' pre-conditions hold on the oracle at P = 17 with the first seed, at all six launches


@pytest.mark.parametrize('side', ['last with all outputs in LDS', 'first output by output'])
@pytest.mark.parametrize('n_s,n_u,N', list(FLIPS))
def test_both_sides_of_the_flip_of_the_cautious_form_with_the_steps(n_s, n_u, N, side):
    """Walking T upward the query answers SX_FORM_STREAM, then SX_FORM_BYOUT, and changes exactly once, where and as
    sx_cem_perf_rollout_taylor_form does with n_perf = T; the launch on either side of the flip matches the oracle, with the
    bounds placed so that con_cost depends on beta.  At the last STREAM T the constants fill the allocation to its end and
    beta lies last in them: the beta = 0 launch is the beta = 0 oracle's and not the beta = 2 launch -- a beta read from
    beyond the allocation would be 0."""
    ssm = case(n_s, n_u, N)[0]
    seq = walk_steps(ssm.device_model)
    assert seq == walk_steps(host_model(n_s, n_u, N))                                # the query reads the sizes alone
    assert seq[1:] == ps.walk_n_perf('taylor', ssm.device_model)                     # (the Taylor entry starts at n_perf = 2)
    changes = [i for i in range(1, len(seq)) if seq[i] != seq[i - 1]]
    assert len(changes) == 1 and seq[0] == SX_FORM_STREAM and seq[-1] == SX_FORM_BYOUT, (changes, seq[0], seq[-1])
    last_stream, last = changes[0], len(seq)
    print(f'sx_cem_cautious_rollout ({n_s},{n_u}) N={N}: all outputs in LDS up to T = {last_stream}, output by output up to '
          f'{last} (derived: {FLIPS[(n_s, n_u, N)]})')
    assert (last_stream, last) == FLIPS[(n_s, n_u, N)]
    steps, want = (last_stream, SX_FORM_STREAM) if side.startswith('last') else (last_stream + 1, SX_FORM_BYOUT)
    inp, probs, envs, refs = placed(n_s, n_u, N, steps, LIMIT_P, FLIP_SEED)
    out = check_cautious(f'cautious, placed bounds ({n_s},{n_u}) N={N} P={LIMIT_P} T={steps}', ssm, envs, probs, inp, refs,
                         steps, True, want)
    decisions_equal(out, refs)
    if want == SX_FORM_STREAM:
        gp = case(n_s, n_u, N)[3]
        flat = tc.launch(ssm, with_bounds(envs[VAR], beta=0.0), inp, steps)
        compared = 0
        for e, rows in enumerate(drawn_rows(inp)):
            ref0 = cautious_rollout(dataclasses.replace(probs[VAR], beta=0.0), gp, inp['x0'][e], rows)
            if float(np.abs(decisions_of([ref0])).min()) > EDGE:
                close(flat['con_cost'][e], ref0.con_cost, rtol=0, atol=0)
                compared += 1
        assert compared > 0
        assert not torch.equal(flat['con_cost'], out['con_cost'])


# the largest N with a form at T = 2 and the longest row it admits, as the LDS arithmetic gives them: {(n_s, n_u): (N, T)}
DERIVED_LIMITS = {(2, 1): (988, 11), (3, 1): (907, 21), (4, 1): (842, 20), (2, 2): (939, 3), (4, 2): (809, 4),
                  (1, 1): (1021, 65)}
SEARCH_TO = 1200


def largest_n(n_s, n_u):
    sizes = [N for N in range(1, SEARCH_TO + 1) if cautious_form(host_model(n_s, n_u, N), 2) >= 0]
    assert sizes and sizes[-1] < SEARCH_TO and sizes == list(range(1, sizes[-1] + 1))   # one interval, inside the search
    return sizes[-1]


def refused_without_a_launch(ssm, env, n_s, n_u, steps):
    """The entry answers SX_ERR_UNSUPPORTED with obj_cost and the status word untouched; the wrapper raises 'no form'."""
    inp = rows_inputs(n_s, n_u, LIMIT_P, steps, seed=1)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.SxError, match='no form'):
        cem_mpc.cem_cautious_rollout(ssm, env, T(inp['x0']), steps, mean=T(inp['mean']), std=T(inp['std']),
                                     noise=T(inp['noise']), status=status)
    bufs = [T(inp[k]) for k in ('x0', 'mean', 'std', 'noise')]
    rows = torch.full((2, LIMIT_P, steps, n_u), float('nan'), dtype=torch.float64, device=DEV)
    obj, con = (torch.full((2, LIMIT_P), float('nan'), dtype=torch.float64, device=DEV) for _ in range(2))
    code = _lib.lib().sx_cem_cautious_rollout(ctypes.byref(ssm.device_model), ctypes.byref(env), 2, LIMIT_P, steps,
                                              *[_lib.ptr(b) for b in bufs + [rows, obj, con]], None, None, None, None, 1,
                                              _lib.ptr(status), _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert code == _lib.SX_ERR_UNSUPPORTED
    assert bool(torch.isnan(obj).all()) and bool(torch.isnan(con).all()) and bool(torch.isnan(rows).all())
    assert int(status.item()) == 0


@pytest.mark.parametrize('which', ['T = 2', 'the last T'])
@pytest.mark.parametrize('n_s,n_u', ALL_SHAPES)
def test_the_largest_model_of_a_shape_in_the_cautious_form(n_s, n_u, which):
    """The largest N the form query accepts at T = 2, built for real, at T = 2 and at the longest row the query still
    accepts, against the oracle; one point more, and one step more, have no form and are refused by the entry before any
    launch.  (1, 1) reaches n_pad = 1024 with its one output in LDS; every other shape ends output by output."""
    N = largest_n(n_s, n_u)
    ssm, envs = case(n_s, n_u, N)[:2]
    seq = walk_steps(ssm.device_model)
    last = len(seq)
    assert ssm.device_model.n_pad == host_model(n_s, n_u, N).n_pad and seq == walk_steps(host_model(n_s, n_u, N))
    print(f'sx_cem_cautious_rollout ({n_s},{n_u}): the largest N with a form {N}, n_pad {ssm.device_model.n_pad}, form '
          f'{seq[1]} at T = 2, the last T {last} (form {seq[-1]}); derived: {DERIVED_LIMITS[(n_s, n_u)]}')
    assert (N, last) == DERIVED_LIMITS[(n_s, n_u)]
    assert seq[-1] == (SX_FORM_STREAM if n_s == 1 else SX_FORM_BYOUT)
    assert cautious_form(ssm.device_model, last + 1) == -1 and cautious_form(host_model(n_s, n_u, N + 1), 2) == -1
    if which == 'T = 2':
        check_default(n_s, n_u, N, 2, True, seq[1], LIMIT_P)
        bigger = case(n_s, n_u, N + 1)
        refused_without_a_launch(bigger[0], bigger[1][VAR], n_s, n_u, 2)
    else:
        check_default(n_s, n_u, N, last, True, seq[-1], LIMIT_P)
        refused_without_a_launch(ssm, envs[VAR], n_s, n_u, last + 1)


@pytest.mark.parametrize('n_s,n_u,N', [(n_s, n_u, N) for n_s, n_u in ((3, 1), (4, 2)) for N in ps.block_edges(n_s, n_u)])
def test_cautious_rollout_at_the_row_block_edges(n_s, n_u, N):
    """N = 1, and n_pad = 16 | 32 and 32 | 48 with the last block full and just opened."""
    edges = ps.block_edges(n_s, n_u)
    assert case(n_s, n_u, N)[0].device_model.n_pad == {edges[0]: 16, edges[1]: 16, edges[2]: 32, edges[3]: 32, edges[4]: 48}[N]
    check_default(n_s, n_u, N, 8, True, SX_FORM_STREAM)


MOST_ROWS_SEED = 4      # the first seed of 0, 1, ... for which placed_bounds' pre-conditions hold on the oracle (0 .. 3: no
                        # control decision needs the spread)


def test_cautious_rollout_with_the_most_polytope_rows():
    """(3, 1), N = 200, T = 8 over SX_MAX_M unit normals, the common offset and the box placed by the method of
    test_gpu_cautious.placed_bounds: con_cost and the sign of every margin are the oracle's, and the deciding row is not
    always the same one."""
    n_s, n_u, N, steps, m = 3, 1, 200, 8, _lib.SX_MAX_M
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    h_mat = np.random.default_rng(50 + m).normal(size=(m, n_s))
    h_mat /= np.linalg.norm(h_mat, axis=1, keepdims=True)
    inp = rows_inputs(n_s, n_u, SMALL, steps, seed=MOST_ROWS_SEED)
    many = {VAR: dataclasses.replace(probs[VAR], h_mat=h_mat, h_vec=np.zeros((m, 1)))}
    prob, refs, h_vec, u = placed_bounds(many, gp, inp)
    assert len({int(np.argmax(ref.state_d[c, t])) for ref in refs for c in range(SMALL) for t in range(steps)}) > 1
    env = with_bounds(envs[VAR], m=m, h_vec=h_vec, u=u)
    _lib.fill(env.h_mat, h_mat)
    out = tc.launch(ssm, env, inp, steps)
    for e, ref in enumerate(refs):
        own = distances_at(prob, inp['x0'][e], N_(out['rows'][e]), N_(out['traj'][e]), N_(out['cov'][e]))
        print(f'(3,1) N=200 T=8 m={m} e={e}: margins at the kernel\'s own outputs '
              f'{worst(out["margins"][e], own, **MEAN_TOL):.2e} of the tolerance, {int(ref.state_viol.sum())} state and '
              f'{int(ref.ctrl_viol.sum())} control violations')
        close(out['margins'][e], own)
        close(out['con_cost'][e], ref.con_cost, rtol=0, atol=0)
    decisions_equal(out, refs)


@functools.lru_cache(maxsize=None)
def costs(n_s):
    """((name, SaturatingCost, its oracle twin), ...): (a) no angle, rank 1; (b) the angle at index 0, full rank n_s + 1;
    (c) the angle at index n_s - 1, rank 2 (rank 1 at n_s = 1)."""
    out = []
    for name, trig_idx, rank in (('a', None, 1), ('b', 0, n_s + 1), ('c', n_s - 1, 2 if n_s > 1 else 1)):
        rng = np.random.default_rng(79 + n_s)
        n_a = n_s + (trig_idx is not None)
        z = rng.normal(0, 0.4, n_a)
        w = random_weight(rng, n_a, rank) * 0.4
        cost = SaturatingCost(z, w, trig_idx)
        assert cost.rank == rank
        out.append((name, cost, so.Cost(z, w, trig_idx)))
    return tuple(out)


def cost_named(n_s, names):
    return [c for c in costs(n_s) if c[0] in names]


@pytest.mark.parametrize('sat', [False, True])
def test_a_nan_start_sets_the_cautious_status_word(sat):
    """(3, 1), N = 200, T = 2, the parent entry and _sat: a NaN in x0 of problem 1 sets SX_STATUS_NAN and leaves every
    obj_cost of problem 1 NaN -- a non-finite objective never ranks; problem 0 is the clean launch bit for bit, and with the
    value restored the clean launch is reproduced."""
    n_s, n_u, N, steps = 3, 1, 200, 2
    ssm, envs = case(n_s, n_u, N)[:2]
    cost = cost_named(n_s, 'b')[0][1] if sat else None
    inp = rows_inputs(n_s, n_u, SMALL, steps, seed=17)
    clean = sc.launch_cautious(ssm, envs[VAR], inp, steps, True, cost)            # asserts a clean status word
    x0 = T(inp['x0'])
    x0[1, n_s - 1] = float('nan')
    out = cem_mpc.cem_cautious_rollout(ssm, envs[VAR], x0, steps, want_traj=True, want_sigma=True, want_cov=True,
                                       want_margins=True, mean=T(inp['mean']), std=T(inp['std']), noise=T(inp['noise']),
                                       **({} if cost is None else dict(cost=cost)))
    torch.cuda.synchronize()
    assert int(out['status'].item()) & _lib.SX_STATUS_NAN
    assert bool(torch.isnan(out['obj_cost'][1]).all())
    for name in tc.OUTPUTS:
        assert bool(torch.isfinite(clean[name]).all()) or name == 'margins'
        assert torch.equal(out[name][0], clean[name][0]), name
    again = sc.launch_cautious(ssm, envs[VAR], inp, steps, True, cost)
    for name in tc.OUTPUTS:
        assert torch.equal(again[name], clean[name]), name


# ---- 3: the saturating cost on the Taylor and the cautious trajectory -----------------------------------------------------------
# (n_s, n_u, N, the costs): the new shapes with all three costs; the old shapes output by output with cost (b)
SAT_CASES = [(n_s, n_u, N, 'abc') for n_s, n_u in NEW for N in SIZES] + [(2, 1, 590, 'b'), (2, 2, 590, 'b')]


def spread_of(label, objective):
    """On the oracle alone: the objective tells the particles apart, and every loss is a loss."""
    assert np.isfinite(objective).all(), label
    print(f'{label}: oracle: objective in [{objective.min():.4f}, {objective.max():.4f}]')
    assert objective.max() - objective.min() > 1e-3, f'{label}: the objective does not tell the particles apart'
    return objective


def against_the_oracles_cost(label, obj, want):
    """(sc.check_objective asserts it; this prints the fraction to more digits.)"""
    print(f'{label}: obj_cost against the oracle\'s rollout: {worst(obj, want, **SIGMA_TOL):.2e} of SIGMA_TOL')


@pytest.mark.parametrize('propagate', [True, False])
@pytest.mark.parametrize('steps', [2, 8])
@pytest.mark.parametrize('n_s,n_u,N,names', SAT_CASES)
def test_cautious_sat_rollout(n_s, n_u, N, names, steps, propagate):
    """The body of test_gpu_sat_cost.test_cautious_sat_rollout under each cost."""
    ssm, envs = case(n_s, n_u, N)[:2]
    inp, refs = cautious_refs(n_s, n_u, N, steps, propagate)
    chosen = cost_named(n_s, names)
    label = lambda name, e: f'cautious ({n_s},{n_u}) N={N} T={steps} propagate={propagate} cost ({name}) e={e}'
    want = {(name, e): spread_of(label(name, e), so.trajectory_cost(twin, ref))
            for name, cost, twin in chosen for e, ref in enumerate(refs)}
    assert cautious_form(ssm.device_model, steps) == form_by_size(n_s, N)
    parent = sc.launch_cautious(ssm, envs[ABS], inp, steps, propagate)
    for name, cost, twin in chosen:
        sat = sc.launch_cautious(ssm, envs[ABS], inp, steps, propagate, cost)
        for field in tc.OUTPUTS:
            if field != 'obj_cost':
                assert torch.equal(parent[field], sat[field]), field
        assert torch.equal(sat['obj_cost'], sc.launch_cautious(ssm, envs[VAR], inp, steps, propagate, cost)['obj_cost'])
        if not propagate:
            assert torch.equal(sat['cov'], torch.diag_embed(sat['sigma']))      # the cost prices diag(var_t)
        for e, ref in enumerate(refs):
            against_the_oracles_cost(label(name, e), sat['obj_cost'][e], want[(name, e)])
            sc.check_objective(label(name, e), twin, sat['obj_cost'][e], sat['traj'][e], sat['cov'][e], ref, steps)


def taylor_refs(n_s, n_u, N, n_perf):
    """(inputs, the oracle's Taylor rollout per problem) with the seed of test_gpu_sat_cost.test_taylor_sat_rollout: the
    pre-condition (spread_of, under every cost of the case) holds on the oracle with it in every case of this file."""
    key = ('taylor', n_s, n_u, N, n_perf)
    if key not in _REFS:
        gp, probs = case(n_s, n_u, N)[3:]
        inp = inputs(n_s, n_u, SMALL, n_perf, 1, seed=n_s + 7 * n_u + N + n_perf)
        refs = [perf_taylor_rollout(probs[ABS], gp, inp['x0'][e], inp['safe'][e], tail, 1) for e, tail in enumerate(tails(inp))]
        assert all(np.isfinite(ref.cov).all() for ref in refs)
        _REFS[key] = (inp, refs)
    return _REFS[key]


@pytest.mark.parametrize('n_perf', [3, 15])
@pytest.mark.parametrize('n_s,n_u,N,names', SAT_CASES)
def test_taylor_sat_rollout(n_s, n_u, N, names, n_perf):
    """The body of test_gpu_sat_cost.test_taylor_sat_rollout under each cost, r = 1."""
    ssm, envs = case(n_s, n_u, N)[:2]
    inp, refs = taylor_refs(n_s, n_u, N, n_perf)
    chosen = cost_named(n_s, names)
    label = lambda name, e: f'taylor ({n_s},{n_u}) N={N} n_perf={n_perf} cost ({name}) e={e}'
    want = {(name, e): spread_of(label(name, e), so.trajectory_cost(twin, ref))
            for name, cost, twin in chosen for e, ref in enumerate(refs)}
    assert ps.form('taylor', ssm.device_model, n_perf) == form_by_size(n_s, N)
    parent = sc.launch_taylor(ssm, envs[ABS], inp, n_perf, 1)
    for name, cost, twin in chosen:
        sat = sc.launch_taylor(ssm, envs[ABS], inp, n_perf, 1, cost)
        for field in TAYLOR_OUTPUTS:
            if field != 'obj_cost':
                assert torch.equal(parent[field], sat[field]), field
        assert torch.equal(sat['obj_cost'], sc.launch_taylor(ssm, envs[VAR], inp, n_perf, 1, cost)['obj_cost'])
        for e, ref in enumerate(refs):
            against_the_oracles_cost(label(name, e), sat['obj_cost'][e], want[(name, e)])
            sc.check_objective(label(name, e), twin, sat['obj_cost'][e], sat['perf_traj'][e], sat['perf_cov'][e], ref, n_perf)


def launch_single_sat(ssm, env, inp, e, n_perf, cost):
    """Problem e of a multi-model case's inputs through the single-model entry."""
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = cem_mpc.cem_perf_rollout_taylor(ssm, env, T(inp['x0'][e:e + 1]), pm.H, n_perf, 1, status=status, want_sigma=True,
                                          want_cov=True, cost=cost, **pm._kw(inp, slice(e, e + 1), None))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


MULTI_SAT_CASES = ([(n_s, n_u, sizes) for n_s, n_u in NEW for sizes in (pm.SIZES, pm.SIZES_STREAM)]
                   + [(2, 1, (590, 200)), (2, 2, (590, 200))])


@pytest.mark.parametrize('n_perf', [3, 15])
@pytest.mark.parametrize('n_s,n_u,sizes', MULTI_SAT_CASES)
def test_taylor_sat_multi_rollout(n_s, n_u, sizes, n_perf):
    """The body of test_gpu_sat_cost.test_taylor_sat_multi_rollout under cost (b); every problem whose own form is the
    launch's is the single-model launch bit for bit."""
    ssms, envs, gps, probs = pm.case(n_s, n_u, sizes)
    (name, cost, twin), = cost_named(n_s, 'b')
    inp = pm.inputs(len(sizes), n_s, n_u, SMALL, n_perf, 1, seed=n_s + 7 * n_u + sum(sizes) + n_perf)
    refs = [perf_taylor_rollout(probs[ABS], gps[e], inp['x0'][e], inp['safe'][e], ptm.tail_of(inp, e), 1)
            for e in range(len(sizes))]
    label = lambda e: f'multi ({n_s},{n_u}) N={sizes} n_perf={n_perf} cost ({name}) e={e}'
    want = [spread_of(label(e), so.trajectory_cost(twin, ref)) for e, ref in enumerate(refs)]
    multi_form, own = ptm.forms(ssms, n_perf)
    assert own == [form_by_size(n_s, N) for N in sizes] and multi_form == max(own), (multi_form, own)
    parent, sat = sc.launch_multi(ssms, envs[ABS], inp, n_perf, 1), sc.launch_multi(ssms, envs[ABS], inp, n_perf, 1, cost)
    for field in TAYLOR_OUTPUTS:
        if field != 'obj_cost':
            assert torch.equal(parent[field], sat[field]), field
    for e, ref in enumerate(refs):
        against_the_oracles_cost(label(e), sat['obj_cost'][e], want[e])
        sc.check_objective(label(e), twin, sat['obj_cost'][e], sat['perf_traj'][e], sat['perf_cov'][e], ref, n_perf)
        if own[e] == multi_form:
            one = launch_single_sat(ssms[e], envs[ABS], inp, e, n_perf, cost)
            for field in TAYLOR_OUTPUTS:
                assert torch.equal(sat[field][e], one[field][0]), f'problem {e}: {field}'
    assert any(f == multi_form for f in own)      # something is compared bit for bit


@pytest.mark.parametrize('n_s,n_u,N,steps,name', [(3, 1, 590, 3, 'c'), (1, 1, 200, 15, 'a'), (4, 2, 200, 15, 'b'),
                                                  (4, 2, 590, 3, 'c')])
def test_sat_tile_does_not_depend_on_the_grid(n_s, n_u, N, steps, name):
    """test_gpu_sat_cost.test_a_tile_does_not_depend_on_the_grid: P = 4096 + 53 per problem; the first 37 particles of each
    problem in a launch of their own are bit-identical, for the three entries.  (4, 2) in both forms: the kernels with the
    most scratch."""
    ssm, envs = case(n_s, n_u, N)[:2]
    cost = cost_named(n_s, name)[0][1]
    assert ps.form('taylor', ssm.device_model, steps) == cautious_form(ssm.device_model, steps - 1) == form_by_size(n_s, N)
    inp = inputs(n_s, n_u, LARGE, steps, 1, seed=n_s + N)
    sub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in inp.items()}
    big, small = sc.launch_taylor(ssm, envs[ABS], inp, steps, 1, cost), sc.launch_taylor(ssm, envs[ABS], sub, steps, 1, cost)
    for field in TAYLOR_OUTPUTS:
        assert torch.equal(small[field], big[field][:, :SMALL]), field
    rows = {k: inp[k] for k in ('x0', 'mean', 'std', 'noise')}
    sub = dict(rows, noise=np.ascontiguousarray(rows['noise'][:, :SMALL]))
    big = sc.launch_cautious(ssm, envs[ABS], rows, steps - 1, True, cost)
    small = sc.launch_cautious(ssm, envs[ABS], sub, steps - 1, True, cost)
    for field in tc.OUTPUTS:
        assert torch.equal(small[field], big[field][:, :SMALL]), field
    ssms, menvs = pm.case(n_s, n_u, (N, 100))[:2]
    minp = pm.inputs(2, n_s, n_u, LARGE, steps, 1, seed=n_s + N)
    msub = {k: (v if k in ('x0', 'mean', 'std') else np.ascontiguousarray(v[:, :SMALL])) for k, v in minp.items()}
    big = sc.launch_multi(ssms, menvs[ABS], minp, steps, 1, cost)
    small = sc.launch_multi(ssms, menvs[ABS], msub, steps, 1, cost)
    for field in TAYLOR_OUTPUTS:
        assert torch.equal(small[field], big[field][:, :SMALL]), field


# ---- 4: the saturating cost on the safety trajectory ----------------------------------------------------------------------------
SAFETY_CASES = ss.MORE_CASES      # (1, 1) and (4, 2) at N = 7, 200, 590; (3, 1), (2, 2), (2, 1) at N = 7, 590


def safety_refs(n_s, n_u, N, horizon):
    """The inputs, after the pre-conditions of the drawn kind on the oracle's rollout of the rows mean + std * noise."""
    key = ('safety', n_s, n_u, N, horizon)
    if key not in _REFS:
        gp, probs = (case(n_s, n_u, N) if isinstance(N, int) else (None,) + pm.case(n_s, n_u, N))[3:]
        gps = [gp] * ss.E if isinstance(N, int) else gp
        inp = ss.inputs(n_s, n_u, SMALL, horizon, ss.seed_of(n_s, n_u, N, horizon))
        refs = [ocem.rollout(probs[ABS], gps[e], inp['x0'][e], inp['actions'][e]) for e in range(ss.E)]
        for e, ref in enumerate(refs):
            label = f'safety ({n_s},{n_u}) N={N} H={horizon} e={e}'
            assert ref.status == 0 and np.isfinite(ref.traj_p).all() and np.isfinite(ref.traj_q).all(), label
            print(f'{label}: oracle: {int((ref.con_cost > 0).sum())} of {SMALL} rows violate')
            assert (ref.con_cost > 0).any(), f'{label}: no row violates'
            for name, cost, twin in cost_named(n_s, 'ab'):
                spread_of(f'{label} cost ({name})', sso.safety_cost(twin, ref))
        _REFS[key] = inp
    return _REFS[key]


@pytest.mark.parametrize('horizon', [3, 15])
@pytest.mark.parametrize('n_s,n_u,N', SAFETY_CASES)
def test_safety_sat_rollout_against_the_parent_the_streaming_parent_and_the_oracle(streaming_parents, n_s, n_u, N, horizon):
    """The bodies of test_gpu_safety_sat.test_sat_rollout_against_the_parent_and_the_oracle and
    test_sat_rollout_equals_the_streaming_parent_bit_for_bit under costs (a) and (b)."""
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    inp = safety_refs(n_s, n_u, N, horizon)
    form = int(_lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), horizon))
    sat_form = int(_lib.lib().sx_cem_rollout_sat_form(ctypes.byref(ssm.device_model), horizon))
    exact = form in (SX_FORM_STREAM, SX_FORM_BYOUT)
    assert sat_form == form_by_size(n_s, N)
    parents = {kind: ss.launch(ssm, envs[ABS], inp, horizon, kind) for kind in ss.KINDS}
    streamed = {kind: dict(np.load(os.path.join(streaming_parents, f'{n_s}_{n_u}_{N}_{horizon}_{kind}.npz')))
                for kind in ss.KINDS}
    first = refs = None
    for name, cost, twin in cost_named(n_s, 'ab'):
        outs = {}
        for kind in ss.KINDS:
            sat = ss.launch(ssm, envs[ABS], inp, horizon, kind, cost)
            label = f'({n_s},{n_u}) N={N} H={horizon} cost ({name}) {kind} (parent form {form}, sat form {sat_form})'
            assert int(sat['status'].item()) == 0
            ss.assert_close_to_parent(label, parents[kind], sat, kind, n_s, exact)
            assert int(streamed[kind]['form']) == sat_form
            for field in ss.names_of(kind):
                assert np.array_equal(N_(sat[field]), streamed[kind][field]), f'{label}: {field} against the streaming parent'
            # obj_mode is not read: every output, the objective included, is the same under the variance objective
            other = ss.launch(ssm, envs[VAR], inp, horizon, kind, cost)
            for field in ss.names_of(kind) + ('obj_cost',):
                assert torch.equal(sat[field], other[field]), f'{label}: {field} depends on obj_mode'
            outs[kind] = sat
        # the drawn form stores the actions it rolled out, and the given form on those is the same rollout
        again = ss.launch(ssm, envs[ABS], dict(inp, actions=N_(outs['drawn']['actions'])), horizon, 'given', cost)
        for field in ('actions', 'traj', 'sigma', 'obj_cost', 'con_cost'):
            assert torch.equal(outs['drawn'][field], again[field]), field
        if first is None:       # the cost does not change the actions: one oracle rollout of the kernel's rows for both costs
            first = outs
            refs = {kind: [ocem.rollout(probs[ABS], gp, inp['x0'][e], N_(outs[kind]['actions'][e])) for e in range(ss.E)]
                    for kind in ('drawn', 'elites')}
        for kind in ('drawn', 'elites'):
            assert torch.equal(outs[kind]['actions'], first[kind]['actions'])
            for e in range(ss.E):
                ss.check_objective(f'({n_s},{n_u}) N={N} H={horizon} cost ({name}) {kind} e={e}', twin, outs[kind], e,
                                   refs[kind][e], horizon, n_s)


SAFETY_MULTI_CASES = [(1, 1, (200, 100)), (3, 1, (200, 100)), (4, 2, (200, 100)), (3, 1, (590, 200)), (4, 2, (590, 200))]


@pytest.mark.parametrize('horizon', [3, 15])
@pytest.mark.parametrize('n_s,n_u,sizes', SAFETY_MULTI_CASES)
def test_safety_sat_multi_rollout_against_the_parent_and_the_oracle(n_s, n_u, sizes, horizon):
    """The body of test_gpu_safety_sat.test_sat_multi_rollout_against_the_parent_and_the_oracle under costs (a) and (b)."""
    ssms, envs, gps, probs = pm.case(n_s, n_u, sizes)
    inp = safety_refs(n_s, n_u, sizes, horizon)
    fresh = lambda: torch.zeros(ss.E, dtype=torch.int32, device=DEV)
    refs = {}
    for name, cost, twin in cost_named(n_s, 'ab'):
        for kind in ss.KINDS:
            parent = ss.launch(ssms, envs[ABS], inp, horizon, kind, status=fresh())
            sat = ss.launch(ssms, envs[ABS], inp, horizon, kind, cost, fresh())
            label = f'multi ({n_s},{n_u}) N={sizes} H={horizon} cost ({name}) {kind}'
            assert sat['status'].tolist() == [0] * ss.E
            ss.assert_close_to_parent(label, parent, sat, kind, n_s, True)   # the multi entries have the streaming kernel only
            other = ss.launch(ssms, envs[VAR], inp, horizon, kind, cost, fresh())
            assert torch.equal(sat['obj_cost'], other['obj_cost'])
            if kind != 'given':
                if kind not in refs:      # the cost does not change the actions: one oracle rollout of them for both costs
                    refs[kind] = (sat['actions'], [ocem.rollout(probs[ABS], gps[e], inp['x0'][e], N_(sat['actions'][e]))
                                                   for e in range(ss.E)])
                assert torch.equal(sat['actions'], refs[kind][0])
                for e in range(ss.E):
                    ss.check_objective(f'{label} e={e}', twin, sat, e, refs[kind][1][e], horizon, n_s)
