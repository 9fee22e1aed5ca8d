"""GPU: Cautious MPC -- sx_cem_cautious_rollout against the numpy oracle (tests/cautious_oracle.py: the block-matrix
covariance step and lin_ellipsoid_safety_distance at c_safety = beta), its decisions exactly with the bounds placed by the
oracle, against the project's Taylor and variance kernels, its independence of the launch's grid, the entry's contract and
forms, CautiousCemMpc.solve against a numpy CEM, and CautiousCemMPC.get_action / do_rollout over a stub environment.

The cases are those of tests/test_gpu_perf_var.py (its case() / inputs(): E = 2, a non-zero feedback k_fb, beta = 2); shapes
(2, 1), (4, 1), (2, 2); N = 7 (one row-block), 200 (all outputs in LDS) and 590 (output by output); T in {1, 2, 8}; P = 37
(three tiles, the last one partial); drawn and given rows, both objective modes, propagate 1 and 0.  The other compiled
shapes -- (3, 1), (1, 1), (4, 2) -- and the size limits of the form at all six are in tests/test_gpu_cost_shapes.py, which
runs the bodies of this file's kernel tests.
Tolerances: rows, means and the affine objective rtol 1e-10, atol 1e-12; sigma (diag G), cov and the variance objective
SIGMA_TOL of test_gpu_perf_var.py; the margins against numpy distances at the kernel's own traj / cov rtol 1e-10, atol 1e-12;
con_cost exactly.  Every case prints its worst error as a fraction of the tolerance before it asserts.

Measured figures: DESIGN.md section 3.11."""
import ctypes
import dataclasses
from unittest import mock

import numpy as np
import pytest
import torch

from cautious_oracle import cautious_rollout, cem_solve_cautious, distances_at
from oracle import cem as ocem
from safe_exploration_amd import _lib, cem_mpc, problems
from test_gpu_perf_taylor import MEAN_TOL
from test_gpu_perf_var import ABS, DEV, MODES, SIGMA_TOL, SOLVE, VAR, N_, T, case, close, decided, inputs, pendulum, worst

pytestmark = pytest.mark.gpu
SMALL, LARGE = 37, 4096 + 53
SHAPES = [(2, 1), (4, 1), (2, 2)]
SIZES = [7, 200, 590]
STEPS = [1, 2, 8]
OUTPUTS = ('rows', 'traj', 'sigma', 'cov', 'margins', 'obj_cost', 'con_cost')
EDGE = 1e-9      # no decision of an oracle comparison lies this close to zero


def rows_inputs(n_s, n_u, P, steps, seed):
    """x0, mean, std, noise of test_gpu_perf_var.inputs for rows of `steps` controls."""
    inp = inputs(n_s, n_u, P, steps + 1, 1, seed)
    return {k: inp[k] for k in ('x0', 'mean', 'std', 'noise')}


def drawn_rows(inp):
    return [inp['mean'][e][None] + inp['std'][e][None] * inp['noise'][e] for e in range(2)]


def launch(ssm, env, inp, steps, rows=None, propagate=True):
    """The drawn form, or with `rows` the given form, with every output."""
    kw = dict(mean=T(inp['mean']), std=T(inp['std']), noise=T(inp['noise'])) if rows is None else dict(rows=rows)
    out = cem_mpc.cem_cautious_rollout(ssm, env, T(inp['x0']), steps, propagate=propagate, want_traj=True, want_sigma=True,
                                       want_cov=True, want_margins=True, **kw)
    torch.cuda.synchronize()
    assert int(out['status'].item()) == 0
    return out


def with_bounds(env, h_vec=None, u=None, m=None, beta=None):
    env = _lib.SxEnv.from_buffer_copy(env)
    if m is not None:
        env.m = m
    if h_vec is not None:
        for j in range(env.m):
            env.h_vec[j] = h_vec
    if u is not None:
        for c in range(env.n_u):
            env.u_min[c], env.u_max[c] = -u, u
    if beta is not None:
        env.beta = beta
    return env


def oracle_objective(prob, ref):
    return sum(ocem.objective_cost(prob, ref.traj[:, t], ref.sigma[:, t]) for t in range(ref.traj.shape[1]))


def sqrt_tolerance(d, rtol, atol):
    """SIGMA_TOL pushed through the square root of a distance's quadratic form, for a spread of about |d|: the figure the
    oracle comparison of the margins is printed against."""
    q = np.maximum(np.abs(d), 1e-3) ** 2
    return (atol + rtol * q) / (2.0 * np.sqrt(q))


# ---- against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('propagate', [True, False])
@pytest.mark.parametrize('steps', STEPS)
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_kernel_matches_the_oracle(n_s, n_u, N, steps, propagate):
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    inp = rows_inputs(n_s, n_u, SMALL, steps, seed=n_s + 7 * n_u + N + SMALL + 100 * steps)
    refs = [cautious_rollout(probs[VAR], gp, inp['x0'][e], rows, propagate) for e, rows in enumerate(drawn_rows(inp))]
    assert sum(int(ref.ctrl_viol.sum()) for ref in refs) > 0, 'no control leaves the box'
    edge = min(float(np.abs(np.concatenate((ref.state_d.reshape(-1), ref.ctrl_d.reshape(-1)))).min()) for ref in refs)
    assert edge > EDGE, 'a decision hangs on the rounding'
    if steps > 2 and propagate:
        assert max(float((ref.sigma - ref.var).max()) for ref in refs) > 100 * SIGMA_TOL['atol']
    outs = {}
    for mode_name, mode in MODES.items():
        drawn = launch(ssm, envs[mode], inp, steps, propagate=propagate)
        given = launch(ssm, envs[mode], inp, steps, rows=drawn['rows'].clone(), propagate=propagate)
        for e, ref in enumerate(refs):
            want_obj = oracle_objective(probs[mode], ref)
            obj_tol = SIGMA_TOL if mode == VAR else MEAN_TOL
            own = distances_at(probs[mode], inp['x0'][e], N_(drawn['rows'][e]), N_(drawn['traj'][e]), N_(drawn['cov'][e]))
            for name, out in (('drawn', drawn), ('given', given)):
                vs_oracle = float((np.abs(N_(out['margins'][e]) - ref.margins)
                                   / sqrt_tolerance(ref.margins, **SIGMA_TOL)).max())
                print(f'({n_s},{n_u}) N={N} T={steps} propagate={propagate} e={e} {mode_name} {name}: of the tolerance: traj '
                      f'{worst(out["traj"][e], ref.traj, **MEAN_TOL):.3f}, diag G '
                      f'{worst(out["sigma"][e], ref.sigma, **SIGMA_TOL):.3f}, cov '
                      f'{worst(out["cov"][e], ref.cov, **SIGMA_TOL):.3f}, obj '
                      f'{worst(out["obj_cost"][e], want_obj, **obj_tol):.3f}, margins at the kernel\'s own outputs '
                      f'{worst(out["margins"][e], own, **MEAN_TOL):.3f}; margins against the oracle\'s: {vs_oracle:.3f} of '
                      f'SIGMA_TOL through the square root; decision closest to zero {edge:.3e}')
                close(out['rows'][e], ref.rows)
                close(out['traj'][e], ref.traj)
                close(out['sigma'][e], ref.sigma, **SIGMA_TOL)
                close(out['cov'][e], ref.cov, **SIGMA_TOL)
                close(out['obj_cost'][e], want_obj, **obj_tol)
                close(out['margins'][e], own)
                close(out['con_cost'][e], ref.con_cost, rtol=0, atol=0)
        for name in OUTPUTS:
            assert torch.equal(drawn[name], given[name]), name                       # the two forms see the same bits
        assert torch.equal(drawn['cov'], drawn['cov'].transpose(-1, -2))              # symmetric to the bit
        if not propagate:
            assert torch.equal(drawn['cov'], torch.diag_embed(drawn['sigma']))
        outs[mode] = drawn
    for name in OUTPUTS[:5] + ('con_cost',):
        assert torch.equal(outs[VAR][name], outs[ABS][name]), name                   # the mode changes the objective only


# ---- decisions, exactly -----------------------------------------------------------------------------------------------------
def widest_gap(values):
    """(offset, gap): the middle of the widest gap between neighbours inside the middle half of the sorted values."""
    order = np.sort(values)
    lo, hi = len(order) // 4, 3 * len(order) // 4
    i = lo + int(np.argmax(np.diff(order[lo:hi + 1])))
    return 0.5 * (order[i] + order[i + 1]), order[i + 1] - order[i]


def placed_bounds(probs, gp, inp, propagate=True):
    """The method of test_terminal_safety on every step: the oracle's largest state distance with h_vec = 0 and its control
    values |k_ff_t[c]| + beta sqrt(K_c Sigma_t K_c^T), each pooled over (problem, particle, step); the common h_vec and
    the symmetric box in the widest gap of the middle half.  Asserts the pre-conditions on the oracle; returns (problem,
    references, h_vec, u)."""
    m = probs[VAR].h_mat.shape[0]
    zero = dataclasses.replace(probs[VAR], h_vec=np.zeros((m, 1)))
    free = [cautious_rollout(zero, gp, inp['x0'][e], rows, propagate) for e, rows in enumerate(drawn_rows(inp))]
    state = np.concatenate([r.state_d.max(axis=2).reshape(-1) for r in free])
    ctrl = np.concatenate([(np.abs(r.rows) + r.spread).max(axis=2).reshape(-1) for r in free])
    (h_vec, gap_s), (u, gap_u) = widest_gap(state), widest_gap(ctrl)
    prob = dataclasses.replace(probs[VAR], h_vec=np.full((m, 1), h_vec), u_min=np.full(zero.n_u, -u), u_max=np.full(zero.n_u, u))
    refs = [cautious_rollout(prob, gp, inp['x0'][e], rows, propagate) for e, rows in enumerate(drawn_rows(inp))]
    d_state = np.concatenate([r.state_d.max(axis=2).reshape(-1) for r in refs])
    d_ctrl = np.concatenate([r.ctrl_d.max(axis=2).reshape(-1) for r in refs])
    n_state, n_ctrl = int((d_state >= 0).sum()), sum(int(r.ctrl_viol.sum()) for r in refs)
    print(f'h_vec {h_vec:.6e} (gap {gap_s:.3e}, {n_state} of {len(d_state)} violate), u {u:.6e} (gap {gap_u:.3e}, {n_ctrl} of '
          f'{len(d_ctrl)} violate), largest spread {max(float(r.spread.max()) for r in refs):.3e}')
    assert gap_s > 1e-6 and gap_u > 1e-6
    assert float(np.abs(d_state).min()) >= 0.5 * gap_s * (1 - 1e-9) and float(np.abs(d_ctrl).min()) >= 0.5 * gap_u * (1 - 1e-9)
    for n, pool in ((n_state, d_state), (n_ctrl, d_ctrl)):
        assert len(pool) // 4 <= n <= 3 * len(pool) // 4 + 1
    if inp['noise'].shape[2] >= 2:
        # a kernel that drops the spread would not pass: some decision of either kind needs it
        flat = [cautious_rollout(dataclasses.replace(prob, beta=0.0), gp, inp['x0'][e], rows, propagate)
                for e, rows in enumerate(drawn_rows(inp))]
        assert any((a.ctrl_viol != b.ctrl_viol).any() for a, b in zip(refs, flat)), 'no control decision needs the spread'
        assert any((a.state_viol != b.state_viol).any() for a, b in zip(refs, flat)), 'no state decision needs the spread'
    return prob, refs, h_vec, u


# (n_s, n_u, N, T, P, seed of the inputs).  The pre-conditions are the oracle's alone, so the seed is the first of 0, 1, ...
# for which they hold.  P = 37 except for (2, 1) at T = 2: a control decision needs the spread only where some
# |k_ff_1| + spread lies within the spread of the bound, the bound sits in the widest gap of 2 P T pooled values, and this
# shape's feedback row is small (|K| <= 0.08 at N = 7: spreads of 0.01 at t = 1) -- at P = 37 half the widest gap of 148
# values exceeds every spread (no seed in 0 .. 199 passes); at P = 149 (ten tiles, the last one partial) it does not.
DECISION_CASES = [(2, 1, 7, 1, 37, 0), (2, 1, 7, 2, 149, 2), (2, 1, 7, 8, 37, 94), (2, 1, 200, 1, 37, 0),
                  (2, 1, 200, 2, 149, 2), (2, 1, 200, 8, 37, 1), (4, 1, 7, 1, 37, 0), (4, 1, 7, 2, 37, 0), (4, 1, 7, 8, 37, 0),
                  (2, 2, 7, 1, 37, 0), (2, 2, 7, 2, 37, 21), (2, 2, 7, 8, 37, 0)]


@pytest.mark.parametrize('n_s,n_u,N,steps,P,seed', DECISION_CASES)
def test_decisions_exactly(n_s, n_u, N, steps, P, seed):
    ssm, envs, spec, gp, probs = case(n_s, n_u, N)
    inp = rows_inputs(n_s, n_u, P, steps, seed=seed)
    prob, refs, h_vec, u = placed_bounds(probs, gp, inp)
    env = with_bounds(envs[VAR], h_vec=h_vec, u=u)
    out = launch(ssm, env, inp, steps)
    for e, ref in enumerate(refs):
        close(out['con_cost'][e], ref.con_cost, rtol=0, atol=0)
        got = N_(out['margins'][e])
        assert np.array_equal(got[..., 0] >= 0, ref.state_viol) and np.array_equal(got[:, 1:, 1] >= 0, ref.ctrl_viol[:, 1:])
        assert np.array_equal(got[:, 0, 1] > 0, ref.ctrl_viol[:, 0])                 # the plain box at t = 0
    if steps >= 2:
        # and the kernel reads beta: without it the counts are the oracle's without it
        flat = launch(ssm, with_bounds(env, beta=0.0), inp, steps)
        for e, rows in enumerate(drawn_rows(inp)):
            ref0 = cautious_rollout(dataclasses.replace(prob, beta=0.0), gp, inp['x0'][e], rows)
            edge = float(np.abs(np.concatenate((ref0.state_d.reshape(-1), ref0.ctrl_d.reshape(-1)))).min())
            if edge > EDGE:
                close(flat['con_cost'][e], ref0.con_cost, rtol=0, atol=0)
        assert not torch.equal(flat['con_cost'], out['con_cost'])


# ---- against the project's other kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [2, 8])
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_against_the_taylor_and_the_variance_kernel(n_s, n_u, N, steps):
    """Without polytope rows and with a box no action leaves: traj, sigma and cov are sx_cem_perf_rollout_taylor's with
    H = r = 1, n_perf = T, bit for bit; propagate = 0 carries sx_cem_perf_rollout_var's variances."""
    ssm, envs = case(n_s, n_u, N)[:2]
    inp = rows_inputs(n_s, n_u, SMALL, steps, seed=17 + n_s + N + steps)
    env = with_bounds(envs[VAR], m=0, u=1e6)
    out = launch(ssm, env, inp, steps)
    assert bool((out['con_cost'] == 0).all()) and bool(torch.isneginf(out['margins'][..., 0]).all())
    E, P = 2, SMALL

    def perf(wrapper, **kw):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        obj = torch.full((E, P), float('nan'), dtype=torch.float64, device=DEV)
        rows = out['rows'].clone()
        rows[:, :, :1] = float('nan')                        # the safety part of the rows is an output
        r = wrapper(ssm, env, T(inp['x0']), 1, steps, 1, safe_actions=out['rows'][:, :, :1].contiguous(), obj_cost=obj,
                    con_cost=torch.zeros((E, P), dtype=torch.float64, device=DEV), status=status, rows=rows, want_traj=True,
                    want_sigma=True, **kw)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        return r

    tay = perf(cem_mpc.cem_perf_rollout_taylor, want_cov=True)
    assert torch.equal(tay['rows'], out['rows'])
    for mine, theirs in (('traj', 'perf_traj'), ('sigma', 'perf_sigma'), ('cov', 'perf_cov'), ('obj_cost', 'obj_cost')):
        assert torch.equal(out[mine], tay[theirs]), mine
    var = perf(cem_mpc.cem_perf_rollout_var)
    me = launch(ssm, env, inp, steps, propagate=False)
    assert torch.equal(me['traj'], var['perf_traj']) and torch.equal(me['sigma'], var['perf_sigma'])
    assert torch.equal(me['cov'], torch.diag_embed(me['sigma'])) and torch.equal(me['obj_cost'], var['obj_cost'])
    assert torch.equal(me['traj'], out['traj']) and not torch.equal(me['sigma'], out['sigma'])


# ---- the grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u,N,steps', [(2, 1, 200, 8), (4, 1, 590, 8), (2, 2, 7, 2)])
def test_a_tile_does_not_depend_on_the_grid(n_s, n_u, N, steps):
    """P = 4096 + 53 per problem; the first 37 particles of each problem in a launch of their own are bit-identical."""
    ssm, envs = case(n_s, n_u, N)[:2]
    inp = rows_inputs(n_s, n_u, LARGE, steps, seed=n_s + N)
    sub = dict(inp, noise=np.ascontiguousarray(inp['noise'][:, :SMALL]))
    env = with_bounds(envs[ABS], h_vec=0.06, u=0.5)
    for propagate in (True, False):
        big, small = launch(ssm, env, inp, steps, propagate=propagate), launch(ssm, env, sub, steps, propagate=propagate)
        assert bool((big['con_cost'] > 0).any())
        for name in OUTPUTS:
            assert torch.equal(small[name], big[name][:, :SMALL]), name


# ---- the entry's contract and the forms ------------------------------------------------------------------------------------
def test_the_entry_answers_before_any_launch():
    """Every pointer is one that would fault if read: the answers come from the host."""
    ssm, envs = case(2, 1, 200)[:2]
    model, env = ssm.device_model, envs[VAR]
    p = lambda v: None if v is None else ctypes.c_void_p(v)

    def call(model=model, env=env, E=2, P=SMALL, steps=8, x0=16, mean=16, std=16, noise=16, rows=16, obj=16, con=16, status=16):
        return _lib.lib().sx_cem_cautious_rollout(None if model is None else ctypes.byref(model),
                                                  None if env is None else ctypes.byref(env), E, P, steps, p(x0), p(mean),
                                                  p(std), p(noise), p(rows), p(obj), p(con), None, None, None, None, 1,
                                                  p(status), _lib.stream_ptr(torch.device(DEV)))

    for kw in (dict(x0=None), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None), dict(mean=None),
               dict(std=None), dict(E=0), dict(P=0), dict(steps=0), dict(model=None), dict(env=None),
               dict(env=case(2, 2, 7)[1][VAR]), dict(env=with_bounds(env, m=-1))):
        assert call(**kw) == _lib.SX_ERR_ARG, kw
    bad_mode = _lib.SxEnv.from_buffer_copy(env)
    bad_mode.obj_mode = 7
    assert call(env=bad_mode) == _lib.SX_ERR_ARG
    unpacked = _lib.SxGpModel.from_buffer_copy(model)
    unpacked.a_pack = None
    assert call(model=unpacked) == _lib.SX_ERR_ARG
    assert call(env=with_bounds(env, m=_lib.SX_MAX_M + 1)) == _lib.SX_ERR_UNSUPPORTED
    assert call(model=case(2, 1, 1100)[0].device_model) == _lib.SX_ERR_UNSUPPORTED
    torch.cuda.synchronize()


def test_the_forms_the_training_sets_take():
    form = lambda ssm, steps=8: int(_lib.lib().sx_cem_cautious_rollout_form(ctypes.byref(ssm.device_model), steps))
    SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3
    for n_s, n_u in SHAPES:
        assert form(case(n_s, n_u, 590)[0]) == SX_FORM_BYOUT
        assert form(case(n_s, n_u, 200)[0]) == SX_FORM_STREAM
        assert form(case(n_s, n_u, 7)[0], 1) == SX_FORM_STREAM
    ssm, envs = case(2, 1, 1100)[:2]
    assert form(ssm, 2) < 0
    with pytest.raises(_lib.SxError, match='no form'):
        launch(ssm, envs[VAR], rows_inputs(2, 1, SMALL, 2, seed=1), 2)
    with pytest.raises(ValueError, match='T'):
        launch(case(2, 1, 7)[0], envs[VAR], rows_inputs(2, 1, SMALL, 1, seed=1), 0)


# ---- the whole solve -------------------------------------------------------------------------------------------------------
CAUTIOUS_SOLVE = dict(T=6, P=SOLVE['P'], k=SOLVE['k'], iters=SOLVE['iters'], init_std=SOLVE['init_std'], seed=SOLVE['seed'])


def solve_problem():
    """The pendulum of test_gpu_perf_var.pendulum() with the chance constraints on its safe polytope."""
    spec, gp = pendulum()
    return spec, gp, problems.oracle_problem(spec, ocem)


@pytest.mark.parametrize('propagate', [True, False])
def test_solve_matches_the_numpy_cem(propagate):
    """The conditions under which the comparison means something are asserted on the ORACLE's values before the GPU is
    touched: every iteration's elite boundary and the final best row pass decided()."""
    from safe_exploration_amd.cem_mpc import CautiousCemMpc
    c = CAUTIOUS_SOLVE
    spec, gp, prob = solve_problem()
    assert prob.obj_mode == ocem.OBJ_NEG_VARIANCE
    noise = np.random.default_rng(c['seed']).normal(size=(c['iters'], c['P'], c['T'], 1))
    x0 = np.array([0.02, -0.03])
    ref_best, trace = cem_solve_cautious(prob, gp, x0, noise, c['k'], c['init_std'], propagate)
    assert ref_best is not None, 'the oracle\'s last iteration does not end feasible'
    assert any((con > 0).any() for con, _, _, _ in trace), 'no constraint is ever active'
    for it, (con, obj, idx, var_min) in enumerate(trace):
        order = ocem.rank(con, obj, c['k'] + 1)
        assert var_min > 0
        assert decided(con, obj, order[-2], order[-1]), f'iteration {it}: the elite set hangs on the tolerance'
    con, obj, idx, _ = trace[-1]
    order = ocem.rank(con, obj, 2)
    assert decided(con, obj, order[0], order[1]), 'the best row hangs on the tolerance: choose another seed'
    ssm, env = problems.build(spec, device=DEV)
    mpc = CautiousCemMpc(ssm, env, c['T'], c['P'], c['k'], c['iters'], device=DEV, init_std=c['init_std'],
                         propagate=propagate, record_rollouts=True)
    best, ok, history, status = mpc.solve(T(x0[None]), noise=T(noise[:, None]))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and len(history) == c['iters']
    assert bool(ok[0].item()) == (ref_best is not None)
    for it, (h, (con, obj, idx, _)) in enumerate(zip(history, trace)):
        print(f'iteration {it}: objective {worst(h.objective_costs, obj, **SIGMA_TOL):.3f} of the tolerance, '
              f'{int((con > 0).sum())} of {len(con)} rows violate')
        close(h.constraint_costs, con, rtol=0, atol=0)
        close(h.objective_costs, obj, **SIGMA_TOL)
        assert tuple(h.perf_cov.shape) == (c['P'], c['T'], 2, 2)
        assert set(ocem.rank(N_(h.constraint_costs), N_(h.objective_costs), c['k'])) == set(idx)
    print(f'best row: max |device - numpy CEM| = {float(np.abs(N_(best[0]) - ref_best).max()):.3e}')
    close(best[0], ref_best, rtol=0, atol=1e-9)


# ---- the class ----------------------------------------------------------------------------------------------------------------
class Conf:
    T = 5
    beta_safety = 2.0
    type_perf_traj = 'taylor'
    cem_num_rollouts = 512
    cem_num_elites = 50
    cem_num_iterations = 4
    cem_init_std = 0.2
    plot_cem_optimisation = False
    device = DEV
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'


def make_cautious(spec, conf, env=None, **opt):
    """A CautiousCemMPC over the spec's GP and constants, the way problems.make_solver builds a CemSafeMPC."""
    from safe_exploration_amd.cautious_mpc import CautiousCemMPC
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    env = env if env is not None else problems.StubEnv(spec, np.zeros(spec.n_s))
    ssm = GpCemSSM(conf, spec.n_s, spec.n_u)
    ssm.set_hyperparameters(spec.lengthscale, spec.outputscale, spec.noise)
    lqr = mock.Mock()
    lqr.get_control_matrix.return_value = spec.k_fb
    opt_env = dict({'lin_model': (spec.a, spec.b), 'ctrl_bounds': np.stack((spec.u_min, spec.u_max), axis=1),
                    'h_mat_safe': spec.h_mat, 'h_safe': spec.h_vec, 'h_mat_obs': None, 'h_obs': None}, **opt)
    solver = CautiousCemMPC(ssm, env, conf, opt_env, None, None, beta_safety=None, safe_policy=None, lqr=lqr)
    y = spec.Y + spec.X[:, :spec.n_s] @ spec.a.T + spec.X[:, spec.n_s:] @ spec.b.T
    solver.update_model(spec.X, y, opt_hyp=False, replace_old=True)
    return solver, env


def test_get_action_the_ladder_and_the_warm_start():
    from safe_exploration_amd.safempc_cem import MpcResult
    spec = problems.pendulum(n_train=200, seed=0)
    env = problems.StubEnv(spec, np.zeros(2))                       # no objective: the solver explores
    safe = type('C', (Conf,), dict(cautious_state_polytope='safe'))()
    solver, _ = make_cautious(spec, safe, env)
    x = np.array([0.02, -0.03])
    action, result, means, covs, row, margins = solver.get_action_verbose(x)
    mpc = solver._solver()
    assert result == MpcResult.FOUND_SOLUTION and action.shape == (1,) and solver.n_fail == 0 and mpc.last_status == 0
    assert mpc._env.m == spec.h_mat.shape[0] and mpc._env.obj_mode == VAR and mpc._env.beta == 2.0 and mpc._propagate
    assert means.shape == (6, 2) and covs.shape == (5, 2, 2) and row.shape == (5, 1) and margins.shape == (5, 2)
    assert np.array_equal(means[0], x) and np.array_equal(row[0], action) and bool((margins < 0).all())
    assert bool((np.abs(row) <= 1.0).all())
    kept = solver.k_ff_old.copy()
    # the second solve starts from the shifted row
    with mock.patch.object(mpc, 'get_actions', wraps=mpc.get_actions) as spy:
        action, result = solver.get_action(x)
    assert result == MpcResult.FOUND_SOLUTION
    np.testing.assert_array_equal(N_(spy.call_args[1]['init_mean'])[0], np.vstack((kept[1:], kept[-1:])))
    kept = solver.k_ff_old.copy()
    # bounds nobody can meet: the kept row's entries 1, 2, ..., then k_fb x
    solver.ctrl_bounds = np.array([[1.0, -1.0]])
    mpc.set_env(solver._build_env()[0])
    for n in range(1, Conf.T):
        action, result = solver.get_action(x)
        assert result == MpcResult.PREVIOUS_SOLUTION and np.array_equal(action, kept[n]) and solver.n_fail == n
    action, result = solver.get_action(x)
    assert result == MpcResult.SAFE_CONTROLLER and np.array_equal(action, spec.k_fb @ x)
    assert solver.get_action_verbose(x)[2:] == (None, None, None, None)
    # the reference's polytope: the pendulum has no obstacle rows
    obs, _ = make_cautious(spec, Conf(), env)
    assert obs._solver()._env.m == 0
    rows = dict(h_mat_obs=spec.h_mat[:1], h_obs=spec.h_vec[:1])
    assert make_cautious(spec, Conf(), env, **rows)[0]._solver()._env.m == 1


def test_do_rollout_runs_with_the_solver():
    from safe_exploration_amd.episode_runner import do_rollout
    from safe_exploration_amd.safempc_cem import MpcResult
    spec = problems.pendulum(n_train=200, seed=0, obj_mode=ABS)
    env = problems.StubEnv(spec, np.array([0.02, -0.03]), never_done=True, objective_target=-0.1)
    solver, _ = make_cautious(spec, type('C', (Conf,), dict(type_perf_traj='mean_equivalent'))(), env)
    xx, yy, cc, codes, failed = do_rollout(env, 3, solver=solver)
    assert codes.shape == (3, 1) and not failed and xx.shape == (2, 3) and env.steps == 3
    assert not solver._solver()._propagate and solver._solver()._env.obj_mode == ABS
    assert solver._batch_fail == [0] and (codes == 1).all()
