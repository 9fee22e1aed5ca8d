"""GPU: the max-variance subset selection (sx_gp_select, GpCemSSM.select_subset, conf.cem_gp_subset_size,
update_models_multi) against the from-the-definition oracle of tests/subset_reference.py.

What decides a greedy step is the gap between the best and the second-best candidate; tests/test_subset_select_host.py
shows that on every case here that gap is at least 1e-9 x sum_d (s_d + noise_d).  The kernel's sel_var must be within a
TENTH of that (1e-10 x the prior) of the float64 oracle, so an error of the size allowed cannot flip a choice, and the
indices must be the oracle's exactly.  Where the long-double oracle reaches (n <= 200, m <= 64) the project's rule
applies too: e_kernel <= 32 x max(e_ref, 8 eps), e = max|q - q_ld| / max|q_ld|.

A workgroup of the kernel owns 64 pool rows (subset_reference.CASES says what each size covers).  Every output buffer
and the workspace end in a canary of 64 words, and every test checks them.  Each check prints its figures before it
asserts (`pytest -s`): DESIGN.md section 3.5 records the worst of them."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import subset_reference as S
import warm_path_reference as R
from safe_exploration_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = 64
FACTOR = 32.0
FLOOR = 8 * R.EPS
NOT_PD = _lib.SX_STATUS_NOT_PD


class Buf:
    """An output buffer of `shape` with CANARY words after its end: NaN (float64) or a fill value (int32) all over,
    then a fixed bit pattern in the canary."""

    def __init__(self, *shape, dtype=torch.float64, fill=0):
        n = int(np.prod(shape))
        self.whole = torch.empty(n + CANARY, dtype=dtype, device=DEV)
        self.bits = torch.int64 if dtype == torch.float64 else torch.int32
        self.whole.fill_(float('nan') if dtype == torch.float64 else fill)
        self.whole[n:].view(self.bits).fill_(0x5AFEC0DE5AFEC0DE if dtype == torch.float64 else 0x5AFEC0DE)
        self.t = self.whole[:n].view(*shape)
        self.expected = self.whole[n:].view(self.bits).clone()
        self.before = self.t.view(self.bits).clone()

    def intact(self):
        return torch.equal(self.whole[self.t.numel():].view(self.bits), self.expected)

    def untouched(self):
        return self.intact() and torch.equal(self.t.view(self.bits), self.before)

    def np(self):
        return self.t.cpu().numpy()


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _struct(p, x, n=None):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = p.n_s, p.n_u, x.size(0) if n is None else n
    _lib.fill(m.inv_ls2, 1.0 / p.ls ** 2)
    _lib.fill(m.outputscale, p.s)
    _lib.fill(m.noise, p.noise)
    m.x_train = x.data_ptr()
    return m


def run_select(probs, m, seeds=None, expect=_lib.SX_OK, n_train=None):
    """sx_gp_select of E problems into canaried buffers: dict(idx [E x m], sel_var [E x m], status [E], ws)"""
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    E = len(probs)
    xs = [_dev(p.X) for p in probs]
    n_train = n_train or [None] * E
    models = (_lib.SxGpModel * E)(*[_struct(p, x, n) for p, x, n in zip(probs, xs, n_train)])
    n_max = max(g.n_train for g in models)
    nbytes = int(lib.sx_gp_select_workspace_bytes(probs[0].n_s, E, min(n_max, 65536), min(m, n_max, 4096)))
    assert nbytes > 0
    b = dict(idx=Buf(E, m, dtype=torch.int32, fill=-7), sel_var=Buf(E, m), status=Buf(E, dtype=torch.int32),
             ws=Buf((nbytes + 7) // 8))
    seed_t, n_seed = None, 0
    if seeds is not None:
        seed_t = torch.tensor(np.asarray(seeds, dtype=np.int32).reshape(E, -1), device=DEV)
        n_seed = seed_t.size(1)
    code = lib.sx_gp_select(models, E, m, _lib.ptr(seed_t), n_seed, _lib.ptr(b['idx'].t), _lib.ptr(b['sel_var'].t),
                            _lib.ptr(b['status'].t), _lib.ptr(b['ws'].t), nbytes, stream)
    torch.cuda.synchronize()
    assert code == expect, f'sx_gp_select answered {code}, expected {expect}'
    return b


def _canaries(b, where):
    for key, buf in b.items():
        assert buf.intact(), f'{where}: the canary after `{key}` was overwritten'


def _against_oracle(where, p, m, seeds, idx, sel_var):
    """idx equals the oracle's; sel_var is within SEL_VAR_TOL x the prior of the float64 oracle's"""
    ref_idx, ref_sel, gap = S.oracle(p, m, seeds)
    prior = S.prior(p)
    err = float(np.abs(sel_var - ref_sel).max()) / prior
    first = int(np.argmax(idx != ref_idx)) if (idx != ref_idx).any() else -1
    print(f'SUBSET {where}: |sel_var - oracle| / prior {err:.3e} (allowed {S.SEL_VAR_TOL:.0e}), first differing step {first}')
    assert np.array_equal(idx, ref_idx), f'{where}: step {first} chose {idx[first]}, the oracle {ref_idx[first]}'
    assert err <= S.SEL_VAR_TOL, f'{where}: sel_var is {err:.3e} x the prior from the oracle'


# ---- the entry ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', S.CASES, ids=[str(c) for c in S.CASES])
def test_selection_matches_the_oracle(case):
    n_s, n_u, n, m, ratio = case
    p = R.problem(n_s, n_u, n, ratio)
    b = run_select([p], m)
    _canaries(b, str(case))
    assert int(b['status'].t[0]) == 0
    idx, sel_var = b['idx'].np()[0], b['sel_var'].np()[0]
    _against_oracle(str(case), p, m, (), idx, sel_var)
    if R.HAVE_LD and n <= 200 and m <= 64:
        _, ld_sel, _ = S.oracle(p, m, (), R.LD)
        _, ref_sel, _ = S.oracle(p, m, ())
        e_ref, e_kernel = R.rel_err(ref_sel, ld_sel), R.rel_err(sel_var, ld_sel)
        ratio_ = e_kernel / max(e_ref, FLOOR)
        print(f'SUBSET 32x sel_var | {case} | e_kernel {e_kernel:.3e} e_ref {e_ref:.3e} ratio {ratio_:.2f}')
        assert ratio_ <= FACTOR, f'{case}: e_kernel {e_kernel:.3e}, e_ref {e_ref:.3e}, ratio {ratio_:.1f} > {FACTOR}'
    elif n <= 200 and m <= 64:
        print(f'SUBSET 32x sel_var | {case} | long double is no wider than double here: rule not applied')


def test_ties_go_to_the_lowest_index():
    """Rows 20 and 150 are one far point: every point ties at step 0 (row 0 wins), the pair ties exactly at step 1 (20
    wins), and 150, then worth only its noise, is never chosen."""
    p = S.tie_problem()
    b = run_select([p], S.TIE_M)
    _canaries(b, 'tie')
    idx = b['idx'].np()[0]
    print(f'SUBSET tie: idx[:6] {idx[:6].tolist()}')
    assert idx[0] == 0 and idx[1] == S.TIE_ROWS[0] and S.TIE_ROWS[1] not in idx
    _against_oracle('tie', p, S.TIE_M, (), idx, b['sel_var'].np()[0])


def test_seeds_come_first():
    p = R.problem(2, 1, 193, 1e-2)
    b = run_select([p], S.SEEDS_M, seeds=[S.SEEDS])
    _canaries(b, 'seeds')
    idx = b['idx'].np()[0]
    print(f'SUBSET seeds: idx[:8] {idx[:8].tolist()}')
    assert int(b['status'].t[0]) == 0 and idx[:len(S.SEEDS)].tolist() == list(S.SEEDS)
    _against_oracle('seeds', p, S.SEEDS_M, S.SEEDS, idx, b['sel_var'].np()[0])


def _bit_equal(where, got, alone, e):
    for key in ('idx', 'sel_var'):
        a, c = got[key].t[e], alone[key].t[0]
        assert torch.equal(a.view(got[key].bits), c.view(alone[key].bits)), f'{where}: `{key}` differs from the call alone'


def test_batch_is_bit_equal_to_single_calls():
    probs = [R.problem(2, 1, n, 1e-2) for n in S.BATCH_N]
    b = run_select(probs, S.BATCH_M)
    _canaries(b, 'batch')
    assert b['status'].np().tolist() == [0, 0, 0]
    for e, p in enumerate(probs):
        alone = run_select([p], S.BATCH_M)
        _canaries(alone, f'batch, problem {e} alone')
        _bit_equal(f'batch, problem {e}', b, alone, e)
        _against_oracle(f'batch, problem {e}', p, S.BATCH_M, (), b['idx'].np()[e], b['sel_var'].np()[e])


def test_not_positive_definite():
    """40 copies of one point with noise = -0.01 s: step 0 succeeds, step 1 meets a negative variance"""
    bad = S.copies_problem(40)
    m = 30
    b = run_select([bad], m)
    _canaries(b, 'not PD')
    idx, sel = b['idx'].np()[0], b['sel_var'].np()[0]
    assert int(b['status'].t[0]) == NOT_PD
    assert idx[0] == 0 and abs(sel[0] - S.prior(bad)) <= 4 * R.EPS * S.prior(bad)
    assert (idx[1:] == -1).all() and np.isnan(sel[1:]).all()
    # between two healthy problems: they stay clean and give what they give alone
    probs = [R.problem(2, 1, 97, 1e-2), bad, R.problem(2, 1, 193, 1e-2)]
    b3 = run_select(probs, m)
    _canaries(b3, 'not PD in a batch')
    assert b3['status'].np().tolist() == [0, NOT_PD, 0]
    _bit_equal('not PD in a batch, the bad problem', b3, b, 1)
    for e in (0, 2):
        alone = run_select([probs[e]], m)
        _bit_equal(f'not PD in a batch, problem {e}', b3, alone, e)
        assert (b3['idx'].np()[e] >= 0).all() and np.isfinite(b3['sel_var'].np()[e]).all()


@pytest.mark.parametrize('seeds,bad_at', [((5, 193, 7), 1), ((5, -1, 7), 1), ((5, 7, 2 ** 30), 2), ((5, 7, 5), 2),
                                          ((9, 9), 1), ((193,), 0)],
                         ids=['past-the-end', 'negative', 'huge', 'repeated', 'repeated-at-once', 'first'])
def test_bad_seed_sets_the_flag(seeds, bad_at):
    p = R.problem(2, 1, 193, 1e-2)
    b = run_select([p], 12, seeds=[seeds])
    _canaries(b, f'seeds {seeds}')
    idx, sel = b['idx'].np()[0], b['sel_var'].np()[0]
    assert int(b['status'].t[0]) == NOT_PD
    assert idx[:bad_at].tolist() == list(seeds[:bad_at]) and np.isfinite(sel[:bad_at]).all()
    assert (idx[bad_at:] == -1).all() and np.isnan(sel[bad_at:]).all()


def test_limits_are_refused_before_any_write():
    p = R.problem(2, 1, 97, 1e-2)
    for m, n_train, code in ((98, None, _lib.SX_ERR_ARG), (10, [65537], _lib.SX_ERR_UNSUPPORTED)):
        b = run_select([p], m, expect=code, n_train=n_train)
        for key, buf in b.items():
            assert buf.untouched(), f'm = {m}, n_train = {n_train}: `{key}` was written'


# ---- Python ------------------------------------------------------------------------------------------------------------

def _conf(**kw):
    base = dict(device=DEV, exact_gp_kernel='rbf', exact_gp_training_iterations=0)
    base.update(kw)
    return type('Conf', (), base)()


def _ssm(p, **kw):
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    ssm = GpCemSSM(_conf(**kw), p.n_s, p.n_u)
    ssm.set_hyperparameters(p.ls, p.s, p.noise)
    return ssm


def _predictions(ssm, p, P=24):
    z = _dev(R.queries(p, P, far=False))
    out = ssm.predict_with_jacobians(z[:, :p.n_s], z[:, p.n_s:])
    torch.cuda.synchronize()
    return out


def _same_predictions(where, a, b):
    for name, x, y in zip(('mean', 'variance', 'jacobian'), a, b):
        assert torch.equal(x, y), f'{where}: the {name} differs'


def test_select_subset_method():
    p = R.problem(2, 1, 193, 1e-2)
    ssm = _ssm(p)
    idx, sel_var = ssm.select_subset(_dev(p.X), S.SEEDS_M, seed_idx=S.SEEDS)
    assert idx.dtype == torch.long and idx.is_cuda and sel_var.is_cuda and idx.shape == sel_var.shape == (S.SEEDS_M,)
    _against_oracle('select_subset', p, S.SEEDS_M, S.SEEDS, idx.cpu().numpy(), sel_var.cpu().numpy())
    with pytest.raises(RuntimeError, match='problem 0'):
        ssm.select_subset(_dev(p.X), 10, seed_idx=(3, 3))
    with pytest.raises(ValueError):
        ssm.select_subset(_dev(p.X), 194)


def test_model_fits_the_selected_subset():
    n_s, n_u, n, m, ratio = S.PYTHON_CASE
    p = R.problem(n_s, n_u, n, ratio)
    ref_idx, _, _ = S.oracle(p, m)
    ssm = _ssm(p, cem_gp_subset_size=m)
    ssm.update_model(_dev(p.X), _dev(p.Y), replace_old=True)
    assert ssm.device_model.n_train == m and ssm.x_train.size(0) == n and ssm.y_train.size(0) == n
    assert ssm._subset_idx.cpu().numpy().tolist() == ref_idx.tolist()
    plain = _ssm(p)
    plain.update_model(_dev(p.X[ref_idx]), _dev(p.Y[ref_idx]), replace_old=True)
    _same_predictions('subset model', _predictions(ssm, p), _predictions(plain, p))
    assert np.array_equal(ssm.information_gain(), plain.information_gain())
    # appending keeps the pool and selects from scratch
    extra = R.problem(n_s, n_u, 50, ratio)
    ssm.update_model(_dev(extra.X), _dev(extra.Y))
    assert ssm.x_train.size(0) == n + 50 and ssm.device_model.n_train == m


def test_small_pool_is_fitted_whole():
    p = R.problem(2, 1, 50, 1e-2)
    ssm, plain = _ssm(p, cem_gp_subset_size=64), _ssm(p)
    for s in (ssm, plain):
        s.update_model(_dev(p.X), _dev(p.Y), replace_old=True)
    assert ssm.device_model.n_train == 50 and ssm._subset_idx is None
    _same_predictions('n <= m', _predictions(ssm, p), _predictions(plain, p))


def test_pool_beyond_the_fit_limit_is_accepted():
    p = R.problem(2, 1, 4100, 1e-2)
    with pytest.raises(ValueError, match='4096'):
        _ssm(p).update_model(_dev(p.X), _dev(p.Y), replace_old=True)
    ssm = _ssm(p, cem_gp_subset_size=12)
    ssm.update_model(_dev(p.X), _dev(p.Y), replace_old=True)
    assert ssm.x_train.size(0) == 4100 and ssm.device_model.n_train == 12
    assert ssm._subset_idx.cpu().numpy().tolist() == S.oracle(p, 12)[0].tolist()


@pytest.mark.parametrize('opt_hyp', [False, True], ids=['fixed', 'opt_hyp'])
def test_update_models_multi_equals_single_updates(opt_hyp):
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import update_models_multi
    probs = [R.problem(2, 1, n, 1e-2) for n in S.BATCH_N]
    kw = dict(cem_gp_subset_size=S.BATCH_M, exact_gp_training_iterations=2)
    together, alone = [_ssm(p, **kw) for p in probs], [_ssm(p, **kw) for p in probs]
    update_models_multi(together, [_dev(p.X) for p in probs], [_dev(p.Y) for p in probs], opt_hyp=opt_hyp, replace_old=True)
    for e, (p, a, t) in enumerate(zip(probs, alone, together)):
        a.update_model(_dev(p.X), _dev(p.Y), opt_hyp=opt_hyp, replace_old=True)
        assert t.device_model.n_train == S.BATCH_M and t.x_train.size(0) == p.X.shape[0]
        assert torch.equal(t._subset_idx, a._subset_idx), f'problem {e}: another subset'
        for name in ('_raw_lengthscale', '_raw_outputscale', '_raw_noise'):
            assert torch.equal(getattr(t, name), getattr(a, name)), f'problem {e}: {name}'
        _same_predictions(f'update_models_multi, problem {e}', _predictions(t, p), _predictions(a, p))
        if not opt_hyp:
            assert t._subset_idx.cpu().numpy().tolist() == S.oracle(p, S.BATCH_M)[0].tolist()


def test_safempc_acts_on_the_subset():
    """One CemSafeMPC.get_action over a model bounded to 64 of 300 points is the action of a solver built on the
    oracle's 64 points."""
    from safe_exploration_amd import problems
    from safe_exploration_amd.safempc_cem import MpcResult
    spec, p = S.solver_problem()
    ref_idx, _, _ = S.oracle(p, S.SOLVER_M)
    P, H, iters = 128, 5, 3
    conf = dict(mpc_time_horizon=H, cem_num_rollouts=P, cem_num_elites=12, cem_num_iterations=iters, cem_init_std=0.5,
                plot_cem_optimisation=False, plot_cem_terminal_states=False, use_state_constraint=True,
                use_prior_model=True)
    noise = torch.tensor(np.random.default_rng(5).normal(size=(iters, 1, P, H, spec.n_u)), device=DEV)
    x0 = np.array([0.02, -0.03])
    actions = []
    for sp, kw in ((spec, dict(cem_gp_subset_size=S.SOLVER_M)),
                   (dataclasses.replace(spec, X=spec.X[ref_idx], Y=spec.Y[ref_idx]), {})):
        solver, _ = problems.make_solver(sp, _conf(**conf, **kw), problems.StubEnv(sp, np.zeros(2)), device=DEV)
        solver.init_solver(lambda *a: 0.0)
        mpc = solver._solver()
        mpc._next_noise = lambda episodes: noise
        action, result = solver.get_action(x0)
        assert result == MpcResult.FOUND_SOLUTION
        assert solver._ssm.device_model.n_train == S.SOLVER_M
        actions.append(np.asarray(action).reshape(-1))
    assert solver._ssm.x_train.size(0) == S.SOLVER_M and len(spec.X) == S.SOLVER_N
    print(f'SUBSET solver: action {actions[0]}, on the oracle\'s subset {actions[1]}')
    assert np.array_equal(actions[0], actions[1])
