"""GPU: sx_gp_drop -- the k <= 64 oldest rows removed from a fitted exact GP -- through the C ABI and through GpCemSSM with
conf.cem_gp_window.

The problems are those of tests/warm_path_reference.py, fitted at N by sx_gp_fit and cut down to their last N - k rows, and the
truth is the long-double factorisation of those rows.  The unit and the allowance are tests/test_gpu_warm_path.py's own
(imported, not restated): a quantity's error against the long-double truth in units of max(LAPACK's float64 error, 8 eps) stays
within FACTOR = 32, and so do the two residuals against LAPACK's.  The (N, k) pairs: one kept row, the 64-row tile edge on both
sides (65 - 1, 66 - 1, 66 - 2, 161 - 64, 193 - 2), the fit's one-workgroup / blocked switch (96 / 97), full and partly filled
stage sets (64, 37, 33, 2, 1), and N = 410, the long-double reference's limit.  Every output buffer and the workspace end in a
canary.  Each check prints its figures before it asserts (`pytest -s`): DESIGN.md section 3.5 records the worst of them."""
import ctypes

import numpy as np
import pytest
import torch

import drop_reference as D
import test_gpu_warm_path as WP
import warm_path_reference as R
from test_gpu_gp_append import PARITY, QUANTITIES, _Spy, _old, fit_head, run_append
from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem import gp_ssm_cem

pytestmark = pytest.mark.gpu
DEV = WP.DEV
PAIRS = ((2, 1), (6, 1), (65, 1), (66, 1), (66, 2), (97, 1), (97, 33), (161, 64), (130, 37), (193, 2), (410, 64))
SHAPES = ((1, 1), (2, 1), (4, 2))
WIDE_CASES = (((1, 5), (66, 1)), ((1, 5), (130, 37)))
RATIOS = (1e-2, 1e-6)
CASES = [(sh, pair) for pair in PAIRS for sh in SHAPES] + list(WIDE_CASES)


def run_drop(n_s, linv_old, y_kept, k, status=None):
    """sx_gp_drop of the first k rows of `linv_old` (device [n_s x N x N]) into canaried buffers; y_kept: device [m x n_s]"""
    lib = _lib.lib()
    n = linv_old.size(1)
    m = n - k
    nbytes = int(lib.sx_gp_drop_workspace_bytes(n_s, n, k))
    assert nbytes > 0 and nbytes % 8 == 0
    b = dict(linv=WP.Buf(n_s, m, m), alpha=WP.Buf(n_s, m), logdet=WP.Buf(n_s), ws=WP.Buf(nbytes // 8),
             status=status if status is not None else WP.Buf(1, dtype=torch.int32))
    _lib.check(lib.sx_gp_drop(n_s, n, k, _lib.ptr(y_kept), _lib.ptr(linv_old), _lib.ptr(b['linv'].t), _lib.ptr(b['alpha'].t),
                              _lib.ptr(b['logdet'].t), _lib.ptr(b['status'].t), _lib.ptr(b['ws'].t), nbytes,
                              _lib.stream_ptr(torch.device(DEV))), 'sx_gp_drop')
    torch.cuda.synchronize()
    return b


def _healthy(b, where):
    for key, buf in b.items():
        assert buf.intact(), f'{where}: the canary after `{key}` was overwritten'
    for key in QUANTITIES:
        assert bool(torch.isfinite(b[key].t).all()), f'{where}: `{key}` has a non-finite element'
    assert int(torch.count_nonzero(torch.triu(b['linv'].t, 1))) == 0, f'{where}: linv is not lower triangular'


def _case(p, k):
    return '({},{}) N={}-{} ratio={:g}'.format(p.n_s, p.n_u, p.X.shape[0], k, p.key[3])


def _ratios(got, kept):
    """error / max(LAPACK's error, 8 eps) of every quantity against the long-double truth of the problem `kept`"""
    f64, ld = R.reference(kept), R.reference(kept, True)
    return {q: R.rel_err(got[q], getattr(ld, q)) / max(R.rel_err(getattr(f64, q), getattr(ld, q)), WP.FLOOR)
            for q in QUANTITIES}


# ---- a. drops from a fit, over the covering set ------------------------------------------------------------------------------

@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('shape,pair', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_drop_products(shape, pair, ratio):
    n, k = pair
    p = R.problem(*shape, n, ratio)
    kept = D.tail(p, k)
    old = fit_head(p, n)
    before = {q: old[q].t.clone() for q in QUANTITIES}
    y = WP._dev(kept.Y)
    b = run_drop(p.n_s, old['linv'].t, y, k)
    case = _case(p, k)
    assert int(b['status'].t.item()) == 0
    _healthy(b, case)
    got = {q: b[q].np() for q in QUANTITIES}
    WP.forward('sx_gp_drop', case, kept, QUANTITIES, got)
    WP.residual_rule('sx_gp_drop', case, kept, R.reference(kept), got['linv'], got['alpha'])
    # the same inputs give the same bits, and the inputs are untouched
    again = run_drop(p.n_s, old['linv'].t, y, k)
    for q in QUANTITIES:
        assert torch.equal(again[q].t, b[q].t), (case, q)
        assert torch.equal(old[q].t, before[q]) and old[q].intact(), (case, q)
    assert torch.equal(y, WP._dev(kept.Y))


# ---- b. drops compose with appends and with each other -----------------------------------------------------------------------

def test_one_slide_from_a_fresh_fit():
    """(2,1), 130 fitted rows, 37 dropped and 5 appended across a tile edge: sx_gp_append takes sx_gp_drop's outputs"""
    p = R.problem(2, 1, 135, 1e-4)
    n, r = 130, 37
    old = fit_head(p, n)
    dropped = run_drop(2, old['linv'].t, WP._dev(p.Y[r:n]), r)
    win = D.window(p, r, 135)
    b = run_append(win, n - r, _old(dropped), status=dropped['status'])
    assert int(b['status'].t.item()) == 0
    got = {q: b[q].np() for q in QUANTITIES}
    WP.forward('sx_gp_drop + sx_gp_append', _case(p, r), win, QUANTITIES, got)
    WP.residual_rule('sx_gp_drop + sx_gp_append', _case(p, r), win, R.reference(win), got['linv'], got['alpha'])


def test_drop_takes_its_own_output():
    """(2,1) N = 140 - 40 - 3: the second call drops from the first one's buffers, across the fit's kernel switch"""
    p = R.problem(2, 1, 140)
    first = run_drop(2, fit_head(p, 140)['linv'].t, WP._dev(p.Y[40:]), 40)
    b = run_drop(2, first['linv'].t, WP._dev(p.Y[43:]), 3)
    assert int(first['status'].t.item()) == 0 and int(b['status'].t.item()) == 0
    _healthy(b, 'two drops')
    kept = D.tail(p, 43)
    got = {q: b[q].np() for q in QUANTITIES}
    WP.forward('sx_gp_drop twice', _case(p, 43), kept, QUANTITIES, got)
    WP.residual_rule('sx_gp_drop twice', _case(p, 43), kept, R.reference(kept), got['linv'], got['alpha'])


# ---- c. chains of slides -------------------------------------------------------------------------------------------------------

CHAIN_RUNS = (('65 by 1', 65, 1, 1e-4, (16, 64, 128)), ('65 by 1', 65, 1, 1e-6, (16, 64, 128)), ('130 by 8', 130, 8, 1e-4, (64,)))
CHAIN_RTOL = 1e-9        # PARITY's rtol: what information_gain() is compared at


def _slide_chain(p, m, step, rows):
    """window m of (2,1) problem p slid `step` rows at a time over `rows` rows; yields (rows slid, buffers) at every step"""
    cur = _old(fit_head(p, m))
    for lo in range(step, rows + 1, step):
        dropped = run_drop(2, cur['linv'], WP._dev(p.Y[lo:lo - step + m]), step)
        b = run_append(D.window(p, lo, lo + m), m - step, _old(dropped), status=dropped['status'])
        assert int(b['status'].t.item()) == 0, lo
        cur = _old(b)
        yield lo, b


@pytest.mark.parametrize('name,m,step,ratio,lengths', CHAIN_RUNS, ids=lambda v: str(v).replace(' ', ''))
def test_chains_of_slides(name, m, step, ratio, lengths):
    """A window slid for 16, 64 and 128 single rows (m = 65) and for 8 x 8 rows (m = 130), against the long-double reference
    of the final window in the unit of (a), beside sx_gp_fit's own ratio on the same window.  Measured on an MI355X
    (ratio = error / max(LAPACK's error, 8 eps); linv, alpha, logdet; sx_gp_fit's own in brackets):
        65 by 1, 1e-4:    16 rows  2.20 1.59 4.14 (0.64 0.55 0.98)    64 rows  4.68 1.18 2.05 (0.64 0.56 0.26)
                         128 rows  14.19 14.77 9.07 (1.38 1.44 1.84)
        65 by 1, 1e-6:    16 rows  0.66 0.57 0.87 (0.45 0.08 1.11)    64 rows  6.05 9.26 12.26 (1.48 1.39 1.64)
                         128 rows  2.32 3.54 1.38 (0.24 0.65 0.28)
        130 by 8, 1e-4:   64 rows  7.83 3.00 24.28 (3.60 2.06 5.20)
    and the log-determinant's relative error stayed below 4e-13.  Every run is within FACTOR at every length, so
    conf.cem_gp_window_max_chain defaults to 128, the longest length measured, and the test asserts the bound at every
    measured length up to the default; the chain's log-determinant meets the parity rtol of 1e-9 at every length."""
    p = R.problem(2, 1, m + max(lengths), ratio)
    for lo, b in _slide_chain(p, m, step, max(lengths)):
        if lo not in lengths:
            continue
        win = D.window(p, lo, lo + m)
        _healthy(b, f'chain {name} at {lo}')
        chain = _ratios({q: b[q].np() for q in QUANTITIES}, win)
        fit = _ratios({q: v.np() for q, v in WP.run_single(win).items() if q in QUANTITIES}, win)
        ld = R.reference(win, True)
        logdet_err = float(np.abs((b['logdet'].np() - ld.logdet.astype(np.float64)) / ld.logdet.astype(np.float64)).max())
        print(f'DROP chain {name} ratio={ratio:g} | {lo} rows | chain ' + ' '.join(f'{q} {chain[q]:.2f}' for q in QUANTITIES)
              + ' | fit ' + ' '.join(f'{q} {fit[q]:.2f}' for q in QUANTITIES) + f' | logdet rel {logdet_err:.2e}')
        assert logdet_err <= CHAIN_RTOL, (lo, logdet_err)
        if lo <= gp_ssm_cem.WINDOW_MAX_CHAIN:
            for q in ('linv', 'alpha'):
                assert chain[q] <= WP.FACTOR, (lo, q, chain[q])


def test_default_chain_bound_is_a_measured_length():
    assert gp_ssm_cem.WINDOW_MAX_CHAIN in (1, 16, 64, 128)

    class Conf:
        device, exact_gp_kernel, exact_gp_training_iterations, cem_gp_incremental, cem_gp_window = DEV, 'rbf', 0, True, 65
    assert gp_ssm_cem.GpCemSSM(Conf(), 2, 1)._window_max_chain == gp_ssm_cem.WINDOW_MAX_CHAIN


# ---- d. through the model ------------------------------------------------------------------------------------------------------

class _Conf:
    device, exact_gp_kernel, exact_gp_training_iterations = DEV, 'rbf', 0

    def __init__(self, incremental, window=None):
        self.cem_gp_incremental = incremental
        if window is not None:
            self.cem_gp_window = window


def _gp(p, incremental, window=None):
    ssm = gp_ssm_cem.GpCemSSM(_Conf(incremental, window), p.n_s, p.n_u)
    ssm.set_hyperparameters(p.ls, p.s, p.noise)
    return ssm


def _counts(spy):
    got = tuple(spy.calls[name] for name in ('sx_gp_fit', 'sx_gp_drop', 'sx_gp_append', 'sx_gp_pack'))
    spy.calls.clear()
    return got


def _same_predictions(ssm, fresh, z, equal=False):
    for got, want in zip(ssm.predict_with_jacobians(z[:, :2], z[:, 2:]), fresh.predict_with_jacobians(z[:, :2], z[:, 2:])):
        if equal:
            assert torch.equal(got, want)
        else:
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), **PARITY)
    if equal:
        assert np.array_equal(ssm.information_gain(), fresh.information_gain())
    else:
        np.testing.assert_allclose(ssm.information_gain(), fresh.information_gain(), **PARITY)


def test_model_slides_row_by_row_and_matches_the_model_fitted_on_the_window(monkeypatch):
    """(2,1), window 70 across the tile edge, filled by a first update of 68 rows and one append, then slid by 1, 1 and 3 rows"""
    p = R.problem(2, 1, 75)
    X, Y = WP._dev(p.X), WP._dev(p.Y)
    z = WP._dev(R.queries(p, 7, far=False))
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', spy)
    ssm = _gp(p, True, window=70)
    ssm.update_model(X[:68], Y[:68])
    spy.calls.clear()
    ssm.update_model(X[68:70], Y[68:70])
    assert _counts(spy) == (0, 0, 1, 1)
    for lo, hi in ((70, 71), (71, 72), (72, 75)):
        ssm.update_model(X[lo:hi], Y[lo:hi])
        assert _counts(spy) == (0, 1, 1, 1), hi
        assert torch.equal(ssm.x_train, X[hi - 70:hi]) and torch.equal(ssm.y_train, Y[hi - 70:hi])
        assert ssm._linv_current and ssm._fit_ws[1].shape == (2, 70, 70) and ssm._appended == hi - 68
        fresh = _gp(p, False)
        fresh.update_model(X[hi - 70:hi], Y[hi - 70:hi])
        spy.calls.clear()
        _same_predictions(ssm, fresh, z)


def test_setting_off_is_the_parent_path(monkeypatch):
    p = R.problem(2, 1, 43)
    X, Y = WP._dev(p.X), WP._dev(p.Y)
    z = WP._dev(R.queries(p, 7, far=False))
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', spy)
    whole = _gp(p, False)
    whole.update_model(X, Y)
    for incremental in (False, True):
        ssm = _gp(p, incremental)
        ssm.update_model(X[:40], Y[:40])
        ssm.update_model(X[40:], Y[40:])
        assert spy.calls['sx_gp_drop'] == 0 and spy.calls['sx_gp_drop_workspace_bytes'] == 0
        assert ssm.x_train.size(0) == 43
        if not incremental:
            _same_predictions(ssm, whole, z, equal=True)
    # a window the data never fill changes nothing either: the appended model's bits
    windowed = _gp(p, True, window=43)
    windowed.update_model(X[:40], Y[:40])
    windowed.update_model(X[40:], Y[40:])
    assert spy.calls['sx_gp_drop'] == 0
    _same_predictions(windowed, ssm, z, equal=True)


def test_safempc_action_after_a_slid_update():
    from safe_exploration_amd import problems
    from safe_exploration_amd.safempc_cem import MpcResult

    class Conf:
        mpc_time_horizon, cem_num_rollouts, cem_num_elites, cem_num_iterations, cem_init_std = 5, 128, 12, 3, 0.2
        device, use_state_constraint, use_prior_model = DEV, True, True
        exact_gp_training_iterations, exact_gp_kernel = 0, 'rbf'
        plot_cem_optimisation = plot_cem_terminal_states = False

    class Windowed(Conf):
        cem_gp_incremental, cem_gp_window = True, 64

    spec = problems.pendulum(n_train=64, seed=0)
    slid, fresh = problems.make_solver(spec, Windowed())[0], problems.make_solver(spec, Conf())[0]
    rng = np.random.default_rng(5)
    x_new, y_new = rng.uniform(-0.3, 0.3, size=(2, 3)), rng.uniform(-0.05, 0.05, size=(2, 2))
    slid.update_model(x_new, y_new, replace_old=False)
    assert slid._ssm._appended == 2 and slid._ssm.x_train.size(0) == 64
    # (the model's own rows, which already are errors to the prior: straight into the fresh solver's model)
    fresh._ssm.update_model(slid._ssm.x_train, slid._ssm.y_train, replace_old=True)
    assert fresh._ssm._appended == 0 and torch.equal(fresh._ssm.x_train, slid._ssm.x_train)
    noise = rng.normal(size=(Conf.cem_num_iterations, Conf.cem_num_rollouts, Conf.mpc_time_horizon, 1))
    x0 = np.array([0.02, -0.03])
    actions = []
    for solver in (slid, fresh):
        it = iter(noise)
        solver._solver().sample_noise = lambda episodes=1, it=it: WP._dev(next(it)[None])
        action, result = solver.get_action(x0)
        assert result == MpcResult.FOUND_SOLUTION
        actions.append(action)
    np.testing.assert_allclose(actions[0], actions[1], rtol=0, atol=1e-9)


# ---- e. a W11 that is no factor: a status, the next call is unaffected, the model fits in full ----------------------------

@pytest.mark.parametrize('value', [float('nan'), float('inf'), -1.0])
def test_bad_w11_is_flagged(value):
    p = R.problem(2, 1, 70)
    old = fit_head(p, 70)
    y = WP._dev(p.Y[5:])
    spoiled = old['linv'].t.clone()
    spoiled[1, 3, 3 if value < 0 else 1] = value
    bad = run_drop(2, spoiled, y, 5)
    for key, buf in bad.items():
        assert buf.intact(), f'bad W11: the canary after `{key}` was overwritten'
    assert int(bad['status'].t.item()) == _lib.SX_STATUS_NOT_PD
    good = run_drop(2, old['linv'].t, y, 5)
    assert int(good['status'].t.item()) == 0
    _healthy(good, 'after a flagged call')
    WP.forward('sx_gp_drop', _case(p, 5), D.tail(p, 5), QUANTITIES, {q: good[q].np() for q in QUANTITIES})
    # the word is or-ed into: a set bit stays
    kept = run_drop(2, old['linv'].t, y, 5, status=bad['status'])
    assert int(kept['status'].t.item()) == _lib.SX_STATUS_NOT_PD and torch.equal(kept['linv'].t, good['linv'].t)


def test_model_falls_back_to_the_full_fit_where_the_drop_is_flagged(monkeypatch):
    p = R.problem(2, 1, 43)
    X, Y = WP._dev(p.X), WP._dev(p.Y)
    z = WP._dev(R.queries(p, 7, far=False))
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', spy)
    ssm = _gp(p, True, window=40)
    ssm.update_model(X[:40], Y[:40])
    ssm._fit_ws[1][0, 0, 0] = float('nan')
    spy.calls.clear()
    ssm.update_model(X[40:], Y[40:])
    assert _counts(spy) == (1, 1, 1, 1) and ssm._appended == 0
    fresh = _gp(p, False)
    fresh.update_model(X[3:], Y[3:])
    _same_predictions(ssm, fresh, z, equal=True)
