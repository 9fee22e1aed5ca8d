"""GPU: sx_gp_append -- k <= 64 rows appended to a fitted exact GP -- through the C ABI and through GpCemSSM with
conf.cem_gp_incremental.

The problems are those of tests/warm_path_reference.py, fitted at N by sx_gp_fit and appended to N + k, and the truth is the
long-double factorisation of the full set.  The unit and the allowance are tests/test_gpu_warm_path.py's own (imported, not
restated): a quantity's error against the long-double truth in units of max(LAPACK's float64 error, 8 eps) stays within
FACTOR = 32, and so do the two residuals against LAPACK's.  The (N, k) pairs are the smallest that reach every branch:
one row and a few, the 64-row tile edge (63, 64, 65), the fit's one-workgroup / blocked switch between the old and the new N
(95, 96), full and partly filled tiles of new rows (64, 37, 2) over two to six row blocks, and N + k = 410, the long-double
reference's limit.  Every output buffer and the workspace end in a canary.  Each check prints its figures before it asserts
(`pytest -s`): DESIGN.md section 3.5 records the worst of them."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import append_reference as A
import test_gpu_warm_path as WP
import warm_path_reference as R
from oracle.gp import ExactGP
from safe_exploration_amd import _lib

pytestmark = pytest.mark.gpu
DEV = WP.DEV
PAIRS = ((1, 1), (5, 1), (63, 1), (64, 1), (65, 1), (95, 1), (96, 1), (97, 64), (130, 37), (193, 2), (346, 64))
SHAPES = ((1, 1), (2, 1), (4, 2))
WIDE_CASES = (((1, 5), (64, 1)), ((1, 5), (130, 37)))
RATIOS = (1e-2, 1e-6)
CASES = [(sh, pair) for pair in PAIRS for sh in SHAPES] + list(WIDE_CASES)
PARITY = dict(rtol=1e-9, atol=1e-11)          # tests/test_gpu_parity.py: GP mean / variance / Jacobian against the oracle
QUANTITIES = ('linv', 'alpha', 'logdet')


def fit_head(p, n):
    """sx_gp_fit of the first n rows of p (canaried buffers, tests/test_gpu_warm_path.py)"""
    b = WP.run_single(A.head(p, n))
    assert int(b['status'].t.item()) == 0
    return b


def run_append(p, n, old, status=None):
    """sx_gp_append of the rows of p beyond the first n to `old` = {linv, alpha, logdet} (device tensors) into canaried
    buffers"""
    lib = _lib.lib()
    n2, k = p.X.shape[0], p.X.shape[0] - n
    x, y = WP._dev(p.X), WP._dev(p.Y)
    m = WP._struct(p, x)
    nbytes = int(lib.sx_gp_append_workspace_bytes(p.n_s, n2, k))
    assert nbytes > 0 and nbytes % 8 == 0
    b = dict(linv=WP.Buf(p.n_s, n2, n2), alpha=WP.Buf(p.n_s, n2), logdet=WP.Buf(p.n_s), ws=WP.Buf(nbytes // 8),
             status=status if status is not None else WP.Buf(1, dtype=torch.int32))
    _lib.check(lib.sx_gp_append(ctypes.byref(m), n, _lib.ptr(y), _lib.ptr(old['linv']), _lib.ptr(old['alpha']),
                                _lib.ptr(old['logdet']), _lib.ptr(b['linv'].t), _lib.ptr(b['alpha'].t), _lib.ptr(b['logdet'].t),
                                _lib.ptr(b['status'].t), _lib.ptr(b['ws'].t), nbytes, _lib.stream_ptr(torch.device(DEV))),
               'sx_gp_append')
    torch.cuda.synchronize()
    return b


def _old(b):
    return {k: b[k].t for k in QUANTITIES}


def _healthy(b, where):
    for key, buf in b.items():
        assert buf.intact(), f'{where}: the canary after `{key}` was overwritten'
    for key in QUANTITIES:
        assert bool(torch.isfinite(b[key].t).all()), f'{where}: `{key}` has a non-finite element'
    assert int(torch.count_nonzero(torch.triu(b['linv'].t, 1))) == 0, f'{where}: linv is not lower triangular'


def _case(p, n):
    return '({},{}) N={}+{} ratio={:g}'.format(p.n_s, p.n_u, n, p.X.shape[0] - n, p.key[3])


# ---- a. through the C ABI, over the covering set ---------------------------------------------------------------------------

@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('shape,pair', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_append_products(shape, pair, ratio):
    n, k = pair
    p = R.problem(*shape, n + k, ratio)
    old = fit_head(p, n)
    b = run_append(p, n, _old(old))
    case = _case(p, n)
    assert int(b['status'].t.item()) == 0
    _healthy(b, case)
    # the old rows are the fit's, bit for bit, in the new stride
    assert torch.equal(b['linv'].t[:, :n, :n], old['linv'].t), case
    got = {q: b[q].np() for q in QUANTITIES}
    WP.forward('sx_gp_append', case, p, QUANTITIES, got)
    WP.residual_rule('sx_gp_append', case, p, R.reference(p), got['linv'], got['alpha'])
    # the same inputs give the same bits
    again = run_append(p, n, _old(old))
    for q in QUANTITIES:
        assert torch.equal(again[q].t, b[q].t), (case, q)
    assert all(old[q].intact() for q in QUANTITIES)


def test_append_takes_its_own_output():
    """(2,1) N = 60 + 37 + 2: the second call appends to the first one's buffers, across the fit's kernel switch"""
    p = R.problem(2, 1, 99)
    first = run_append(A.head(p, 97), 60, _old(fit_head(p, 60)))
    b = run_append(p, 97, _old(first))
    assert int(first['status'].t.item()) == 0 and int(b['status'].t.item()) == 0
    _healthy(b, 'two appends')
    got = {q: b[q].np() for q in QUANTITIES}
    WP.forward('sx_gp_append twice', _case(p, 97), p, QUANTITIES, got)
    WP.residual_rule('sx_gp_append twice', _case(p, 97), p, R.reference(p), got['linv'], got['alpha'])


# ---- b. a chain of single-row appends ---------------------------------------------------------------------------------------

CHAIN = (2, 1, 65, 129, 1e-4)       # shape, N, final N, noise / outputscale


def test_chain_of_64_single_row_appends():
    """N = 65 -> 129 one row at a time, against the long-double reference of the final set in the unit of (a), beside
    sx_gp_fit's own ratio on the same set.  Measured on an MI355X (ratio = error / max(LAPACK's error, 8 eps)):
        linv    chain 1.30    fit 1.08
        alpha   chain 1.00   fit 1.19
        logdet  chain 1.87  fit 1.27
    The chain stays within FACTOR, so conf.cem_gp_incremental_max_chain defaults to None and the test asserts at the full
    length."""
    n_s, n_u, n0, n1, ratio = CHAIN
    p = R.problem(n_s, n_u, n1, ratio)
    cur = _old(fit_head(p, n0))
    last = None
    for m in range(n0 + 1, n1 + 1):
        last = run_append(A.head(p, m), m - 1, cur)
        assert int(last['status'].t.item()) == 0, m
        cur = _old(last)
    _healthy(last, 'chain')
    fit = WP.run_single(p)
    f64, ld = R.reference(p), R.reference(p, True)
    ratios = {}
    for q in QUANTITIES:
        e_ref = R.rel_err(getattr(f64, q), getattr(ld, q))
        for who, b in (('chain', last), ('fit', fit)):
            ratios[who, q] = R.rel_err(b[q].np(), getattr(ld, q)) / max(e_ref, WP.FLOOR)
        print(f'APPEND chain 65->129 | {q} | e_ref {e_ref:.3e} chain ratio {ratios["chain", q]:.2f} '
              f'fit ratio {ratios["fit", q]:.2f}')
    for q in QUANTITIES:
        assert ratios['chain', q] <= WP.FACTOR, (q, ratios['chain', q])
    WP.residual_rule('sx_gp_append chain', _case(p, n1 - 1), p, f64, last['linv'].np(), last['alpha'].np())
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM

    class Conf:
        device, exact_gp_kernel, exact_gp_training_iterations, cem_gp_incremental = DEV, 'rbf', 0, True
    assert GpCemSSM(Conf(), 2, 1)._max_chain is None


# ---- c. not positive definite: a status, and the next call is unaffected -----------------------------------------------------

@pytest.mark.parametrize('n_all,a,b', [(70, 5, 65), (66, 5, 65), (130, 3, 100)])
def test_not_positive_definite_schur_complement_is_flagged(n_all, a, b):
    """Row b repeats row a < b on a grid where K = s I and noise = -0.01 s: the first b rows factorise, and an appended row b
    makes the first pivot of S  0.99 s - s / 0.99 < 0."""
    p = R.not_pd_problem(n_all, a, b)
    with pytest.raises(np.linalg.LinAlgError):
        A.append(p, b)
    old = fit_head(p, b)
    bad = run_append(p, b, _old(old))
    for key, buf in bad.items():
        assert buf.intact(), f'not PD: the canary after `{key}` was overwritten'
    assert int(bad['status'].t.item()) == _lib.SX_STATUS_NOT_PD
    # a healthy problem in the next call
    q = R.problem(2, 1, 66)
    good = run_append(q, 65, _old(fit_head(q, 65)))
    assert int(good['status'].t.item()) == 0
    _healthy(good, 'after a not-PD call')
    WP.forward('sx_gp_append', _case(q, 65), q, QUANTITIES, {k: good[k].np() for k in QUANTITIES})
    # the word is or-ed into: a set bit stays
    kept = run_append(q, 65, _old(fit_head(q, 65)), status=bad['status'])
    assert int(kept['status'].t.item()) == _lib.SX_STATUS_NOT_PD and torch.equal(kept['linv'].t, good['linv'].t)


# ---- d. downstream: sx_gp_pack and sx_gp_predict take the appended factor ----------------------------------------------------

def test_pack_and_predict_from_the_appended_factor():
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    p = R.problem(2, 1, 167)
    b = run_append(p, 130, _old(fit_head(p, 130)))
    assert int(b['status'].t.item()) == 0
    x = WP._dev(p.X)
    m = WP._struct(p, x)
    a_n, t_n = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.sx_gp_pack_sizes(m.n_s, m.n_u, m.n_train, ctypes.byref(a_n), ctypes.byref(t_n)), 'sx_gp_pack_sizes')
    a_pack = torch.empty(a_n.value, dtype=torch.float64, device=DEV)
    stage_tab = torch.empty(t_n.value, dtype=torch.int32, device=DEV)
    m.a_pack, m.stage_tab = a_pack.data_ptr(), stage_tab.data_ptr()
    _lib.check(lib.sx_gp_pack(ctypes.byref(m), _lib.ptr(b['linv'].t), _lib.ptr(b['alpha'].t), stream), 'sx_gp_pack')
    P = 7
    z = R.queries(p, P, far=False)
    zt = WP._dev(z)
    mean, var, jac = WP.Buf(P, 2), WP.Buf(P, 2), WP.Buf(P, 2, 3)
    ws_bytes = int(lib.sx_gp_predict_workspace_bytes(ctypes.byref(m), P))
    assert ws_bytes == 0
    _lib.check(lib.sx_gp_predict(ctypes.byref(m), _lib.ptr(zt), P, _lib.ptr(mean.t), _lib.ptr(var.t), _lib.ptr(jac.t), None, 0,
                                 stream), 'sx_gp_predict')
    torch.cuda.synchronize()
    assert mean.intact() and var.intact() and jac.intact()
    mo, vo, jo = ExactGP(p.X, p.Y, p.ls, p.s, p.noise).predict(z)
    np.testing.assert_allclose(mean.np(), mo, **PARITY)
    np.testing.assert_allclose(var.np(), vo, **PARITY)
    np.testing.assert_allclose(jac.np(), jo, **PARITY)


# ---- e. through Python ------------------------------------------------------------------------------------------------------

class _Spy:
    def __init__(self, real):
        self.real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


class _Conf:
    device, exact_gp_kernel, exact_gp_training_iterations = DEV, 'rbf', 0

    def __init__(self, incremental):
        self.cem_gp_incremental = incremental


def _gp(p, incremental):
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    ssm = GpCemSSM(_Conf(incremental), p.n_s, p.n_u)
    ssm.set_hyperparameters(p.ls, p.s, p.noise)
    return ssm


def test_model_appends_row_by_row_and_matches_the_model_fitted_whole(monkeypatch):
    """(2,1), N = 40 and three single-row updates.  The appended model and the model given the same rows in one update_model
    are not bit-equal: the appended W' comes from another sequence of roundings (S = K_cc - B^T B on the old inverse factor
    instead of the Cholesky factorisation's own updates), so they agree to the parity tolerance of the GP outputs."""
    p = R.problem(2, 1, 43)
    X, Y = WP._dev(p.X), WP._dev(p.Y)
    z = WP._dev(R.queries(p, 7, far=False))
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', spy)
    ssm = _gp(p, True)
    ssm.update_model(X[:40], Y[:40])
    assert (spy.calls['sx_gp_fit'], spy.calls['sx_gp_append']) == (1, 0)
    for n in (41, 42, 43):
        spy.calls.clear()
        ssm.update_model(X[n - 1:n], Y[n - 1:n])
        assert (spy.calls['sx_gp_fit'], spy.calls['sx_gp_append'], spy.calls['sx_gp_pack']) == (0, 1, 1), n
        whole = _gp(p, False)
        whole.update_model(X[:n], Y[:n])
        assert spy.calls['sx_gp_append'] == 1
        for got, want in zip(ssm.predict_with_jacobians(z[:, :2], z[:, 2:]), whole.predict_with_jacobians(z[:, :2], z[:, 2:])):
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), **PARITY)
        np.testing.assert_allclose(ssm.information_gain(), whole.information_gain(), **PARITY)
        assert ssm._linv_current and ssm._fit_ws[1].shape == (2, n, n) and ssm._appended == n - 40
    # hyper-parameter training invalidates the factor: that update and the next one fit in full
    spy.calls.clear()
    more = R.problem(2, 1, 3, 1e-4)
    ssm.update_model(WP._dev(more.X[:1]), WP._dev(more.Y[:1]), opt_hyp=True)
    assert spy.calls['sx_gp_append'] == 0 and spy.calls['sx_gp_fit'] >= 1
    spy.calls.clear()
    ssm.update_model(WP._dev(more.X[1:2]), WP._dev(more.Y[1:2]))
    assert (spy.calls['sx_gp_fit'], spy.calls['sx_gp_append']) == (1, 0)
    ssm.update_model(WP._dev(more.X[2:3]), WP._dev(more.Y[2:3]))
    assert (spy.calls['sx_gp_fit'], spy.calls['sx_gp_append']) == (1, 1)


def test_setting_off_is_the_parent_path(monkeypatch):
    p = R.problem(2, 1, 43)
    X, Y = WP._dev(p.X), WP._dev(p.Y)
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', spy)
    ssm = _gp(p, False)
    ssm.update_model(X[:40], Y[:40])
    ssm.update_model(X[40:], Y[40:])
    assert spy.calls['sx_gp_append'] == 0 and spy.calls['sx_gp_append_workspace_bytes'] == 0
    whole = _gp(p, False)
    whole.update_model(X, Y)
    z = WP._dev(R.queries(p, 7, far=False))
    for got, want in zip(ssm.predict_with_jacobians(z[:, :2], z[:, 2:]), whole.predict_with_jacobians(z[:, :2], z[:, 2:])):
        assert torch.equal(got, want)


def test_update_models_multi_equals_single_updates_bit_for_bit():
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import update_models_multi
    probs = [R.problem(2, 1, n) for n in (43, 99, 130)]
    first = (40, 97, 60)                      # model 2 gets 70 rows at once: it does not qualify
    z = WP._dev(R.queries(probs[0], 7, far=False))

    def models():
        out = []
        for p, n in zip(probs, first):
            ssm = _gp(p, True)
            ssm.update_model(WP._dev(p.X[:n]), WP._dev(p.Y[:n]))
            out.append(ssm)
        return out

    alone, together = models(), models()
    xs = [WP._dev(p.X[n:]) for p, n in zip(probs, first)]
    ys = [WP._dev(p.Y[n:]) for p, n in zip(probs, first)]
    for m, x, y in zip(alone, xs, ys):
        m.update_model(x, y)
    update_models_multi(together, xs, ys)
    assert [m._appended for m in together] == [3, 2, 0]
    for a, b in zip(alone, together):
        assert a.x_train.size(0) == b.x_train.size(0)
        for u, v in zip(a.predict_with_jacobians(z[:, :2], z[:, 2:]), b.predict_with_jacobians(z[:, :2], z[:, 2:])):
            assert torch.equal(u, v)
        assert np.array_equal(a.information_gain(), b.information_gain())


def test_safempc_action_after_an_appended_update():
    from safe_exploration_amd import problems
    from safe_exploration_amd.safempc_cem import MpcResult

    class Conf:
        mpc_time_horizon, cem_num_rollouts, cem_num_elites, cem_num_iterations, cem_init_std = 5, 128, 12, 3, 0.2
        device, use_state_constraint, use_prior_model = DEV, True, True
        exact_gp_training_iterations, exact_gp_kernel = 0, 'rbf'
        plot_cem_optimisation = plot_cem_terminal_states = False

    class Incremental(Conf):
        cem_gp_incremental = True

    spec = problems.pendulum(n_train=64, seed=0)
    appended, whole = problems.make_solver(spec, Incremental())[0], problems.make_solver(spec, Conf())[0]
    rng = np.random.default_rng(5)
    x_new, y_new = rng.uniform(-0.3, 0.3, size=(2, 3)), rng.uniform(-0.05, 0.05, size=(2, 2))
    for solver in (appended, whole):
        solver.update_model(x_new, y_new, replace_old=False)
    assert appended._ssm._appended == 2 and whole._ssm._appended == 0
    noise = rng.normal(size=(Conf.cem_num_iterations, Conf.cem_num_rollouts, Conf.mpc_time_horizon, 1))
    x0 = np.array([0.02, -0.03])
    actions = []
    for solver in (appended, whole):
        it = iter(noise)
        solver._solver().sample_noise = lambda episodes=1, it=it: WP._dev(next(it)[None])
        action, result = solver.get_action(x0)
        assert result == MpcResult.FOUND_SOLUTION
        actions.append(action)
    np.testing.assert_allclose(actions[0], actions[1], rtol=0, atol=1e-9)
