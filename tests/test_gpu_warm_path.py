"""GPU: the exact-GP warm path (sx_gp_fit[_multi], sx_gp_mll_grad[_multi], sx_gp_predict_var_jac,
sx_gp_predict_mean_hessian) against the reference of tests/warm_path_reference.py, at the sizes where the one-workgroup
kernel's panels, the blocked path's 64-blocks and the 1024- and 256-thread strides begin or end, at the advertised
limits, at noise / outputscale down to 1e-6, and where K is not positive definite.

Tolerances come from the reference, never from the kernels.  For N <= 410 LAPACK's float64 error against the long-double
reference is computed per quantity and case, e_ref = max|q_64 - q_ld| / max|q_ld|, and the kernels' error against the same
long-double reference must stay within  FACTOR * max(e_ref, 8 eps).  For larger N the same rule holds for the residuals
max|W K W^T - I| and max|K alpha - y| / max|y| against LAPACK's residuals on the same K, and forward quantities are
compared with LAPACK's at the a-priori bound N eps cond_2(K): two backward-stable float64 factorisations differ by no
more, and nothing sharper is known without a wider reference.  FACTOR = 32: another summation order and the 64-wide
blocking change the rounding by a modest factor; a dropped block, a wrong index or a single-precision intermediate is
wrong by 1e6 or more.

Every output buffer ends in a canary of 64 words, and every test checks it.  Each check prints its figures before it
asserts (`pytest -s`): DESIGN.md section 3.5 records the worst of them."""
import ctypes

import numpy as np
import pytest
import torch

import warm_path_reference as R
from safe_exploration_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = 64
FACTOR = 32.0
FLOOR = 8 * R.EPS
BLOCKED_MIN_N = 96      # kBlockedFitMinN: at or below, the one-workgroup kernels


class Buf:
    """An output buffer of `shape` with CANARY words after its end: NaN (float64) or zero (the int32 status words) all
    over, then a fixed bit pattern in the canary."""

    def __init__(self, *shape, dtype=torch.float64):
        n = int(np.prod(shape))
        self.whole = torch.empty(n + CANARY, dtype=dtype, device=DEV)
        self.bits = torch.int64 if dtype == torch.float64 else torch.int32
        self.whole.fill_(float('nan') if dtype == torch.float64 else 0)
        self.whole[n:].view(self.bits).fill_(0x5AFEC0DE5AFEC0DE if dtype == torch.float64 else 0x5AFEC0DE)
        self.t = self.whole[:n].view(*shape)
        self.expected = self.whole[n:].view(self.bits).clone()

    def intact(self):
        return torch.equal(self.whole[self.t.numel():].view(self.bits), self.expected)

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())

    def np(self):
        return self.t.cpu().numpy()


def _path(n):
    return 'one-workgroup' if n <= BLOCKED_MIN_N else 'blocked'


def _struct(p, x, n=None):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = p.n_s, p.n_u, x.size(0) if n is None else n
    _lib.fill(m.inv_ls2, 1.0 / p.ls ** 2)
    _lib.fill(m.outputscale, p.s)
    _lib.fill(m.noise, p.noise)
    m.x_train = x.data_ptr()
    return m


def _buffers(n_s, D, n):
    return dict(work=Buf(n_s, n, n), linv=Buf(n_s, n, n), alpha=Buf(n_s, n), logdet=Buf(n_s), mll=Buf(n_s),
                grad=Buf(n_s, D + 2), status=Buf(1, dtype=torch.int32))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _canaries(b, where):
    for key, buf in b.items():
        assert buf.intact(), f'{where}: the canary after `{key}` was overwritten'


def _healthy(b, where, mll=False):
    """the canaries, every documented element finite, the strictly upper triangle of linv exactly zero"""
    _canaries(b, where)
    for key in ('linv', 'alpha', 'logdet') + (('mll', 'grad') if mll else ()):
        assert bool(torch.isfinite(b[key].t).all()), f'{where}: `{key}` has a non-finite element'
    assert int(torch.count_nonzero(torch.triu(b['linv'].t, 1))) == 0, f'{where}: linv is not lower triangular'


def run_single(p, mll=False):
    """sx_gp_fit (and sx_gp_mll_grad) of one model into canaried buffers"""
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    x, y = _dev(p.X), _dev(p.Y)
    m = _struct(p, x)
    b = _buffers(p.n_s, p.X.shape[1], p.X.shape[0])
    _lib.check(lib.sx_gp_fit(ctypes.byref(m), _lib.ptr(y), _lib.ptr(b['work'].t), _lib.ptr(b['linv'].t),
                             _lib.ptr(b['alpha'].t), _lib.ptr(b['logdet'].t), _lib.ptr(b['status'].t), stream), 'sx_gp_fit')
    if mll:
        _lib.check(lib.sx_gp_mll_grad(ctypes.byref(m), _lib.ptr(y), _lib.ptr(b['linv'].t), _lib.ptr(b['alpha'].t),
                                      _lib.ptr(b['logdet'].t), _lib.ptr(b['work'].t), _lib.ptr(b['mll'].t),
                                      _lib.ptr(b['grad'].t), stream), 'sx_gp_mll_grad')
    torch.cuda.synchronize()
    return b


def run_multi(probs):
    """sx_gp_fit_multi and sx_gp_mll_grad_multi of E problems of one shape: per-problem buffers, and the shared status
    [E], mll [E x n_s] and grad [E x n_s x (D + 2)]"""
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    E, n_s, D = len(probs), probs[0].n_s, probs[0].X.shape[1]
    xs, ys = [_dev(p.X) for p in probs], [_dev(p.Y) for p in probs]
    models = (_lib.SxGpModel * E)(*[_struct(p, x) for p, x in zip(probs, xs)])
    bufs = [{k: v for k, v in _buffers(n_s, D, p.X.shape[0]).items() if k in ('work', 'linv', 'alpha', 'logdet')}
            for p in probs]
    shared = dict(status=Buf(E, dtype=torch.int32), mll=Buf(E, n_s), grad=Buf(E, n_s, D + 2))
    arr = lambda key: (ctypes.c_void_p * E)(*[b[key].t.data_ptr() for b in bufs])
    host = ctypes.create_string_buffer(int(lib.sx_gp_fit_table_bytes(E)))
    _lib.check(lib.sx_gp_fit_table(models, E, (ctypes.c_void_p * E)(*[y.data_ptr() for y in ys]), arr('work'), arr('linv'),
                                   arr('alpha'), arr('logdet'), _lib.ptr(shared['status'].t), _lib.ptr(shared['mll'].t),
                                   _lib.ptr(shared['grad'].t), host), 'sx_gp_fit_table')
    table = torch.tensor(np.frombuffer(host.raw, dtype=np.uint8), device=DEV)
    _lib.check(lib.sx_gp_fit_multi(models, E, _lib.ptr(table), stream), 'sx_gp_fit_multi')
    _lib.check(lib.sx_gp_mll_grad_multi(models, E, _lib.ptr(table), stream), 'sx_gp_mll_grad_multi')
    torch.cuda.synchronize()
    return bufs, shared


# ---- the tolerance rule ----------------------------------------------------------------------------------------------

def rule(entry, case, quantity, got, f64, ld):
    """FACTOR x: the kernel's error against the long-double truth, in units of max(LAPACK's error, 8 eps)"""
    e_ref, e_kernel = R.rel_err(f64, ld), R.rel_err(got, ld)
    ratio = e_kernel / max(e_ref, FLOOR)
    print(f'WARM_PATH 32x {entry} | {quantity} | {case} | e_kernel {e_kernel:.3e} e_ref {e_ref:.3e} ratio {ratio:.2f}')
    assert ratio <= FACTOR, f'{entry} {quantity} {case}: e_kernel {e_kernel:.3e}, e_ref {e_ref:.3e}, ratio {ratio:.1f} > {FACTOR}'


def residual_rule(entry, case, p, ref, linv, alpha):
    """FACTOR x on the two residuals of every output, against LAPACK's residuals on the same K"""
    for d in range(p.n_s):
        mine = R.residuals(ref.K[d], linv[d], alpha[d], p.Y[:, d])
        theirs = R.residuals(ref.K[d], ref.linv[d], ref.alpha[d], p.Y[:, d])
        for name, r, r_ref in zip(('max|W K W^T - I|', 'max|K alpha - y|/max|y|'), mine, theirs):
            ratio = r / max(r_ref, FLOOR)
            print(f'WARM_PATH 32x {entry} | {name} | {case} d={d} | r_kernel {r:.3e} r_ref {r_ref:.3e} ratio {ratio:.2f}')
            assert ratio <= FACTOR, f'{entry} {name} {case} output {d}: {r:.3e} against LAPACK\'s {r_ref:.3e}'


def a_priori(entry, case, quantity, got, f64, n, cond):
    """beyond the long-double reference's reach: against LAPACK at N eps cond_2(K)"""
    e, bound = R.rel_err(got, f64), n * R.EPS * cond
    print(f'WARM_PATH a-priori {entry} | {quantity} | {case} | e_kernel {e:.3e} bound {bound:.3e} (cond {cond:.2e})')
    assert e <= bound, f'{entry} {quantity} {case}: {e:.3e} > N eps cond_2(K) = {bound:.3e}'


def forward(entry, case, p, quantities, got):
    """`quantities` of the kernels' `got` against the reference: the 32x rule where the long-double reference reaches,
    the a-priori bound against LAPACK beyond"""
    n, ref = p.X.shape[0], R.reference(p)
    if R.HAVE_LD and n <= R.LD_MAX_N:
        ld = R.reference(p, True)
        for q in quantities:
            rule(entry, case, q, got[q], getattr(ref, q), getattr(ld, q))
    else:
        cond = max(R.cond2(K) for K in ref.K)
        for q in quantities:
            a_priori(entry, case, q, got[q], getattr(ref, q), n, cond)


def _case(p):
    return '({},{}) N={} ratio={:g}'.format(*p.key)


# ---- a. fit products over the covering set ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape,n', R.fit_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_fit_products(shape, n):
    p = R.problem(*shape, n)
    b = run_single(p)
    assert int(b['status'].t.item()) == 0
    _healthy(b, _case(p))
    got = {k: b[k].np() for k in ('linv', 'alpha', 'logdet')}
    entry = f'sx_gp_fit {_path(n)}'
    forward(entry, _case(p), p, ('linv', 'alpha', 'logdet'), got)
    residual_rule(entry, _case(p), p, R.reference(p), got['linv'], got['alpha'])


# ---- b. the limit ----------------------------------------------------------------------------------------------------

def test_fit_and_mll_grad_at_the_limit():
    p = R.problem(1, 1, R.LIMIT_N)
    ref = R.reference(p)
    b = run_single(p, mll=True)
    assert int(b['status'].t.item()) == 0
    _healthy(b, _case(p), mll=True)
    got = {k: b[k].np() for k in ('linv', 'alpha', 'logdet', 'mll', 'grad')}
    entry = 'sx_gp_fit blocked'
    residual_rule(entry, _case(p), p, ref, got['linv'], got['alpha'])
    cond = R.cond2(ref.K[0])
    a_priori(entry, _case(p), 'logdet', got['logdet'], ref.logdet, R.LIMIT_N, cond)
    for q in ('mll', 'grad'):
        a_priori('sx_gp_mll_grad blocked', _case(p), q, got[q], getattr(ref, q), R.LIMIT_N, cond)


def test_one_point_past_the_limit_is_refused_before_any_write():
    p = R.problem(1, 1, 2)
    x, y = _dev(p.X), _dev(p.Y)
    m = _struct(p, x, n=R.LIMIT_N + 1)
    b = _buffers(1, 2, 2)
    rc = _lib.lib().sx_gp_fit(ctypes.byref(m), _lib.ptr(y), _lib.ptr(b['work'].t), _lib.ptr(b['linv'].t), _lib.ptr(b['alpha'].t),
                              _lib.ptr(b['logdet'].t), _lib.ptr(b['status'].t), _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == _lib.SX_ERR_UNSUPPORTED
    assert all(b[k].untouched() for k in ('work', 'linv', 'alpha', 'logdet'))
    assert b['status'].intact() and int(b['status'].t.item()) == 0


# ---- c. conditioning -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ratio', R.RATIOS)
@pytest.mark.parametrize('n', R.COND_SIZES)
def test_fit_forward_error_over_conditioning(n, ratio):
    p = R.problem(2, 1, n, ratio)
    b = run_single(p)
    assert int(b['status'].t.item()) == 0
    _healthy(b, _case(p))
    forward(f'sx_gp_fit {_path(n)}', _case(p), p, ('linv', 'alpha', 'logdet'), {k: b[k].np() for k in ('linv', 'alpha', 'logdet')})


@pytest.mark.parametrize('ratio', R.RATIOS[1:])
def test_fit_residuals_over_conditioning_n1100(ratio):
    p = R.problem(2, 1, 1100, ratio)
    b = run_single(p)
    assert int(b['status'].t.item()) == 0
    _healthy(b, _case(p))
    residual_rule('sx_gp_fit blocked', _case(p), p, R.reference(p), b['linv'].np(), b['alpha'].np())


# ---- d. MLL and gradient ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', R.SHAPES + R.WIDE_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_mll_grad_single_and_multi(shape):
    """One multi launch over MLL_SIZES and, at the shapes sx_gp_mll_grad takes, a single launch per size: each against
    the closed form, and bit for bit against each other.  The wide shapes go through the multi entry only (DESIGN
    section 3.5): the single entry answers SX_ERR_ARG for them and writes nothing."""
    probs = [R.problem(*shape, n) for n in R.MLL_SIZES]
    wide = shape in R.WIDE_SHAPES
    bufs, shared = run_multi(probs)
    _canaries(shared, f'multi {shape}')
    assert shared['status'].t.cpu().tolist() == [0] * len(probs)
    assert bool(torch.isfinite(shared['mll'].t).all()) and bool(torch.isfinite(shared['grad'].t).all())
    mll, grad = shared['mll'].np(), shared['grad'].np()
    for e, p in enumerate(probs):
        n = p.X.shape[0]
        _healthy(bufs[e], f'multi {_case(p)}')
        forward(f'sx_gp_mll_grad_multi {_path(n)}', _case(p), p, ('mll', 'grad'), dict(mll=mll[e], grad=grad[e]))
        if wide:
            x, y = _dev(p.X), _dev(p.Y)
            m = _struct(p, x)
            out = dict(mll=Buf(p.n_s), grad=Buf(p.n_s, p.X.shape[1] + 2))
            rc = _lib.lib().sx_gp_mll_grad(ctypes.byref(m), _lib.ptr(y), _lib.ptr(bufs[e]['linv'].t), _lib.ptr(bufs[e]['alpha'].t),
                                           _lib.ptr(bufs[e]['logdet'].t), _lib.ptr(bufs[e]['work'].t), _lib.ptr(out['mll'].t),
                                           _lib.ptr(out['grad'].t), _lib.stream_ptr(torch.device(DEV)))
            torch.cuda.synchronize()
            assert rc == _lib.SX_ERR_ARG and out['mll'].untouched() and out['grad'].untouched()
            continue
        b = run_single(p, mll=True)
        assert int(b['status'].t.item()) == 0
        _healthy(b, f'single {_case(p)}', mll=True)
        forward(f'sx_gp_mll_grad {_path(n)}', _case(p), p, ('mll', 'grad'), dict(mll=b['mll'].np(), grad=b['grad'].np()))
        for key in ('linv', 'alpha', 'logdet'):
            assert torch.equal(b[key].t, bufs[e][key].t), (_case(p), key)
        assert torch.equal(b['mll'].t, shared['mll'].t[e]) and torch.equal(b['grad'].t, shared['grad'].t[e]), _case(p)


@pytest.mark.parametrize('ratio', R.RATIOS)
@pytest.mark.parametrize('n', (96, 410))
def test_mll_grad_over_conditioning(n, ratio):
    p = R.problem(2, 1, n, ratio)
    b = run_single(p, mll=True)
    assert int(b['status'].t.item()) == 0
    _healthy(b, _case(p), mll=True)
    forward(f'sx_gp_mll_grad {_path(n)}', _case(p), p, ('mll', 'grad'), dict(mll=b['mll'].np(), grad=b['grad'].np()))


def test_mixed_paths_in_one_multi_launch_are_bitwise_the_single_entries():
    probs = [R.problem(3, 1, n) for n in R.MIX_SIZES]
    bufs, shared = run_multi(probs)
    _canaries(shared, 'multi (3,1)')
    assert shared['status'].t.cpu().tolist() == [0] * len(probs)
    for e, p in enumerate(probs):
        b = run_single(p, mll=True)
        _healthy(b, f'single {_case(p)}', mll=True)
        _healthy(bufs[e], f'multi {_case(p)}')
        for key in ('linv', 'alpha', 'logdet'):
            assert torch.equal(b[key].t, bufs[e][key].t), (_case(p), key)
        assert torch.equal(b['mll'].t, shared['mll'].t[e]) and torch.equal(b['grad'].t, shared['grad'].t[e]), _case(p)


# ---- e. not positive definite, found where it happens ----------------------------------------------------------------

def _assert_fails_exactly_at(p, b):
    for d in range(p.n_s):
        K = R.kmat(p, d)
        np.linalg.cholesky(K[:b, :b])
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(K[:b + 1, :b + 1])


@pytest.mark.parametrize('n,a,b', R.NOT_PD_CASES)
def test_not_positive_definite_is_flagged_where_it_happens(n, a, b):
    """(90, 70): the one-workgroup kernel's third panel; (200, 5): the blocked path's first block; (200, 195): its last,
    partly filled block, a pivot first met in block column 3; (65, 64): the single row past the second 32-column panel.  A status flag on a defined path (the square root
    of a negative pivot, NaN in the problem's own buffers): nothing is read or written out of bounds."""
    p = R.not_pd_problem(n, a, b)
    _assert_fails_exactly_at(p, b)
    bufs = run_single(p)
    _canaries(bufs, f'not PD N={n} b={b}')
    assert int(bufs['status'].t.item()) == _lib.SX_STATUS_NOT_PD


def test_not_positive_definite_problem_keeps_to_itself_in_a_multi_launch():
    n, a, b = R.NOT_PD_CASES[2]
    bad = R.not_pd_problem(n, a, b)
    _assert_fails_exactly_at(bad, b)
    lo, hi = (R.problem(2, 1, m) for m in R.NOT_PD_MULTI)
    bufs, shared = run_multi([lo, bad, hi])
    _canaries(shared, 'multi with a not-PD problem')
    for bb in bufs:
        _canaries(bb, 'multi with a not-PD problem')
    assert shared['status'].t.cpu().tolist() == [0, _lib.SX_STATUS_NOT_PD, 0]
    for e, p in ((0, lo), (2, hi)):
        single = run_single(p, mll=True)
        _healthy(single, _case(p), mll=True)
        _healthy(bufs[e], f'multi {_case(p)}')
        for key in ('linv', 'alpha', 'logdet'):
            assert torch.equal(single[key].t, bufs[e][key].t), (_case(p), key)
        assert torch.equal(single['mll'].t, shared['mll'].t[e]) and torch.equal(single['grad'].t, shared['grad'].t[e])


# ---- f. sx_gp_predict_var_jac and sx_gp_predict_mean_hessian ---------------------------------------------------------

def run_predict(p, linv, alpha, z):
    """both entries at z from device linv / alpha: (jac_var Buf [P x n_s x D], hess Buf [P x n_s x D x D])"""
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    x, zt = _dev(p.X), _dev(z)
    m = _struct(p, x)
    P, D = z.shape
    jac, hess = Buf(P, p.n_s, D), Buf(P, p.n_s, D, D)
    if linv is not None:
        _lib.check(lib.sx_gp_predict_var_jac(ctypes.byref(m), _lib.ptr(linv), _lib.ptr(zt), P, _lib.ptr(jac.t), stream),
                   'sx_gp_predict_var_jac')
    if alpha is not None:
        _lib.check(lib.sx_gp_predict_mean_hessian(ctypes.byref(m), _lib.ptr(alpha), _lib.ptr(zt), P, _lib.ptr(hess.t), stream),
                   'sx_gp_predict_mean_hessian')
    torch.cuda.synchronize()
    return jac, hess


def _check_predict(case, p, z, jac, hess, refs, far):
    """refs = {'jac': (f64, ld), 'hess': (f64, ld)}; `far`: the index of the query beyond all data, or None"""
    assert jac.intact() and hess.intact(), f'{case}: a canary was overwritten'
    assert bool(torch.isfinite(jac.t).all()) and bool(torch.isfinite(hess.t).all()), case
    assert torch.equal(hess.t, hess.t.transpose(2, 3)), f'{case}: the Hessian is not exactly symmetric'
    near = [i for i in range(z.shape[0]) if i != far]
    for name, entry, got in (('jac', 'sx_gp_predict_var_jac', jac.np()), ('hess', 'sx_gp_predict_mean_hessian', hess.np())):
        f64, ld = refs[name]
        rule(entry, case, name, got[near], f64[near], ld[near])
        if far is not None:
            # every k* underflows there: the reference's values are below float64's smallest normal number, and so
            # must the kernel's be (finite, checked above)
            tiny = np.finfo(np.float64).tiny
            assert np.abs(ld[far]).max() < tiny and np.abs(got[far]).max() < tiny, (case, name, got[far])


@pytest.mark.parametrize('n', R.PREDICT_SIZES)
@pytest.mark.parametrize('shape', R.PREDICT_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_var_jac_and_mean_hessian_on_their_own(shape, n):
    """linv and alpha are the float64 reference's, uploaded; the closed forms are evaluated from the same linv and
    alpha in long double (the truth) and in float64 (e_ref)."""
    p = R.problem(*shape, n)
    ref = R.reference(p)
    linv, alpha = _dev(ref.linv), _dev(ref.alpha)
    for P in (1, 3):
        z = R.queries(p, P)
        jac, hess = run_predict(p, linv, alpha, z)
        refs = dict(jac=(R.variance_jacobian(p, ref.linv, z), R.variance_jacobian(p, ref.linv, z, R.LD)),
                    hess=(R.mean_hessian(p, ref.alpha, z), R.mean_hessian(p, ref.alpha, z, R.LD)))
        _check_predict(f'{_case(p)} P={P}', p, z, jac, hess, refs, far=2 if P == 3 else None)


def test_var_jac_and_mean_hessian_from_the_fit():
    """sx_gp_fit's own linv and alpha, against the closed forms of the long-double factorisation; e_ref: those of LAPACK's"""
    p = R.problem(2, 2, 257)
    b = run_single(p)
    _healthy(b, _case(p))
    z = R.queries(p, 3)
    jac, hess = run_predict(p, b['linv'].t, b['alpha'].t, z)
    ref, ld = R.reference(p), R.reference(p, True)
    refs = dict(jac=(R.variance_jacobian(p, ref.linv, z), R.variance_jacobian(p, ld.linv, z, R.LD)),
                hess=(R.mean_hessian(p, ref.alpha, z), R.mean_hessian(p, ld.alpha, z, R.LD)))
    _check_predict(f'{_case(p)} from sx_gp_fit', p, z, jac, hess, refs, far=2)


def test_var_jac_past_64_kb_of_lds_and_again_with_the_grant_remembered():
    """N = 4160: 2 N doubles are 66 560 bytes, the smallest N on a 64-row grid that needs the allow_lds grant"""
    p = R.problem(1, 1, R.VAR_JAC_LDS_N)
    W = R.reference(p).linv
    linv = _dev(W)
    z = R.queries(p, 2)
    first, _ = run_predict(p, linv, None, z)
    second, _ = run_predict(p, linv, None, z)
    assert first.intact() and second.intact() and bool(torch.isfinite(first.t).all())
    assert torch.equal(first.t, second.t)
    rule('sx_gp_predict_var_jac', f'{_case(p)} P=2', 'jac', first.np(), R.variance_jacobian(p, W, z),
         R.variance_jacobian(p, W, z, R.LD))


def test_var_jac_past_its_limit_is_refused_before_any_write():
    p = R.problem(1, 1, 2)
    x, z = _dev(p.X), _dev(R.queries(p, 1))
    m = _struct(p, x, n=8193)
    jac = Buf(1, 1, 2)
    rc = _lib.lib().sx_gp_predict_var_jac(ctypes.byref(m), _lib.ptr(x), _lib.ptr(z), 1, _lib.ptr(jac.t),
                                          _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == _lib.SX_ERR_UNSUPPORTED and jac.untouched()
