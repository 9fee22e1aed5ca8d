"""CPU: sx_gp_append, host side.  The declarations of _lib.py against include/sx_amd.h; the codes the entry answers bad
arguments with, before any device access (the pointers are placeholders nothing dereferences); with a counting fake in
place of the library, when GpCemSSM takes the append path (conf.cem_gp_incremental) and when it fits in full; and the
algebra itself (tests/append_reference.py) in long double against the long-double factorisation of the full set."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import append_reference as A
import warm_path_reference as R
from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem import gp_ssm_cem
from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM, update_models_multi

ARG, UNSUPPORTED, OK = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED, _lib.SX_OK
_P = ctypes.c_void_p(16)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sx_amd.h')


@pytest.fixture(autouse=True)
def the_feature():
    """Every test of this file is about sx_gp_append and conf.cem_gp_incremental: none passes on a tree without them."""
    assert 'sx_gp_append' in _lib.SIGNATURES and 'sx_gp_append_workspace_bytes' in _lib.SIGNATURES
    assert hasattr(_lib.lib(), 'sx_gp_append') and hasattr(gp_ssm_cem, 'MAX_APPEND_ROWS')
    assert GpCemSSM(Conf(), 2, 1)._incremental is True


# ---- declarations ----------------------------------------------------------------------------------------------------------

def _ctype(decl):
    decl = decl.strip()
    if '*' in decl:
        return ctypes.POINTER(_lib.SxGpModel) if 'sx_gp_model' in decl else ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[decl.rsplit(' ', 1)[0].strip()]


@pytest.mark.parametrize('name', ['sx_gp_append', 'sx_gp_append_workspace_bytes'])
def test_declarations_match_the_header(name):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ret, args = re.search(r'(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', text).groups()
    res, argtypes = _lib.SIGNATURES[name]
    assert res is {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[ret]
    assert argtypes == [_ctype(a) for a in args.split(',')]
    assert getattr(_lib.lib(), name).argtypes == argtypes


# ---- argument errors, without a device -------------------------------------------------------------------------------------

def _model(n_s=2, n_u=1, n_train=11):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train, m.n_pad = n_s, n_u, n_train, 0
    m.x_train = 16
    return m


def _call(model, n_old=10, nulls=(), ws_bytes=None):
    lib = _lib.lib()
    bufs = [None if i in nulls else _P for i in range(9)]   # y, linv_old, alpha_old, logdet_old, linv, alpha, logdet, status, ws
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.sx_gp_append(ctypes.byref(model) if model is not None else None, n_old, *bufs, ws_bytes, None)


def test_append_answers_before_any_device_access():
    assert _call(None) == ARG
    for i in range(9):
        assert _call(_model(), nulls=(i,)) == ARG, i
    no_x = _model()
    no_x.x_train = None
    assert _call(no_x) == ARG
    for bad in (dict(n_s=0), dict(n_s=5), dict(n_u=0), dict(n_s=2, n_u=5), dict(n_train=0), dict(n_train=-3)):
        assert _call(_model(**bad)) == ARG, bad
    assert _call(_model(), n_old=0) == ARG and _call(_model(), n_old=-1) == ARG
    assert _call(_model(n_train=10), n_old=10) == ARG                     # k = 0
    assert _call(_model(n_train=9), n_old=10) == ARG                      # k < 0
    assert _call(_model(n_train=75), n_old=10) == ARG                     # k = 65
    need = int(_lib.lib().sx_gp_append_workspace_bytes(2, 11, 1))
    assert need > 0
    assert _call(_model(), ws_bytes=need - 1) == ARG and _call(_model(), ws_bytes=0) == ARG
    assert _call(_model(n_train=4097), n_old=4096) == UNSUPPORTED
    assert _call(_model(n_train=4097, n_s=1, n_u=5), n_old=4090) == UNSUPPORTED     # the wide shape is accepted: only N refuses
    assert _call(_model(n_train=4097), n_old=4096, nulls=(3,)) == ARG     # argument errors answer first
    assert _call(_model(n_train=4097), n_old=4000) == ARG


def test_workspace_bytes():
    fn = _lib.lib().sx_gp_append_workspace_bytes
    for bad in ((0, 11, 1), (5, 11, 1), (2, 11, 0), (2, 80, 65), (2, 11, 11), (2, 5, 6), (2, 4097, 1), (2, -1, 1)):
        assert fn(*bad) < 0, bad
    assert fn(2, 2, 1) > 0 and fn(4, 4096, 64) > 0 and fn(1, 4096, 1) > 0
    assert fn(2, 1011, 11) == fn(2, 1001, 1)                               # a function of (n_s, N) alone
    assert fn(2, 2001, 1) > fn(2, 1001, 1) and fn(4, 1001, 1) == 2 * fn(2, 1001, 1)
    assert fn(2, 2001, 1) >= 2 * 2 * 2000 * 64 * 8                          # K_c and B


# ---- which path GpCemSSM takes, with a counting fake in place of the library ------------------------------------------------

class FakeLib:
    """Every entry counted; the host-only size queries answer for real, every other entry answers SX_OK and touches
    nothing -- but for sx_gp_append, which writes `append_status` into its status word (a host tensor here)."""
    HOST_ONLY = ('_bytes', '_sizes')

    def __init__(self, lib):
        self._lib, self.calls, self.append_status = lib, collections.Counter(), 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            if name.endswith(self.HOST_ONLY):
                return fn(*args)
            if name == 'sx_gp_append':
                ctypes.cast(args[9], ctypes.POINTER(ctypes.c_int32))[0] |= self.append_status
            return OK
        return counted


class Conf:
    device = 'cpu'
    exact_gp_kernel = 'rbf'
    exact_gp_training_iterations = 0

    def __init__(self, incremental=True, **kw):
        if incremental is not None:
            self.cem_gp_incremental = incremental
        for key, v in kw.items():
            setattr(self, key, v)


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: lib)
    monkeypatch.setattr(_lib, 'require_gpu', lambda *a: None)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda dev: None)
    return lib


def _rows(n, seed=0, n_s=2, n_u=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, n_s + n_u), dtype=torch.float64, generator=g),
            torch.rand((n, n_s), dtype=torch.float64, generator=g))


def _fitted(fake, n=20, **kw):
    ssm = GpCemSSM(Conf(**kw), 2, 1)
    ssm.update_model(*_rows(n))
    assert (fake.calls['sx_gp_fit'], fake.calls['sx_gp_append']) == (1, 0)
    fake.calls.clear()
    return ssm


def _counts(fake):
    got = (fake.calls['sx_gp_fit'], fake.calls['sx_gp_append'])
    fake.calls.clear()
    return got


def test_second_update_appends_and_never_fits(fake):
    ssm = _fitted(fake)
    ssm.update_model(*_rows(1, seed=1))
    assert fake.calls['sx_gp_pack'] == 1 and _counts(fake) == (0, 1)
    ssm.update_model(*_rows(64, seed=2))
    assert fake.calls['sx_gp_pack'] == 1 and _counts(fake) == (0, 1)
    assert ssm.x_train.size(0) == 85 and ssm.device_model.n_train == 85
    assert ssm._fit_ws[1].shape == (2, 85, 85) and ssm._alpha.shape == (2, 85)
    ssm.update_model(*_rows(3, seed=3))
    assert _counts(fake) == (0, 1) and ssm._appended == 68


@pytest.mark.parametrize('incremental', [False, None])
def test_setting_off_never_appends(fake, incremental):
    ssm = GpCemSSM(Conf(incremental), 2, 1)
    for seed, n in enumerate((20, 1, 5, 1)):
        ssm.update_model(*_rows(n, seed=seed))
    assert _counts(fake) == (4, 0)


def test_fall_backs_fit_in_full(fake):
    ssm = _fitted(fake)
    ssm.update_model(*_rows(65, seed=1))                                   # k = 65
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(0, seed=1))                                    # k = 0
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(10, seed=2), replace_old=True)                 # other rows
    assert _counts(fake) == (1, 0)
    x, y = (torch.cat(p) for p in zip((ssm.x_train, ssm.y_train), _rows(1, seed=2)))
    ssm.update_model(x, y, replace_old=True)      # replace_old is a full fit even where the data extend the fitted rows
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(1, seed=3))
    assert _counts(fake) == (0, 1)
    ssm.set_hyperparameters(lengthscale=0.7)                               # refits at once, in full
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(1, seed=4))
    assert _counts(fake) == (0, 1)
    ssm.load_state_dict(ssm.state_dict())
    assert _counts(fake) == (1, 0)
    ssm.mll_and_grad(ssm.x_train, ssm.y_train)                             # reuses the fit workspace: the factor is gone
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(1, seed=5))
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(1, seed=6))
    assert _counts(fake) == (0, 1)
    ssm.update_model(*_rows(1, seed=7), opt_hyp=True)                      # (0 training iterations: the update itself)
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(1, seed=8))                                    # ... and the next update is a full fit too
    assert _counts(fake) == (1, 0)
    ssm.update_model(*_rows(1, seed=9))
    assert _counts(fake) == (0, 1)
    ssm._y_train = ssm._y_train.clone()
    ssm._y_train[3, 0] += 1.0                                              # the stored targets are not the fitted ones
    ssm.update_model(*_rows(1, seed=10))
    assert _counts(fake) == (1, 0)
    ssm._raw_noise = ssm._raw_noise + 0.1                                  # hyper-parameters moved behind the model's back
    ssm.update_model(*_rows(1, seed=11))
    assert _counts(fake) == (1, 0)


def test_limits_of_the_decision(fake, monkeypatch):
    ssm = _fitted(fake, n=20, cem_gp_subset_size=25)
    x, y = (torch.cat(p) for p in zip((ssm.x_train, ssm.y_train), _rows(5, seed=1)))
    assert ssm._append_rows(x, y) == 5                                     # 25 rows: nothing is selected
    x6, y6 = (torch.cat(p) for p in zip((ssm.x_train, ssm.y_train), _rows(6, seed=1)))
    assert ssm._append_rows(x6, y6) == 0                                   # 26 rows: the update selects a subset
    monkeypatch.setattr(gp_ssm_cem, 'MAX_TRAINING_POINTS', 24)
    assert ssm._append_rows(x, y) == 0                                     # N + k beyond the fit's limit
    monkeypatch.setattr(gp_ssm_cem, 'MAX_TRAINING_POINTS', 4096)
    ssm._linv_current = False
    assert ssm._append_rows(x, y) == 0


def test_max_chain_bounds_the_rows_between_full_fits(fake):
    ssm = _fitted(fake, cem_gp_incremental_max_chain=3)
    seen = []
    for seed in range(1, 9):
        ssm.update_model(*_rows(1, seed=seed))
        seen.append(_counts(fake))
    assert seen == [(0, 1)] * 3 + [(1, 0)] + [(0, 1)] * 3 + [(1, 0)]
    ssm.update_model(*_rows(4, seed=20))                                   # more than the chain allows at once
    assert _counts(fake) == (1, 0)
    with pytest.raises(ValueError):
        GpCemSSM(Conf(cem_gp_incremental_max_chain=-1), 2, 1)
    assert GpCemSSM(Conf(), 2, 1)._max_chain is None                       # the default: no limit


def test_lockstep_training_invalidates_the_factor_as_the_single_update_does(fake, monkeypatch):
    """update_models_multi(opt_hyp=True) trains in lockstep; like update_model(opt_hyp=True) it leaves a model whose next
    update is a full fit, so that the two ways stay equal bit for bit."""
    real_empty = torch.empty     # (the lockstep fit's problem table sits in pinned memory, which needs a device)
    monkeypatch.setattr(torch, 'empty', lambda *a, pin_memory=False, **kw: real_empty(*a, **kw))
    seen = {}
    for way in ('multi', 'single'):
        ssms = [GpCemSSM(Conf(), 2, 1), GpCemSSM(Conf(), 2, 1)]
        for e, m in enumerate(ssms):
            m.update_model(*_rows(20 + e, seed=e))
        new = [_rows(2, seed=10 + e) for e in range(2)]
        if way == 'multi':
            update_models_multi(ssms, [x for x, _ in new], [y for _, y in new], opt_hyp=True)
        else:
            for m, (x, y) in zip(ssms, new):
                m.update_model(x, y, opt_hyp=True)
        assert not any(m._append_ok for m in ssms)
        fake.calls.clear()
        for e, m in enumerate(ssms):
            m.update_model(*_rows(1, seed=20 + e))
        seen[way] = _counts(fake)
        for e, m in enumerate(ssms):                                       # ... and the update after that appends again
            m.update_model(*_rows(1, seed=30 + e))
        assert _counts(fake) == (0, 2)
    assert seen == {'multi': (2, 0), 'single': (2, 0)}


def test_update_models_multi_decides_once_per_model(fake, monkeypatch):
    ssms = [GpCemSSM(Conf(), 2, 1), GpCemSSM(Conf(), 2, 1)]
    for e, m in enumerate(ssms):
        m.update_model(*_rows(20 + e, seed=e))
    asked = collections.Counter()
    real = GpCemSSM._append_rows
    monkeypatch.setattr(GpCemSSM, '_append_rows', lambda self, x, y: (asked.update([id(self)]), real(self, x, y))[1])
    new = [_rows(2, seed=10 + e) for e in range(2)]
    fake.calls.clear()
    update_models_multi(ssms, [x for x, _ in new], [y for _, y in new])
    assert _counts(fake) == (0, 2) and sorted(asked.values()) == [1, 1]
    assert [m.x_train.size(0) for m in ssms] == [22, 23] and [m._appended for m in ssms] == [2, 2]


def test_not_pd_append_packs_nothing_from_the_unspecified_outputs(fake):
    ssm = _fitted(fake)
    fake.append_status = _lib.SX_STATUS_NOT_PD
    ssm.update_model(*_rows(1, seed=1))
    assert fake.calls['sx_gp_pack'] == 1 and _counts(fake) == (1, 1)       # the fallback fit's pack alone


def test_not_pd_append_falls_back_to_the_full_fit(fake):
    ssm = _fitted(fake)
    before = ssm.device_model
    fake.append_status = _lib.SX_STATUS_NOT_PD
    ssm.update_model(*_rows(1, seed=1))
    assert _counts(fake) == (1, 1)
    assert ssm.device_model is not before and ssm.device_model.n_train == 21 and ssm._appended == 0


def test_update_models_multi_appends_model_by_model(fake, monkeypatch):
    real_empty = torch.empty     # (the lockstep fit's problem table sits in pinned memory, which needs a device)
    monkeypatch.setattr(torch, 'empty', lambda *a, pin_memory=False, **kw: real_empty(*a, **kw))
    ssms =[GpCemSSM(Conf(), 2, 1), GpCemSSM(Conf(False), 2, 1), GpCemSSM(Conf(), 2, 1)]
    for e, m in enumerate(ssms):
        m.update_model(*_rows(20 + e, seed=e))
    fake.calls.clear()
    ssms[2].set_hyperparameters(noise=0.2)
    ssms[2]._append_ok = False                                             # model 2 does not qualify
    fake.calls.clear()
    new = [_rows(2, seed=10 + e) for e in range(3)]
    update_models_multi(ssms, [x for x, _ in new], [y for _, y in new])
    assert fake.calls['sx_gp_append'] == 1 and fake.calls['sx_gp_fit'] == 0
    assert fake.calls['sx_gp_fit_multi'] == 1 and fake.calls['sx_gp_pack'] == 3
    assert [m.device_model.n_train for m in ssms] == [22, 23, 24]


# ---- the algebra -----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not R.HAVE_LD, reason='long double is no wider than double on this platform')
@pytest.mark.parametrize('shape,n,k,ratio', [((2, 1), 40, 1, 1e-2), ((2, 1), 65, 37, 1e-6), ((1, 5), 64, 1, 1e-2),
                                             ((4, 2), 30, 64, 1e-4)])
def test_long_double_append_is_the_long_double_fit_of_the_full_set(shape, n, k, ratio):
    """Both are exact but for long-double rounding, so they agree to N eps_ld cond_2(K) (the rule of
    test_warm_path_reference_host.py, with long double's eps), and the appended factor reproduces the identity to the
    1e-16 that file asks of its own W L - I."""
    p = R.problem(*shape, n + k, ratio)
    full, got = R.reference(p, True), A.append(p, n, R.LD)
    assert got.linv.dtype == np.longdouble
    eps_ld = float(np.finfo(np.longdouble).eps)
    bound = (n + k) * eps_ld * max(R.cond2(K) for K in full.K)
    for key in ('linv', 'alpha', 'logdet'):
        err = R.rel_err(getattr(got, key), getattr(full, key))
        print(f'APPEND ld {shape} N={n} k={k} ratio={ratio:g} | {key} | {err:.3e} bound {bound:.3e}')
        assert err <= bound, key
    for d in range(p.n_s):
        W, K = got.linv[d], full.K[d]
        # (evaluated in long double, whose own rounding in the two products is bounded by N eps_ld |W| |K| |W^T|: 1e-16 at
        # the size and conditioning that file checks, more where W is larger)
        rounding = (n + k) * eps_ld * float((np.abs(W) @ np.abs(K) @ np.abs(W.T)).max())
        assert np.abs(W @ K @ W.T - np.eye(n + k)).max() < max(1e-16, rounding)
        assert np.count_nonzero(np.triu(W, 1)) == 0
        assert np.array_equal(W[:n, :n], R.Reference(A.head(p, n), R.LD).linv[d]) and not W[:n, n:].any()


@pytest.mark.skipif(not R.HAVE_LD, reason='long double is no wider than double on this platform')
def test_plain_float64_product_with_the_inverse_sets_the_error_of_the_new_rows():
    """Why append_b_kernel accumulates B = W K_c in twice the working precision.  (1,1), N = 130 + 37,
    noise / outputscale = 1e-6, from the long-double factor of the first 130 rows rounded to float64, every step in float64:
    with B accumulated in plain float64 the error of W' against the long-double truth is several times what it is with B
    accumulated in long double and rounded once (12.6 against 3.3 times LAPACK's error of a fresh factorisation): |W| |K_c|
    exceeds |B| by up to the condition number of L, and every other step together adds less than that one product.  At
    least a factor 2 is asserted -- the product with the inverse must be the dominant term, not one of several."""
    p, n = R.problem(1, 1, 167, 1e-6), 130
    f64, ld = R.reference(p), R.reference(p, True)
    e_ref = R.rel_err(f64.linv, ld.linv)
    exact = R.Reference(A.head(p, n), R.LD)
    start = A.Appended(exact.linv.astype(R.F64), exact.alpha.astype(R.F64), exact.logdet.astype(R.F64))
    plain = R.rel_err(A.append(p, n, R.F64, start=start).linv, ld.linv) / e_ref
    careful = R.rel_err(A.append(p, n, R.F64, start=start, b_dtype=R.LD).linv, ld.linv) / e_ref
    print(f'APPEND B = W K_c | plain float64 {plain:.2f} x LAPACK, accumulated in long double {careful:.2f} x')
    assert plain >= 2 * careful and careful <= 32


def test_float64_append_and_chain_agree_with_lapack_to_the_conditioning():
    p = R.problem(2, 1, 48, 1e-4)
    full = R.reference(p)
    bound = 48 * R.EPS * max(R.cond2(K) for K in full.K)
    for got in (A.append(p, 40), A.chain(p, 40)):
        for key in ('linv', 'alpha', 'logdet'):
            assert R.rel_err(getattr(got, key), getattr(full, key)) <= bound, key


def test_reference_meets_the_pivot_that_is_not_positive():
    p = R.not_pd_problem(70, 5, 65)
    R.Reference(A.head(p, 65), R.F64)                                      # the fitted rows are healthy
    with pytest.raises(np.linalg.LinAlgError, match='pivot 0'):
        A.append(p, 65)
