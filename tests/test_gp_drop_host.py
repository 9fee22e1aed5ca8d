"""CPU: sx_gp_drop, host side.  The declarations of _lib.py against include/sx_amd.h; the codes the entry answers bad arguments
with, before any device access (the pointers are placeholders nothing dereferences); the algebra itself
(tests/drop_reference.py) in long double against the long-double factorisation of the kept rows, and in float64 within the
allowance of tests/test_gpu_warm_path.py; and, with a counting fake in place of the library, when GpCemSSM slides its window
(conf.cem_gp_window) and when it fits the last m rows in full."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import drop_reference as D
import warm_path_reference as R
from test_gpu_warm_path import FACTOR, FLOOR
from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem import gp_ssm_cem
from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM, update_models_multi

ARG, UNSUPPORTED, OK = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED, _lib.SX_OK
_P = ctypes.c_void_p(16)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sx_amd.h')


# ---- a. declarations and argument errors, without a device -----------------------------------------------------------------

def _ctype(decl):
    decl = decl.strip()
    if '*' in decl:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[decl.rsplit(' ', 1)[0].strip()]


@pytest.mark.parametrize('name', ['sx_gp_drop', 'sx_gp_drop_workspace_bytes'])
def test_declarations_match_the_header(name):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ret, args = re.search(r'(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', text).groups()
    res, argtypes = _lib.SIGNATURES[name]
    assert res is {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[ret]
    assert argtypes == [_ctype(a) for a in args.split(',')]
    assert getattr(_lib.lib(), name).argtypes == argtypes


def _call(n_s=2, n_old=11, k=1, nulls=(), ws_bytes=1 << 40):
    bufs = [None if i in nulls else _P for i in range(7)]   # y, linv_old, linv, alpha, logdet, status, workspace
    return _lib.lib().sx_gp_drop(n_s, n_old, k, *bufs, ws_bytes, None)


def test_drop_answers_before_any_device_access():
    for i in range(7):
        assert _call(nulls=(i,)) == ARG, i
    for bad in (dict(n_s=0), dict(n_s=5), dict(n_s=-1), dict(k=0), dict(k=-2), dict(k=65, n_old=100), dict(n_old=1, k=1),
                dict(n_old=5, k=5), dict(n_old=5, k=6), dict(n_old=0), dict(n_old=-4)):
        assert _call(**bad) == ARG, bad
    need = int(_lib.lib().sx_gp_drop_workspace_bytes(2, 11, 1))
    assert need > 0
    assert _call(ws_bytes=need - 1) == ARG and _call(ws_bytes=0) == ARG and _call(ws_bytes=-8) == ARG
    assert _call(n_old=4097) == UNSUPPORTED and _call(n_old=5000, k=64, n_s=4) == UNSUPPORTED
    assert _call(n_old=4097, nulls=(2,)) == ARG          # argument errors answer first
    assert _call(n_old=4097, k=65) == ARG
    assert _call(n_old=4097, ws_bytes=8) == ARG


def test_workspace_bytes():
    fn = _lib.lib().sx_gp_drop_workspace_bytes
    for bad in ((0, 11, 1), (5, 11, 1), (2, 11, 0), (2, 80, 65), (2, 11, 11), (2, 5, 6), (2, 4097, 1), (2, -1, 1), (2, 1, 1)):
        assert fn(*bad) < 0, bad
    assert fn(2, 2, 1) > 0 and fn(4, 4096, 64) > 0 and fn(1, 4096, 1) > 0
    for n_s, n, k, stages in ((2, 11, 1, 1), (1, 4096, 64, 64), (4, 130, 37, 64), (2, 70, 5, 8), (2, 70, 2, 2), (3, 99, 33, 64),
                              (3, 99, 32, 32)):
        m = n - k
        # L11, V [m x 64], the (u, dinv, coef) of every row and compiled stage (the power of two >= k), t [m]
        assert fn(n_s, n, k) == 8 * n_s * (64 * 64 + m * 64 + 3 * m * stages + m), (n_s, n, k)
    assert fn(4, 1001, 1) == 2 * fn(2, 1001, 1) and fn(2, 2001, 1) > fn(2, 1001, 1) and fn(2, 1002, 2) > fn(2, 1001, 1)


# ---- b. the algebra ----------------------------------------------------------------------------------------------------------

PAIRS = ((2, 1), (6, 1), (65, 1), (66, 2), (97, 33), (130, 37), (167, 37), (193, 64), (257, 1), (410, 64))
ALGEBRA = [((2, 1), pair, ratio) for pair in PAIRS for ratio in (1e-2, 1e-6)] \
    + [(sh, pair, 1e-6) for sh in ((1, 1), (4, 2)) for pair in ((6, 1), (66, 2), (130, 37))]


@pytest.mark.skipif(not R.HAVE_LD, reason='long double is no wider than double on this platform')
@pytest.mark.parametrize('shape,pair,ratio', ALGEBRA, ids=lambda v: str(v).replace(' ', ''))
def test_drop_in_long_double_is_the_fit_of_the_tail_and_float64_keeps_the_rule(shape, pair, ratio):
    """The long-double drop and the long-double fit of the kept rows are both exact but for long-double rounding: they agree
    to N eps_ld cond_2(K) (the rule of test_gp_append_host.py).  The float64 drop from LAPACK's factor of all N rows stays
    within FACTOR times max(LAPACK's own error on the kept rows, 8 eps) against the long-double truth, both ways of forming
    L11.  (The (1,1) and (4,2) shapes run three of the pairs.  Each figure is printed before it is asserted.)"""
    n, k = pair
    p = R.problem(*shape, n, ratio)
    kept = D.tail(p, k)
    truth, lapack = R.reference(kept, True), R.reference(kept)
    got = D.drop(p, k, R.LD, start=R.reference(p, True))
    assert got.linv.dtype == np.longdouble
    eps_ld = float(np.finfo(np.longdouble).eps)
    bound = n * eps_ld * max(R.cond2(K) for K in R.reference(p).K)
    for key in ('linv', 'alpha', 'logdet'):
        err = R.rel_err(getattr(got, key), getattr(truth, key))
        print(f'DROP ld {shape} N={n} k={k} ratio={ratio:g} | {key} | {err:.3e} bound {bound:.3e}')
        assert err <= bound, key
    for d in range(p.n_s):
        assert np.count_nonzero(np.triu(got.linv[d], 1)) == 0
    for l11 in ('inverse', 'chol'):
        f64 = D.drop(p, k, R.F64, start=R.reference(p), l11=l11)
        assert f64.linv.dtype == np.float64
        for key in ('linv', 'alpha', 'logdet'):
            e_ref = R.rel_err(getattr(lapack, key), getattr(truth, key))
            ratio_ = R.rel_err(getattr(f64, key), getattr(truth, key)) / max(e_ref, FLOOR)
            print(f'DROP f64 L11={l11} {shape} N={n} k={k} ratio={ratio:g} | {key} | e_ref {e_ref:.3e} ratio {ratio_:.2f}')
            assert ratio_ <= FACTOR, (l11, key, ratio_)


def test_reference_refuses_a_w11_that_is_no_factor():
    p = R.problem(2, 1, 12)
    ref = R.reference(p)
    for value in (np.nan, np.inf, -1.0, 0.0):
        linv = ref.linv.copy()
        linv[0, 1, 1] = value
        with pytest.raises(np.linalg.LinAlgError):
            D.drop(p, 3, start=D.Dropped(linv, ref.alpha, ref.logdet))


# ---- c. which path GpCemSSM takes, with a counting fake in place of the library ---------------------------------------------

class FakeLib:
    """Every entry counted; the host-only size queries answer for real, every other entry answers SX_OK and touches nothing --
    but for sx_gp_drop and sx_gp_append, which or `drop_status` / `append_status` into their status word (a host tensor
    here)."""
    HOST_ONLY = ('_bytes', '_sizes')
    STATUS_ARG = {'sx_gp_drop': 8, 'sx_gp_append': 9}

    def __init__(self, lib):
        self._lib, self.calls, self.status, self.args = lib, collections.Counter(), {}, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            self.args[name] = args
            if name.endswith(self.HOST_ONLY):
                return fn(*args)
            if name in self.STATUS_ARG:
                ctypes.cast(args[self.STATUS_ARG[name]], ctypes.POINTER(ctypes.c_int32))[0] |= self.status.get(name, 0)
            return OK
        return counted


class Conf:
    device = 'cpu'
    exact_gp_kernel = 'rbf'
    exact_gp_training_iterations = 0

    def __init__(self, window=25, incremental=True, **kw):
        if window is not None:
            self.cem_gp_window = window
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


def _counts(fake):
    got = (fake.calls['sx_gp_fit'], fake.calls['sx_gp_drop'], fake.calls['sx_gp_append'], fake.calls['sx_gp_pack'])
    fake.calls.clear()
    return got


def _fitted(fake, n=25, **kw):
    ssm = GpCemSSM(Conf(**kw), 2, 1)
    ssm.update_model(*_rows(n))
    assert _counts(fake) == (1, 0, 0, 1)
    return ssm


def _fitted_on(ssm, rows_x, rows_y):
    """the model's device rows are exactly these"""
    return torch.equal(ssm._buffers[0], rows_x) and torch.equal(ssm._fit_state[0], rows_y) \
        and torch.equal(ssm.x_train, rows_x) and torch.equal(ssm.y_train, rows_y)


def test_bad_settings_raise_at_construction():
    for kw in (dict(window=0), dict(window=-3), dict(window=4097), dict(incremental=False), dict(incremental=None),
               dict(cem_gp_subset_size=20), dict(cem_gp_window_max_chain=-1)):
        with pytest.raises(ValueError):
            GpCemSSM(Conf(**kw), 2, 1)
    ssm = GpCemSSM(Conf(window=4096), 2, 1)
    assert ssm._window == 4096 and ssm._window_max_chain == gp_ssm_cem.WINDOW_MAX_CHAIN
    assert GpCemSSM(Conf(window=1, cem_gp_window_max_chain=None), 2, 1)._window_max_chain is None
    assert GpCemSSM(Conf(window=None), 2, 1)._window is None


def test_a_slide_drops_once_appends_once_and_never_fits(fake):
    ssm = _fitted(fake)
    all_x, all_y = ssm.x_train, ssm.y_train
    for seed, k in ((1, 1), (2, 3), (3, 16)):
        x, y = _rows(k, seed=seed)
        ssm.update_model(x, y)
        assert _counts(fake) == (0, 1, 1, 1), k
        all_x, all_y = torch.cat((all_x, x)), torch.cat((all_y, y))
        assert _fitted_on(ssm, all_x[-25:], all_y[-25:])
        n_s, n_old, r = fake.args['sx_gp_drop'][:3]
        assert (n_s, n_old, r) == (2, 25, k)
        assert fake.args['sx_gp_append'][1] == 25 - k and ssm.device_model.n_train == 25
        assert ssm._fit_ws[1].shape == (2, 25, 25) and ssm._alpha.shape == (2, 25)
    assert ssm._appended == 20


def test_below_the_window_the_model_appends_and_then_slides_the_overflow(fake):
    ssm = _fitted(fake, n=20)
    ssm.update_model(*_rows(3, seed=1))                                    # 23 rows: r = -2
    assert _counts(fake) == (0, 0, 1, 1) and ssm.x_train.size(0) == 23
    ssm.update_model(*_rows(2, seed=2))                                    # 25 rows: r = 0
    assert _counts(fake) == (0, 0, 1, 1) and ssm.x_train.size(0) == 25
    ssm.update_model(*_rows(1, seed=3))
    assert _counts(fake) == (0, 1, 1, 1) and ssm.x_train.size(0) == 25
    ssm2 = _fitted(fake, n=20)
    ssm2.update_model(*_rows(8, seed=4))                                   # 28 rows: drops 3 and appends 8
    assert _counts(fake) == (0, 1, 1, 1) and ssm2.x_train.size(0) == 25
    assert fake.args['sx_gp_drop'][:3] == (2, 20, 3) and fake.args['sx_gp_append'][1] == 17


def test_every_update_trims_and_each_fall_back_is_one_full_fit_of_the_last_m_rows(fake):
    ssm = GpCemSSM(Conf(), 2, 1)
    x0, y0 = _rows(40)
    ssm.update_model(x0, y0)                                               # the first update: more rows than the window
    assert _counts(fake) == (1, 0, 0, 1) and _fitted_on(ssm, x0[-25:], y0[-25:])
    all_x, all_y = x0, y0

    def update(k, seed, want, **kw):
        nonlocal all_x, all_y
        x, y = _rows(k, seed=seed)
        ssm.update_model(x, y, **kw)
        all_x, all_y = (x, y) if kw.get('replace_old') else (torch.cat((all_x, x)), torch.cat((all_y, y)))
        assert _counts(fake) == want, (k, seed, kw)
        assert _fitted_on(ssm, all_x[-25:], all_y[-25:]) and ssm.device_model.n_train == min(25, all_x.size(0))

    update(1, 1, (0, 1, 1, 1))
    update(25, 2, (1, 0, 0, 1))                                            # r = 25 = N: nothing of the fit is kept
    update(16, 3, (0, 1, 1, 1))
    update(30, 4, (1, 0, 0, 1), replace_old=True)
    update(1, 5, (0, 1, 1, 1))
    update(1, 6, (1, 0, 0, 1), opt_hyp=True)                               # (0 training iterations: the update itself)
    update(1, 7, (1, 0, 0, 1))                                             # ... and the next update is a full fit too
    update(1, 8, (0, 1, 1, 1))
    ssm.set_hyperparameters(lengthscale=0.7)
    assert _counts(fake) == (1, 0, 0, 1) and ssm.x_train.size(0) == 25
    update(1, 9, (0, 1, 1, 1))
    ssm._raw_noise = ssm._raw_noise + 0.1                                  # hyper-parameters moved behind the model's back
    update(1, 10, (1, 0, 0, 1))
    update(1, 11, (0, 1, 1, 1))
    ssm._y_train = ssm._y_train.clone()
    ssm._y_train[0, 0] += 1.0                                              # a dropped row differs: the tail is what counts
    all_y = all_y.clone()
    all_y[-25, 0] += 1.0
    update(1, 12, (0, 1, 1, 1))
    ssm._y_train = ssm._y_train.clone()
    ssm._y_train[5, 0] += 1.0                                              # a kept row is not the fitted one
    all_y = all_y.clone()
    all_y[-20, 0] += 1.0
    update(1, 13, (1, 0, 0, 1))
    ssm._linv_current = False
    update(1, 14, (1, 0, 0, 1))
    ssm.mll_and_grad(ssm.x_train, ssm.y_train)                             # reuses the fit workspace: the factor is gone
    assert _counts(fake)[0] == 1
    update(1, 15, (1, 0, 0, 1))
    update(1, 16, (0, 1, 1, 1))


def test_limits_of_a_slide(fake, monkeypatch):
    assert gp_ssm_cem.MAX_SLIDE_ROWS == 16 <= gp_ssm_cem.MAX_DROP_ROWS == 64
    ssm = _fitted(fake, n=100, window=100)
    ssm.update_model(*_rows(17, seed=1))                                   # r = 17: past the measured break-even
    assert _counts(fake) == (1, 0, 0, 1) and ssm.x_train.size(0) == 100
    ssm.update_model(*_rows(16, seed=2))
    assert _counts(fake) == (0, 1, 1, 1)
    small = _fitted(fake, n=10, window=80, cem_gp_window_max_chain=None)
    small.update_model(*_rows(64, seed=3))                                 # 74 rows, below the window
    assert _counts(fake) == (0, 0, 1, 1)
    small.update_model(*_rows(22, seed=4))                                 # k = 22 appended, r = 16 of N = 74 dropped
    assert _counts(fake) == (0, 1, 1, 1) and small.x_train.size(0) == 80
    assert fake.args['sx_gp_drop'][:3] == (2, 74, 16) and fake.args['sx_gp_append'][1] == 58
    small.update_model(*_rows(65, seed=5))                                 # k = 65
    assert _counts(fake) == (1, 0, 0, 1)
    monkeypatch.setattr(gp_ssm_cem, 'MAX_SLIDE_ROWS', 64)                  # the entry itself takes 64
    wide = _fitted(fake, n=100, window=100)
    wide.update_model(*_rows(64, seed=6))
    assert _counts(fake) == (0, 1, 1, 1) and fake.args['sx_gp_drop'][:3] == (2, 100, 64)
    wide.update_model(*_rows(65, seed=7))
    assert _counts(fake) == (1, 0, 0, 1)


@pytest.mark.parametrize('which', ['sx_gp_drop', 'sx_gp_append'])
def test_not_pd_from_either_call_falls_back_and_packs_nothing_from_the_unspecified_outputs(fake, which):
    ssm = _fitted(fake)
    before = ssm.device_model
    fake.status[which] = _lib.SX_STATUS_NOT_PD
    x, y = _rows(1, seed=1)
    want_x = torch.cat((ssm.x_train, x))[-25:]
    ssm.update_model(x, y)
    assert _counts(fake) == (1, 1, 1, 1)                                   # the fallback fit's pack alone
    assert ssm.device_model is not before and ssm._appended == 0 and torch.equal(ssm._buffers[0], want_x)


def test_window_chain_bounds_the_rows_between_full_fits(fake):
    ssm = _fitted(fake, n=23, cem_gp_window_max_chain=4)
    seen = []
    for seed in range(1, 11):
        ssm.update_model(*_rows(1, seed=seed))
        seen.append(_counts(fake))
    # two appends below the window and two slides, a full fit, four slides, a full fit
    assert seen == [(0, 0, 1, 1)] * 2 + [(0, 1, 1, 1)] * 2 + [(1, 0, 0, 1)] + [(0, 1, 1, 1)] * 4 + [(1, 0, 0, 1)]
    ssm.update_model(*_rows(5, seed=20))                                   # more than the chain allows at once
    assert _counts(fake) == (1, 0, 0, 1)
    free = _fitted(fake, cem_gp_window_max_chain=None)
    for seed in range(1, 2 * gp_ssm_cem.WINDOW_MAX_CHAIN):
        free.update_model(*_rows(1, seed=seed))
    assert _counts(fake)[0] == 0
    unwindowed = GpCemSSM(Conf(window=None, cem_gp_window_max_chain=1), 2, 1)   # the bound is the windowed model's alone
    unwindowed.update_model(*_rows(20))
    for seed in range(1, 4):
        unwindowed.update_model(*_rows(1, seed=seed))
    assert _counts(fake) == (1, 0, 3, 4)


@pytest.mark.parametrize('incremental', [True, False, None])
def test_setting_off_calls_neither_new_entry(fake, incremental):
    ssm = GpCemSSM(Conf(window=None, incremental=incremental), 2, 1)
    for seed, n in enumerate((20, 1, 5, 1)):
        ssm.update_model(*_rows(n, seed=seed))
    assert fake.calls['sx_gp_drop'] == 0 and fake.calls['sx_gp_drop_workspace_bytes'] == 0
    assert ssm.x_train.size(0) == 27
    assert _counts(fake)[0] == (1 if incremental else 4)


def test_update_models_multi_handles_windowed_models_one_by_one(fake, monkeypatch):
    real_empty = torch.empty     # (the lockstep fit's problem table sits in pinned memory, which needs a device)
    monkeypatch.setattr(torch, 'empty', lambda *a, pin_memory=False, **kw: real_empty(*a, **kw))
    ssms = [GpCemSSM(Conf(), 2, 1), GpCemSSM(Conf(window=None), 2, 1), GpCemSSM(Conf(window=None, incremental=False), 2, 1),
            GpCemSSM(Conf(window=30), 2, 1)]
    for e, m in enumerate(ssms):
        m.update_model(*_rows(25 + e, seed=e))
    fake.calls.clear()
    new = [_rows(2, seed=10 + e) for e in range(4)]
    update_models_multi(ssms, [x for x, _ in new], [y for _, y in new])
    # model 0 slides, model 1 appends, model 2 is fitted (through the multi fit), model 3 appends below its window
    assert fake.calls['sx_gp_drop'] == 1 and fake.calls['sx_gp_append'] == 3 and fake.calls['sx_gp_fit'] == 0
    assert fake.calls['sx_gp_fit_multi'] == 1 and fake.calls['sx_gp_pack'] == 4
    assert [m.device_model.n_train for m in ssms] == [25, 28, 29, 30]
    fake.calls.clear()
    update_models_multi(ssms, [x for x, _ in new], [y for _, y in new], replace_old=True)
    assert fake.calls['sx_gp_drop'] == 0 and fake.calls['sx_gp_append'] == 0
    assert [m.x_train.size(0) for m in ssms] == [2, 2, 2, 2]
