"""CPU: the single-model entries of the exact-GP warm path (sx_gp_pack_sizes, sx_gp_fit, sx_gp_mll_grad, sx_gp_pack,
sx_gp_predict_var_jac, sx_gp_predict_mean_hessian), host side -- the code each one answers a bad argument with, and which
model shapes each accepts: fit, pack and pack_sizes take the wide n_u (n_s + n_u <= SX_MAX_D, the kept-column model of a
junk-dimension rollout), mll_grad, var_jac and mean_hessian keep n_u <= SX_MAX_NU.  Every case returns before the entry's
first HIP call, so none of them needs a GPU; the pointers are non-null placeholders that nothing dereferences."""
import ctypes

import pytest

from safe_exploration_amd import _lib

ARG, UNSUPPORTED, OK = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED, _lib.SX_OK
_P = ctypes.c_void_p(16)


def _model(n_s=2, n_u=1, n_train=10):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train, m.n_pad = n_s, n_u, n_train, 0
    m.x_train, m.a_pack, m.stage_tab = 16, 16, 16
    return m


# the shapes every entry refuses, and the wide one (n_s = 1, n_u = 5) that only fit / pack / pack_sizes take
BAD_SHAPES = [dict(n_s=0), dict(n_s=5), dict(n_u=0), dict(n_train=0), dict(n_s=2, n_u=5), dict(n_s=-1), dict(n_u=-1),
              dict(n_train=-3)]
WIDE = dict(n_s=1, n_u=5)


def _entry(name, n_buffers):
    """call(model, nulls=(), **kw): the entry with `n_buffers` placeholder pointers, those in `nulls` (indices) NULL."""
    fn = getattr(_lib.lib(), name)

    def call(model, nulls=()):
        bufs = [None if i in nulls else _P for i in range(n_buffers)]
        return fn(ctypes.byref(model) if model is not None else None, *bufs, None)

    return call


def test_pack_sizes_shapes():
    fn = _lib.lib().sx_gp_pack_sizes
    a, t = ctypes.c_int64(-1), ctypes.c_int64(-1)
    for bad in BAD_SHAPES:
        kw = dict(dict(n_s=2, n_u=1, n_train=10), **bad)
        assert fn(kw['n_s'], kw['n_u'], kw['n_train'], ctypes.byref(a), ctypes.byref(t)) == ARG, bad
        assert (a.value, t.value) == (-1, -1)                              # a refusal writes nothing
    assert fn(2, 1, 10, ctypes.byref(a), ctypes.byref(t)) == OK and a.value > 0 and t.value > 0
    assert fn(1, 5, 10, ctypes.byref(a), ctypes.byref(t)) == OK            # the wide shape
    assert fn(4, 2, 10, None, None) == OK                                  # either output may be NULL


def test_fit_answers_before_any_launch():
    call = _entry('sx_gp_fit', 6)                                          # y, work, linv, alpha, logdet, status
    big = 4097                                                             # beyond the fit's N: refused after the checks
    assert call(None) == ARG
    for i in range(6):
        assert call(_model(n_train=big), nulls=(i,)) == ARG, i             # a null buffer answers before the size
    no_x = _model(n_train=big)
    no_x.x_train = None
    assert call(no_x) == ARG
    for bad in BAD_SHAPES:
        assert call(_model(**dict(dict(n_train=big), **bad))) == ARG, bad  # and so does a bad shape
    assert call(_model(n_train=big)) == UNSUPPORTED
    assert call(_model(n_train=big, **WIDE)) == UNSUPPORTED                # the wide shape is accepted: only N refuses it
    assert call(_model(n_s=4, n_u=2, n_train=big)) == UNSUPPORTED


def test_mll_grad_answers_before_any_launch():
    call = _entry('sx_gp_mll_grad', 7)                                     # y, linv, alpha, logdet, work, mll, grad
    assert call(None) == ARG
    for i in range(7):
        assert call(_model(), nulls=(i,)) == ARG, i
    no_x = _model()
    no_x.x_train = None
    assert call(no_x) == ARG
    for bad in BAD_SHAPES:
        assert call(_model(**bad)) == ARG, bad
    assert call(_model(**WIDE)) == ARG                                     # n_u <= SX_MAX_NU here
    assert call(_model(n_s=2, n_u=3)) == ARG


def test_pack_answers_before_any_launch():
    call = _entry('sx_gp_pack', 2)                                         # linv, alpha
    assert call(None) == ARG
    for i in range(2):
        assert call(_model(), nulls=(i,)) == ARG, i
    for field in ('x_train', 'a_pack', 'stage_tab'):
        m = _model()
        setattr(m, field, None)
        assert call(m) == ARG, field
    for bad in BAD_SHAPES:
        m = _model(**bad)
        assert call(m) == ARG, bad
        assert m.n_pad == 0                                                # a refused model is left as it was


@pytest.mark.parametrize('name', ['sx_gp_predict_var_jac', 'sx_gp_predict_mean_hessian'])
def test_query_derivatives_answer_before_any_launch(name):
    fn = getattr(_lib.lib(), name)

    def call(model, P=4, second=_P, z=_P, out=_P):                         # second: linv (var_jac) / alpha (mean_hessian)
        return fn(ctypes.byref(model) if model is not None else None, second, z, P, out, None)

    assert call(None) == ARG
    assert call(None, P=0) == ARG
    assert call(_model(), P=-1) == ARG
    assert call(_model(), P=0) == OK                                       # an empty batch is not an error ...
    assert call(_model(), P=0, second=None, z=None, out=None) == OK        # ... its pointers may be NULL ...
    assert call(_model(n_s=5), P=0) == OK                                  # ... and its shape is not looked at
    assert call(_model(), second=None) == ARG
    assert call(_model(), z=None) == ARG
    assert call(_model(), out=None) == ARG
    no_x = _model()
    no_x.x_train = None
    assert call(no_x) == ARG
    for bad in BAD_SHAPES:
        assert call(_model(**bad)) == ARG, bad
    assert call(_model(**WIDE)) == ARG                                     # n_u <= SX_MAX_NU here
    assert call(_model(n_s=2, n_u=3)) == ARG
    if name == 'sx_gp_predict_var_jac':
        assert call(_model(n_train=8193)) == UNSUPPORTED                   # 2 N doubles of LDS: N <= 8192
        assert call(_model(n_train=8193), z=None) == ARG                   # argument errors answer first
        assert call(_model(n_train=8193, **WIDE)) == ARG
