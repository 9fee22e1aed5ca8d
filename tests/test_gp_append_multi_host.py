"""CPU: the lockstep append (sx_gp_append_table / sx_gp_append_multi, conf.cem_gp_incremental_lockstep), host side.  The
declarations of _lib.py against include/sx_amd.h; the codes the two entries answer bad arguments with, before any device
access (the device pointers are placeholders nothing dereferences); and, with a counting fake in place of the library,
which calls update_models_multi makes with the setting off and on, how it groups the models, what a problem that is not
positive definite costs, and that the number of device-to-host reads of a lockstep update does not grow with the models."""
import collections
import ctypes
import os
import re

import pytest
import torch

from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM, update_models_multi

ARG, UNSUPPORTED, OK = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED, _lib.SX_OK
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sx_amd.h')
NAMES = ('sx_gp_append_table_bytes', 'sx_gp_append_table', 'sx_gp_append_multi')


# ---- declarations ----------------------------------------------------------------------------------------------------------

def _ctype(decl):
    decl = decl.strip()
    if 'sx_gp_model' in decl:
        return ctypes.POINTER(_lib.SxGpModel)
    if decl.count('*') == 2:
        return ctypes.POINTER(ctypes.c_void_p)
    if '*' in decl:
        return ctypes.POINTER(ctypes.c_int64) if 'int64_t' in decl else ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[decl.rsplit(' ', 1)[0].strip()]


@pytest.mark.parametrize('name', NAMES)
def test_symbols_are_exported_and_declared_as_the_header_declares_them(name):
    assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ret, args = re.search(r'(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', text).groups()
    res, argtypes = _lib.SIGNATURES[name]
    assert res is {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[ret]
    assert argtypes == [_ctype(a) for a in args.split(',')]
    assert getattr(_lib.lib(), name).argtypes == argtypes


def test_entry_size_is_the_header_s():
    text = open(HEADER).read()
    size = int(re.search(r'#define\s+SX_GP_APPEND_ENTRY_BYTES\s+(\d+)', text).group(1))
    assert size == _lib.SX_GP_APPEND_ENTRY_BYTES and size % 8 == 0
    fn = _lib.lib().sx_gp_append_table_bytes
    assert fn(0) < 0 and fn(-1) < 0
    assert [fn(E) for E in (1, 2, 6, 1000)] == [E * size for E in (1, 2, 6, 1000)]


# ---- argument errors, without a device -------------------------------------------------------------------------------------

def _models(n_trains=(11, 21), n_s=2, n_u=1):
    arr = (_lib.SxGpModel * len(n_trains))()
    for m, n in zip(arr, n_trains):
        m.n_s, m.n_u, m.n_train, m.n_pad = n_s, n_u, n, 0
        m.x_train = 16
    return arr


def _table(models, E=None, k=1, null_array=None, null_element=None, ws_bytes=None, no_status=False, no_table=False):
    """sx_gp_append_table with placeholder device pointers and a real host table"""
    lib = _lib.lib()
    n = len(models) if models is not None else 2
    E = n if E is None else E
    arrays = []
    for i in range(8):        # y, linv_old, alpha_old, logdet_old, linv, alpha, logdet, workspace
        a = (ctypes.c_void_p * n)(*([16] * n))
        if null_element == i:
            a[n - 1] = None
        arrays.append(None if null_array == i else a)
    sizes = (ctypes.c_int64 * n)(*(ws_bytes if ws_bytes is not None else [1 << 40] * n))
    table = ctypes.create_string_buffer(max(n, 1) * _lib.SX_GP_APPEND_ENTRY_BYTES)
    return lib.sx_gp_append_table(models, E, k, *arrays[:7], None if no_status else ctypes.c_void_p(16), arrays[7],
                                  None if null_array == 8 else sizes, None if no_table else table)


def test_table_answers_before_any_device_access():
    assert _table(_models()) == OK
    assert _table(None) == ARG
    for i in range(9):
        assert _table(_models(), null_array=i) == ARG, i
    for i in range(8):
        assert _table(_models(), null_element=i) == ARG, i
    assert _table(_models(), no_status=True) == ARG and _table(_models(), no_table=True) == ARG
    assert _table(_models(), E=0) == ARG and _table(_models(), E=-2) == ARG
    for k in (0, -1, 65):
        assert _table(_models((100, 120)), k=k) == ARG, k
    assert _table(_models((100, 120)), k=64) == OK
    mixed = _models()
    mixed[1].n_u = 2
    assert _table(mixed) == ARG
    mixed = _models()
    mixed[1].n_s = 1
    assert _table(mixed) == ARG
    for bad in (dict(n_s=0), dict(n_s=5), dict(n_u=0), dict(n_s=2, n_u=5)):
        assert _table(_models(**bad)) == ARG, bad
    assert _table(_models(n_s=1, n_u=5)) == OK                              # the wide shape is accepted
    assert _table(_models((11, 0))) == ARG and _table(_models((11, -3))) == ARG
    assert _table(_models((11, 1))) == ARG                                  # N_e = 0
    assert _table(_models((11, 5)), k=5) == ARG
    no_x = _models()
    no_x[1].x_train = None
    assert _table(no_x) == ARG
    need = [int(_lib.lib().sx_gp_append_workspace_bytes(2, n, 1)) for n in (11, 21)]
    assert min(need) > 0
    assert _table(_models(), ws_bytes=need) == OK
    assert _table(_models(), ws_bytes=[need[0], need[1] - 1]) == ARG
    assert _table(_models(), ws_bytes=[0, need[1]]) == ARG
    assert _table(_models((11, 4097))) == UNSUPPORTED
    assert _table(_models((4096, 4097)), k=64) == UNSUPPORTED
    assert _table(_models((4096, 4096)), k=64) == OK
    assert _table(_models((11, 4097)), null_array=3) == ARG                 # argument errors answer first
    assert _table(_models((11, 4097)), ws_bytes=[1 << 40, 8]) == ARG
    many = 65535 // 2 + 1                                                   # E n_s = 65536
    assert _table(_models((11,) * many)) == UNSUPPORTED
    assert _table(_models((11,) * (many - 1))) == OK


def test_multi_answers_before_any_device_access():
    """(only refusals: a call that is accepted launches)"""
    fn = _lib.lib().sx_gp_append_multi
    P = ctypes.c_void_p(16)
    assert fn(None, 2, 1, P, None) == ARG
    assert fn(_models(), 2, 1, None, None) == ARG
    assert fn(_models(), 0, 1, P, None) == ARG
    for k in (0, 65):
        assert fn(_models((100, 120)), 2, k, P, None) == ARG
    mixed = _models()
    mixed[1].n_u = 2
    assert fn(mixed, 2, 1, P, None) == ARG
    assert fn(_models(n_s=5), 2, 1, P, None) == ARG
    assert fn(_models((11, 1)), 2, 1, P, None) == ARG
    no_x = _models()
    no_x[0].x_train = None
    assert fn(no_x, 2, 1, P, None) == ARG
    assert fn(_models((11, 4097)), 2, 1, P, None) == UNSUPPORTED
    many = 65535 // 2 + 1
    assert fn(_models((11,) * many), many, 1, P, None) == UNSUPPORTED
    assert fn(_models((11, 4097)), 2, 1, None, None) == ARG


# ---- which calls update_models_multi makes, with a counting fake in place of the library ------------------------------------

class FakeLib:
    """Every entry counted; the host-only size queries answer for real, every other entry answers SX_OK and touches
    nothing -- but for the status words (host tensors here): sx_gp_append or-s `append_status` into its word, and
    sx_gp_append_multi `multi_status[e]` into word e of the status sx_gp_append_table was given."""
    HOST_ONLY = ('_bytes', '_sizes')

    def __init__(self, lib):
        self._lib, self.calls, self.append_status, self.multi_status = lib, collections.Counter(), 0, {}
        self.groups, self._status = [], None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            if name.endswith(self.HOST_ONLY):
                return fn(*args)
            if name == 'sx_gp_append':
                ctypes.cast(args[9], ctypes.POINTER(ctypes.c_int32))[0] |= self.append_status
            if name == 'sx_gp_append_table':
                self._status = ctypes.cast(args[10], ctypes.POINTER(ctypes.c_int32))
            if name == 'sx_gp_append_multi':
                E, k = args[1], args[2]
                self.groups.append((k, [args[0][e].n_train for e in range(E)]))
                for e in range(E):
                    self._status[e] |= self.multi_status.get(e, 0)
            return OK
        return counted


class Conf:
    device = 'cpu'
    exact_gp_kernel = 'rbf'
    exact_gp_training_iterations = 0

    def __init__(self, incremental=True, lockstep=True, **kw):
        self.cem_gp_incremental, self.cem_gp_incremental_lockstep = incremental, lockstep
        for key, v in kw.items():
            setattr(self, key, v)


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: lib)
    monkeypatch.setattr(_lib, 'require_gpu', lambda *a: None)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda dev: None)
    real_empty = torch.empty     # (the problem tables sit in pinned memory, which needs a device)
    monkeypatch.setattr(torch, 'empty', lambda *a, pin_memory=False, **kw: real_empty(*a, **kw))
    return lib


def _rows(n, seed=0, n_s=2, n_u=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, n_s + n_u), dtype=torch.float64, generator=g),
            torch.rand((n, n_s), dtype=torch.float64, generator=g))


def _fitted(fake, confs, n0=20):
    ssms = [GpCemSSM(c, 2, 1) for c in confs]
    for e, m in enumerate(ssms):
        m.update_model(*_rows(n0 + e, seed=e))
    assert fake.calls['sx_gp_fit'] == len(ssms)
    fake.calls.clear()
    return ssms


def _update(ssms, ks, seed=10):
    new = [_rows(k, seed=seed + e) for e, k in enumerate(ks)]
    update_models_multi(ssms, [x for x, _ in new], [y for _, y in new])


def _counts(fake):
    got = tuple(fake.calls[n] for n in ('sx_gp_fit', 'sx_gp_fit_multi', 'sx_gp_append', 'sx_gp_append_multi', 'sx_gp_pack'))
    fake.calls.clear()
    return got


def test_setting_needs_the_incremental_one():
    with pytest.raises(ValueError, match='cem_gp_incremental'):
        GpCemSSM(Conf(incremental=False), 2, 1)
    assert GpCemSSM(Conf(), 2, 1)._lockstep is True
    assert GpCemSSM(Conf(lockstep=False), 2, 1)._lockstep is False

    class Bare:
        device, exact_gp_kernel, exact_gp_training_iterations, cem_gp_incremental = 'cpu', 'rbf', 0, True
    assert GpCemSSM(Bare(), 2, 1)._lockstep is False                        # the default: off


@pytest.mark.parametrize('E', [2, 4])
def test_setting_off_appends_model_by_model(fake, E):
    ssms = _fitted(fake, [Conf(lockstep=False)] * E)
    _update(ssms, [1] * E)
    assert fake.calls['sx_gp_append_table'] == 0
    assert _counts(fake) == (0, 0, E, 0, E)
    assert [m._appended for m in ssms] == [1] * E


@pytest.mark.parametrize('E', [2, 4])
def test_setting_on_appends_in_one_call(fake, E):
    ssms = _fitted(fake, [Conf()] * E)
    before = [m.device_model for m in ssms]
    _update(ssms, [1] * E)
    assert fake.calls['sx_gp_append_table'] == 1
    assert _counts(fake) == (0, 0, 0, 1, E)
    assert fake.groups == [(1, [21 + e for e in range(E)])]
    for e, (m, b) in enumerate(zip(ssms, before)):
        n = 21 + e
        assert m.device_model is not b and m.device_model.n_train == n and m.x_train.size(0) == n
        assert m._fit_ws[0].shape == (2, 0, 0) and m._fit_ws[1].shape == (2, n, n) and m._alpha.shape == (2, n)
        assert m._appended == 1 and m._append_ok and m._linv_current
        assert m._fit_state[0].shape == (n, 2) and m._fit_state[1].shape == (2,)
    # ... and again, to the buffers the lockstep call left; the group's workspace and tables are kept
    kept = ssms[0]._lockstep_bufs
    ws = kept.ws
    _update(ssms, [3] * E, seed=30)
    assert _counts(fake) == (0, 0, 0, 1, E) and [m._appended for m in ssms] == [4] * E
    assert ssms[0]._lockstep_bufs is kept and kept.ws is ws


def test_groups_share_the_number_of_new_rows(fake):
    ssms = _fitted(fake, [Conf()] * 3)
    _update(ssms, [1, 1, 2])
    assert _counts(fake) == (0, 0, 1, 1, 3)
    assert fake.groups == [(1, [21, 22])]
    assert [m.device_model.n_train for m in ssms] == [21, 22, 24] and [m._appended for m in ssms] == [1, 1, 2]


def test_models_without_the_setting_append_alone(fake):
    ssms = _fitted(fake, [Conf(), Conf(lockstep=False), Conf(), Conf(lockstep=False)])
    _update(ssms, [2] * 4)
    assert _counts(fake) == (0, 0, 2, 1, 4)
    assert fake.groups == [(2, [22, 24])]
    assert [m._appended for m in ssms] == [2] * 4


def test_model_that_does_not_qualify_is_fitted_beside_the_group(fake):
    ssms = _fitted(fake, [Conf()] * 4)
    ssms[2].set_hyperparameters(noise=0.2)
    ssms[2]._append_ok = False                                             # model 2 does not qualify ...
    ssms[3]._y_train = ssms[3]._y_train.clone()
    ssms[3]._y_train[3, 0] += 1.0                                          # ... nor 3: its stored targets are not the fitted ones
    fake.calls.clear()
    _update(ssms, [2] * 4)
    assert _counts(fake) == (0, 1, 0, 1, 4)
    assert fake.groups == [(2, [22, 23])]
    assert [m.device_model.n_train for m in ssms] == [22, 23, 24, 25]
    assert [m._appended for m in ssms] == [2, 2, 0, 0]


def test_not_pd_problem_is_fitted_in_full_alone_and_the_others_are_installed(fake):
    ssms = _fitted(fake, [Conf()] * 3)
    fake.multi_status = {1: _lib.SX_STATUS_NOT_PD}
    _update(ssms, [1] * 3)
    assert _counts(fake) == (1, 0, 0, 1, 3)                                # one full fit; its pack and the two installs'
    assert [m.device_model.n_train for m in ssms] == [21, 22, 23]
    assert [m._appended for m in ssms] == [1, 0, 1]
    assert ssms[1]._fit_ws[0].shape == (2, 22, 22) and ssms[0]._fit_ws[0].shape == (2, 0, 0)
    fake.multi_status = {}
    _update(ssms, [1] * 3, seed=40)
    assert _counts(fake) == (0, 0, 0, 1, 3) and [m._appended for m in ssms] == [2, 1, 2]


def test_max_chain_is_respected(fake):
    ssms = _fitted(fake, [Conf(cem_gp_incremental_max_chain=2), Conf(), Conf()])
    seen = []
    for step in range(4):
        _update(ssms, [1] * 3, seed=50 + 10 * step)
        seen.append(_counts(fake))
    # the third update would be model 0's third appended row: it is fitted in full (alone: the lockstep fit of one model)
    assert seen == [(0, 0, 0, 1, 3), (0, 0, 0, 1, 3), (0, 1, 0, 1, 3), (0, 0, 0, 1, 3)]
    assert fake.groups[2] == (1, [24, 25]) and [m._appended for m in ssms] == [1, 4, 4]


def test_group_of_one_appends_as_the_single_model_does(fake):
    ssms = _fitted(fake, [Conf()] * 2)
    ssms[1]._append_ok = False
    _update(ssms, [1, 1])
    assert _counts(fake) == (0, 1, 1, 0, 2) and fake.calls['sx_gp_append_table'] == 0


# ---- host waits ---------------------------------------------------------------------------------------------------------------

def _reads(monkeypatch, fake, E, lockstep):
    """the device-to-host reads of one update that appends a row to each of E models, by kind"""
    ssms = _fitted(fake, [Conf(lockstep=lockstep)] * E)
    seen = collections.Counter()
    real = dict(cpu=torch.Tensor.cpu, item=torch.Tensor.item, equal=torch.equal)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, 'cpu', lambda self, *a, **kw: (seen.update(['cpu']), real['cpu'](self, *a, **kw))[1])
        mp.setattr(torch.Tensor, 'item', lambda self: (seen.update(['item']), real['item'](self))[1])
        mp.setattr(torch, 'equal', lambda a, b: (seen.update(['equal']), real['equal'](a, b))[1])
        _update(ssms, [1] * E)
    assert _counts(fake) == ((0, 0, 0, 1, E) if lockstep else (0, 0, E, 0, E))
    return dict(seen)


def test_reads_do_not_grow_with_the_models(monkeypatch, fake):
    """One read for the decision (every model's comparison of its fitted rows, in one tensor) and one for the results
    (status [E] and logdet [E x n_s] in one copy); model by model each model reads four times: two comparisons, the
    status and the log-determinant."""
    assert _reads(monkeypatch, fake, 2, True) == _reads(monkeypatch, fake, 4, True) == {'cpu': 2}
    for E in (2, 4):
        assert _reads(monkeypatch, fake, E, False) == {'equal': 2 * E, 'item': E, 'cpu': E}
