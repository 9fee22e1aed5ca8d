"""CPU: the lockstep drop (sx_gp_drop_table / sx_gp_drop_multi) and the lockstep slide of windowed models
(conf.cem_gp_window with conf.cem_gp_incremental_lockstep), host side.  The declarations of _lib.py against include/sx_amd.h;
the codes the two entries answer bad arguments with, before any device access (the device pointers are placeholders nothing
dereferences); and, with a counting fake in place of the library, which calls update_models_multi makes for windowed models
with the setting on, how it groups them, what a problem that is not positive definite costs, and that the number of
device-to-host reads of a lockstep slide does not grow with the models."""
import collections
import ctypes
import os
import re

import pytest
import torch

from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem import gp_ssm_cem
from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM, update_models_multi

ARG, UNSUPPORTED, OK = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED, _lib.SX_OK
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sx_amd.h')
NAMES = ('sx_gp_drop_table_bytes', 'sx_gp_drop_table', 'sx_gp_drop_multi')
NOT_PD = _lib.SX_STATUS_NOT_PD


# ---- declarations ----------------------------------------------------------------------------------------------------------

def _ctype(decl):
    decl = decl.strip()
    if decl.count('*') == 2:
        return ctypes.POINTER(ctypes.c_void_p)
    if '*' in decl:
        if 'int64_t' in decl:
            return ctypes.POINTER(ctypes.c_int64)
        return ctypes.POINTER(ctypes.c_int) if re.match(r'const\s+int\s*\*', decl) else ctypes.c_void_p
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
    """(sx_gp_drop_table_bytes answers with the compiled sizeof(DropEntry), which a static_assert ties to the header's)"""
    text = open(HEADER).read()
    size = int(re.search(r'#define\s+SX_GP_DROP_ENTRY_BYTES\s+(\d+)', text).group(1))
    assert size == _lib.SX_GP_DROP_ENTRY_BYTES and size % 8 == 0
    fn = _lib.lib().sx_gp_drop_table_bytes
    assert fn(0) < 0 and fn(-1) < 0
    assert [fn(E) for E in (1, 2, 6, 1000)] == [E * size for E in (1, 2, 6, 1000)]


# ---- argument errors, without a device -------------------------------------------------------------------------------------

def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def _table(n_old=(11, 21), n_s=2, E=None, k=1, null_array=None, null_element=None, ws_bytes=None, no_status=False,
           no_table=False, no_n_old=False):
    """sx_gp_drop_table with placeholder device pointers and a real host table"""
    lib = _lib.lib()
    n = len(n_old)
    E = n if E is None else E
    arrays = []
    for i in range(6):        # y, linv_old, linv, alpha, logdet, workspace
        a = (ctypes.c_void_p * n)(*([16] * n))
        if null_element == i:
            a[n - 1] = None
        arrays.append(None if null_array == i else a)
    sizes = (ctypes.c_int64 * n)(*(ws_bytes if ws_bytes is not None else [1 << 40] * n))
    table = ctypes.create_string_buffer(max(n, 1) * _lib.SX_GP_DROP_ENTRY_BYTES)
    return lib.sx_gp_drop_table(n_s, E, k, None if no_n_old else _ints(n_old), *arrays[:5],
                                None if no_status else ctypes.c_void_p(16), arrays[5], None if null_array == 6 else sizes,
                                None if no_table else table)


def test_table_answers_before_any_device_access():
    assert _table() == OK
    assert _table(no_table=True) == ARG and _table(no_status=True) == ARG and _table(no_n_old=True) == ARG
    for i in range(7):
        assert _table(null_array=i) == ARG, i
    for i in range(6):
        assert _table(null_element=i) == ARG, i
    assert _table(E=0) == ARG and _table(E=-2) == ARG
    for k in (0, -1, 65):
        assert _table((100, 120), k=k) == ARG, k
    assert _table((100, 120), k=64) == OK
    for n_s in (0, -1, 5):
        assert _table(n_s=n_s) == ARG, n_s
    assert _table((11, 1)) == ARG and _table((11, 0)) == ARG and _table((11, -3)) == ARG      # n_old[e] = k, and below
    assert _table((11, 5), k=5) == ARG and _table((11, 5), k=6) == ARG
    assert _table((11, 6), k=5) == OK                                                         # m = 1
    need = [int(_lib.lib().sx_gp_drop_workspace_bytes(2, n, 1)) for n in (11, 21)]
    assert min(need) > 0
    assert _table(ws_bytes=need) == OK
    assert _table(ws_bytes=[need[0], need[1] - 1]) == ARG
    assert _table(ws_bytes=[need[0] - 1, need[1]]) == ARG and _table(ws_bytes=[0, need[1]]) == ARG
    assert _table((11, 4097)) == UNSUPPORTED
    assert _table((4096, 4097), k=64) == UNSUPPORTED
    assert _table((4096, 4096), k=64) == OK
    assert _table((11, 4097), null_array=2) == ARG                          # argument errors answer first
    assert _table((11, 4097), null_element=4) == ARG
    assert _table((11, 4097), ws_bytes=[1 << 40, 8]) == ARG
    assert _table((11, 4097), k=65) == ARG
    many = 65535 // 2 + 1                                                   # E n_s = 65536
    assert _table((11,) * many) == UNSUPPORTED
    assert _table((11,) * (many - 1)) == OK
    assert _table((11,) * 65536, n_s=1) == UNSUPPORTED and _table((11,) * 65535, n_s=1) == OK


def test_table_writes_the_problems_extents():
    """the entry ends in the problem's own grid extents: 64-row blocks and 4-row blocks of its m kept rows"""
    lib = _lib.lib()
    n_old, k = (66, 130, 346), 37
    table = ctypes.create_string_buffer(3 * _lib.SX_GP_DROP_ENTRY_BYTES)
    ptrs = lambda: (ctypes.c_void_p * 3)(16, 16, 16)
    assert lib.sx_gp_drop_table(2, 3, k, _ints(n_old), ptrs(), ptrs(), ptrs(), ptrs(), ptrs(), ctypes.c_void_p(4096), ptrs(),
                                (ctypes.c_int64 * 3)(*[1 << 40] * 3), table) == OK
    for e, n in enumerate(n_old):
        entry = table.raw[e * _lib.SX_GP_DROP_ENTRY_BYTES:(e + 1) * _lib.SX_GP_DROP_ENTRY_BYTES]
        words = [int.from_bytes(entry[at:at + 4], 'little', signed=True) for at in range(80, 104, 4)]
        m = n - k
        assert words == [n, k, m, 2, (m + 63) // 64, (m + 3) // 4]
        assert int.from_bytes(entry[40:48], 'little') == 4096 + 4 * e       # the problem's own status word


def test_multi_answers_before_any_device_access():
    """(only refusals: a call that is accepted launches)"""
    fn = _lib.lib().sx_gp_drop_multi
    P = ctypes.c_void_p(16)
    assert fn(2, 2, 1, _ints((11, 21)), None, None) == ARG
    assert fn(2, 2, 1, None, P, None) == ARG
    assert fn(2, 0, 1, _ints((11, 21)), P, None) == ARG
    for k in (0, 65):
        assert fn(2, 2, k, _ints((100, 120)), P, None) == ARG
    for n_s in (0, 5):
        assert fn(n_s, 2, 1, _ints((11, 21)), P, None) == ARG
    assert fn(2, 2, 1, _ints((11, 1)), P, None) == ARG
    assert fn(2, 2, 5, _ints((5, 11)), P, None) == ARG
    assert fn(2, 2, 1, _ints((11, 4097)), P, None) == UNSUPPORTED
    many = 65535 // 2 + 1
    assert fn(2, many, 1, _ints((11,) * many), P, None) == UNSUPPORTED
    assert fn(2, 2, 1, _ints((11, 4097)), None, None) == ARG
    assert fn(2, 2, 65, _ints((11, 4097)), P, None) == ARG


# ---- which calls update_models_multi makes, with a counting fake in place of the library ------------------------------------

class FakeLib:
    """Every entry counted; the host-only size queries answer for real, every other entry answers SX_OK and touches
    nothing -- but for the status words (host tensors here): sx_gp_drop and sx_gp_append or `status[name]` into their word,
    and sx_gp_drop_multi / sx_gp_append_multi or `status[name][e]` into word e of the status their table call was given."""
    HOST_ONLY = ('_bytes', '_sizes')
    STATUS_ARG = {'sx_gp_drop': 8, 'sx_gp_append': 9}
    TABLE_STATUS_ARG = {'sx_gp_drop_table': 9, 'sx_gp_append_table': 10}

    def __init__(self, lib):
        self._lib, self.calls, self.status, self.log = lib, collections.Counter(), {}, []
        self._words = {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            if name.endswith(self.HOST_ONLY):
                return fn(*args)
            if name in self.STATUS_ARG:
                ctypes.cast(args[self.STATUS_ARG[name]], ctypes.POINTER(ctypes.c_int32))[0] |= self.status.get(name, 0)
            if name in self.TABLE_STATUS_ARG:
                at = args[self.TABLE_STATUS_ARG[name]]
                self._words[name.replace('_table', '_multi')] = (ctypes.cast(at, ctypes.POINTER(ctypes.c_int32)),
                                                                 ctypes.cast(at, ctypes.c_void_p).value)
            if name == 'sx_gp_drop_multi':
                n_s, E, k = args[:3]
                self.log.append(('drop', k, [args[3][e] for e in range(E)], self._words[name][1]))
            if name == 'sx_gp_append_multi':
                E, k = args[1], args[2]
                self.log.append(('append', k, [args[0][e].n_train for e in range(E)], self._words[name][1]))
            if name in ('sx_gp_drop_multi', 'sx_gp_append_multi'):
                for e, bits in self.status.get(name, {}).items():
                    self._words[name][0][e] |= bits
            return OK
        return counted


class Conf:
    device = 'cpu'
    exact_gp_kernel = 'rbf'
    exact_gp_training_iterations = 0
    cem_gp_incremental = True

    def __init__(self, window=25, lockstep=True, **kw):
        self.cem_gp_incremental_lockstep = lockstep
        if window is not None:
            self.cem_gp_window = window
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


class Models:
    """models fitted on n0[e] rows each, and the rows every one of them has been given so far"""

    def __init__(self, fake, confs, n0):
        self.fake, self.ssms, self.all = fake, [GpCemSSM(c, 2, 1) for c in confs], []
        for e, (m, n) in enumerate(zip(self.ssms, n0)):
            x, y = _rows(n, seed=e)
            m.update_model(x, y)
            self.all.append((x, y))
        assert fake.calls['sx_gp_fit'] == len(self.ssms)
        fake.calls.clear()

    def update(self, ks, seed=100, **kw):
        new = [_rows(k, seed=seed + e) for e, k in enumerate(ks)]
        update_models_multi(self.ssms, [x for x, _ in new], [y for _, y in new], **kw)
        for e, (x, y) in enumerate(new):
            self.all[e] = (x, y) if kw.get('replace_old') else (torch.cat((self.all[e][0], x)), torch.cat((self.all[e][1], y)))

    def fitted_on_the_last_rows(self):
        """every model's device rows and stored rows are exactly the last min(window, all) rows it was given"""
        for m, (x, y) in zip(self.ssms, self.all):
            w = m._window if m._window is not None else x.size(0)
            if not (torch.equal(m._buffers[0], x[-w:]) and torch.equal(m._fit_state[0], y[-w:])
                    and torch.equal(m.x_train, x[-w:]) and torch.equal(m.y_train, y[-w:])
                    and m.device_model.n_train == min(w, x.size(0)) and m._fit_ws[1].size(1) == m.device_model.n_train
                    and m._linv_current):
                return False
        return True

    def counts(self):
        got = tuple(self.fake.calls[n] for n in ('sx_gp_drop_multi', 'sx_gp_append_multi', 'sx_gp_drop', 'sx_gp_append',
                                                 'sx_gp_fit', 'sx_gp_fit_multi', 'sx_gp_pack'))
        self.fake.calls.clear()
        return got


WINDOWS = (25, 26, 40, 31)


def test_steady_state_is_one_drop_call_and_one_append_call(fake):
    """four windowed lockstep models with full windows get one row each"""
    ms = Models(fake, [Conf(w) for w in WINDOWS], WINDOWS)
    for step in range(3):
        ms.update([1] * 4, seed=100 + 10 * step)
        assert fake.calls['sx_gp_drop_table'] == 1 and fake.calls['sx_gp_append_table'] == 1
        assert ms.counts() == (1, 1, 0, 0, 0, 0, 4), step
        assert ms.fitted_on_the_last_rows()
        assert [m._appended for m in ms.ssms] == [step + 1] * 4 and all(m._append_ok for m in ms.ssms)
    # the drop of the fitted rows, then the append onto the kept ones, on the same status words
    (d, rd, n_old, words_d), (a, ka, n_train, words_a) = fake.log[:2]
    assert (d, rd, n_old) == ('drop', 1, list(WINDOWS)) and (a, ka, n_train) == ('append', 1, list(WINDOWS))
    assert words_d == words_a
    lead = ms.ssms[0]._lockstep_bufs
    assert lead.ws is not None and lead.drop.ws is not None and lead.drop.table is not lead.table
    assert all(m._lockstep_bufs is None for m in ms.ssms[1:])
    for m in ms.ssms:
        assert m._fit_ws[0].shape == (2, 0, 0) and m._alpha.shape == (2, m._window)


def test_groups_share_the_dropped_and_the_new_rows(fake):
    ms = Models(fake, [Conf(25), Conf(30), Conf(35)], (25, 30, 35))
    ms.update([1, 1, 3])                                                    # (r, k) = (1, 1), (1, 1), (3, 3)
    assert ms.counts() == (1, 1, 1, 1, 0, 0, 3)
    assert [(kind, k, ns) for kind, k, ns, _ in fake.log] == [('drop', 1, [25, 30]), ('append', 1, [25, 30])]
    assert ms.fitted_on_the_last_rows() and [m._appended for m in ms.ssms] == [1, 1, 3]
    # the same k with another r is another group: model 2 is two rows below its window
    ms2 = Models(fake, [Conf(25), Conf(25), Conf(27)], (25, 25, 25))
    fake.log.clear()
    ms2.update([3, 3, 3])                                                   # (3, 3), (3, 3), (1, 3)
    assert ms2.counts() == (1, 1, 1, 1, 0, 0, 3)
    assert [(kind, k, ns) for kind, k, ns, _ in fake.log] == [('drop', 3, [25, 25]), ('append', 3, [25, 25])]
    assert ms2.fitted_on_the_last_rows()


def test_below_its_window_a_windowed_model_appends_with_the_others(fake):
    ms = Models(fake, [Conf(30), Conf(None)], (25, 22))
    ms.update([2, 2])
    assert ms.counts() == (0, 1, 0, 0, 0, 0, 2)
    assert fake.log == [('append', 2, [27, 24], fake.log[0][3])]
    assert ms.fitted_on_the_last_rows()
    ms.update([3, 3], seed=200)                                             # exactly full: still an append
    assert ms.counts() == (0, 1, 0, 0, 0, 0, 2) and ms.ssms[0].x_train.size(0) == 30
    ms.update([1, 1], seed=300)                                             # model 0 slides alone, model 1 appends alone
    assert ms.counts() == (0, 0, 1, 2, 0, 0, 2)
    assert ms.fitted_on_the_last_rows() and ms.ssms[0].x_train.size(0) == 30 and ms.ssms[1].x_train.size(0) == 28


def test_model_without_the_setting_goes_alone(fake):
    ms = Models(fake, [Conf(25), Conf(25, lockstep=False), Conf(30), Conf(28)], (25, 25, 30, 28))
    ms.update([1] * 4)
    assert ms.counts() == (1, 1, 1, 1, 0, 0, 4)
    assert [(kind, k, ns) for kind, k, ns, _ in fake.log] == [('drop', 1, [25, 30, 28]), ('append', 1, [25, 30, 28])]
    assert ms.fitted_on_the_last_rows() and [m._appended for m in ms.ssms] == [1] * 4


def test_setting_off_everywhere_makes_no_multi_call(fake):
    ms = Models(fake, [Conf(25, lockstep=False)] * 3, (25,) * 3)
    ms.update([1] * 3)
    assert fake.calls['sx_gp_drop_table'] == 0 and fake.calls['sx_gp_drop_table_bytes'] == 0
    assert ms.counts() == (0, 0, 3, 3, 0, 0, 3) and ms.fitted_on_the_last_rows()


@pytest.mark.parametrize('which', ['sx_gp_drop_multi', 'sx_gp_append_multi'])
def test_not_pd_problem_is_fitted_on_its_last_rows_alone_and_the_others_are_installed(fake, which):
    ms = Models(fake, [Conf(25), Conf(30), Conf(35)], (25, 30, 35))
    before = [m.device_model for m in ms.ssms]
    fake.status[which] = {1: NOT_PD}
    ms.update([1] * 3)
    assert ms.counts() == (1, 1, 0, 0, 1, 0, 3)                             # one full fit; its pack and the two installs'
    assert ms.fitted_on_the_last_rows()
    assert [m._appended for m in ms.ssms] == [1, 0, 1]
    assert all(m.device_model is not b for m, b in zip(ms.ssms, before))
    assert ms.ssms[1]._fit_ws[0].shape == (2, 30, 30) and ms.ssms[0]._fit_ws[0].shape == (2, 0, 0)
    fake.status.clear()
    ms.update([1] * 3, seed=200)
    assert ms.counts() == (1, 1, 0, 0, 0, 0, 3) and [m._appended for m in ms.ssms] == [2, 1, 2]


def test_opt_hyp_and_replace_old_slide_nothing(fake):
    ms = Models(fake, [Conf(25), Conf(30)], (25, 30))
    ms.update([1, 1], opt_hyp=True)                                         # (0 training iterations: the update itself)
    assert ms.counts() == (0, 0, 0, 0, 2, 0, 2) and ms.fitted_on_the_last_rows()
    ms.update([1, 1], seed=200)                                             # ... and the next update is a full fit too
    assert ms.counts()[:4] == (0, 0, 0, 0) and ms.fitted_on_the_last_rows()
    ms.update([1, 1], seed=300)
    assert ms.counts() == (1, 1, 0, 0, 0, 0, 2)
    ms.update([40, 40], seed=400, replace_old=True)
    assert ms.counts() == (0, 0, 0, 0, 2, 0, 2) and ms.fitted_on_the_last_rows()
    ms.update([1, 1], seed=500)
    assert ms.counts() == (1, 1, 0, 0, 0, 0, 2) and ms.fitted_on_the_last_rows()


def test_seventeen_rows_fit_in_full(fake):
    assert gp_ssm_cem.MAX_SLIDE_ROWS == 16
    ms = Models(fake, [Conf(100), Conf(110)], (100, 110))
    ms.update([17, 17])                                                     # r = 17: past the measured break-even
    got = ms.counts()
    assert got[:4] == (0, 0, 0, 0) and got[4] + got[5] >= 1 and got[6] == 2
    assert ms.fitted_on_the_last_rows() and [m._appended for m in ms.ssms] == [0, 0]
    ms.update([16, 16], seed=200)
    assert ms.counts() == (1, 1, 0, 0, 0, 0, 2) and ms.fitted_on_the_last_rows()


def test_models_that_may_not_slide_are_fitted_together_on_their_last_rows(fake):
    ms = Models(fake, [Conf(25), Conf(30), Conf(35), Conf(28)], (25, 30, 35, 28))
    ms.ssms[2]._y_train = ms.ssms[2]._y_train.clone()
    ms.ssms[2]._y_train[7, 0] += 1.0                                        # a kept row is not the fitted one
    ms.all[2] = (ms.all[2][0], ms.ssms[2]._y_train)
    ms.ssms[3]._linv_current = False
    ms.update([1] * 4)
    assert ms.counts() == (1, 1, 0, 0, 0, 1, 4)
    assert [(kind, k, ns) for kind, k, ns, _ in fake.log] == [('drop', 1, [25, 30]), ('append', 1, [25, 30])]
    assert ms.fitted_on_the_last_rows() and [m._appended for m in ms.ssms] == [1, 1, 0, 0]
    # a DROPPED row that differs does not matter: the tail is what counts
    ms.ssms[0]._y_train = ms.ssms[0]._y_train.clone()
    ms.ssms[0]._y_train[0, 0] += 1.0
    ms.update([1] * 4, seed=200)
    assert ms.counts() == (1, 1, 0, 0, 0, 0, 4)


def test_window_chain_is_respected(fake):
    ms = Models(fake, [Conf(25, cem_gp_window_max_chain=2), Conf(30), Conf(35)], (25, 30, 35))
    seen = []
    for step in range(4):
        ms.update([1] * 3, seed=100 + 10 * step)
        seen.append(ms.counts())
    # the third update would be model 0's third slid row: it is fitted in full (alone: the lockstep fit of one model)
    assert seen == [(1, 1, 0, 0, 0, 0, 3), (1, 1, 0, 0, 0, 0, 3), (1, 1, 0, 0, 0, 1, 3), (1, 1, 0, 0, 0, 0, 3)]
    assert ms.fitted_on_the_last_rows() and [m._appended for m in ms.ssms] == [1, 4, 4]


def test_one_call_with_every_kind_of_update(fake):
    """One update_models_multi call in which every way a model can be updated occurs: two lockstep models that append two rows
    (one unwindowed, one below its window), two that slide by a row, one that slides by three, a windowed model without the
    setting, a model without conf.cem_gp_incremental and one whose installed fit may not be appended to.  The two that are
    fitted go first, together; then the groups in the order their first members stand in the list; then the lone slider;
    the windowed model without the setting last."""
    confs = [Conf(None), Conf(25), Conf(40), Conf(30), Conf(35), Conf(28, lockstep=False),
             Conf(None, lockstep=False, cem_gp_incremental=False), Conf(None)]
    ms = Models(fake, confs, (22, 25, 30, 30, 35, 28, 20, 21))
    ms.ssms[7]._append_ok = False
    ms.update([2, 1, 2, 1, 3, 1, 1, 2])
    order = [n for n in fake.calls if n in ('sx_gp_fit_multi', 'sx_gp_append_multi', 'sx_gp_drop_multi', 'sx_gp_drop',
                                            'sx_gp_append')]              # (a Counter keeps its keys in first-call order)
    assert order == ['sx_gp_fit_multi', 'sx_gp_append_multi', 'sx_gp_drop_multi', 'sx_gp_drop', 'sx_gp_append']
    assert fake.calls['sx_gp_drop_table'] == 1 and fake.calls['sx_gp_append_table'] == 2 and fake.calls['sx_gp_fit_table'] == 1
    assert ms.counts() == (1, 2, 2, 2, 0, 1, 8)
    (a2, k2, n2, _), (d, rd, n_old, words_d), (a, ka, n_train, words_a) = fake.log
    assert (a2, k2, n2) == ('append', 2, [24, 32])
    assert (d, rd, n_old) == ('drop', 1, [25, 30]) and (a, ka, n_train) == ('append', 1, [25, 30]) and words_d == words_a
    assert [m._appended for m in ms.ssms] == [2, 1, 2, 1, 3, 1, 0, 0]
    assert [m._append_ok for m in ms.ssms] == [True] * 6 + [False, True]
    assert ms.ssms[0]._lockstep_bufs.ws is not None and ms.ssms[1]._lockstep_bufs.drop.ws is not None
    assert all(m._lockstep_bufs is None for m in ms.ssms[2:])
    # (the model without conf.cem_gp_incremental keeps no fitted targets to compare: its rows are checked here, the others' by
    # `fitted_on_the_last_rows`)
    plain, (x, y) = ms.ssms.pop(6), ms.all.pop(6)
    assert torch.equal(plain._buffers[0], x) and torch.equal(plain.x_train, x) and torch.equal(plain.y_train, y)
    assert plain.device_model.n_train == 21 and plain._fit_state is None and plain._linv_current
    assert ms.fitted_on_the_last_rows()


# ---- host waits ---------------------------------------------------------------------------------------------------------------

def _reads(monkeypatch, fake, E, lockstep):
    """the device-to-host reads of one update that slides each of E full windows by a row, by kind"""
    ms = Models(fake, [Conf(25 + e, lockstep=lockstep) for e in range(E)], [25 + e for e in range(E)])
    seen = collections.Counter()
    real = dict(cpu=torch.Tensor.cpu, item=torch.Tensor.item, equal=torch.equal)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, 'cpu', lambda self, *a, **kw: (seen.update(['cpu']), real['cpu'](self, *a, **kw))[1])
        mp.setattr(torch.Tensor, 'item', lambda self: (seen.update(['item']), real['item'](self))[1])
        mp.setattr(torch, 'equal', lambda a, b: (seen.update(['equal']), real['equal'](a, b))[1])
        ms.update([1] * E)
    assert ms.counts() == ((1, 1, 0, 0, 0, 0, E) if lockstep else (0, 0, E, E, 0, 0, E))
    return dict(seen)


def test_reads_do_not_grow_with_the_models(monkeypatch, fake):
    """One read for the decision (every model's comparison of its kept fitted rows, in one tensor) and one for the results of
    both calls (status [E] and logdet [E x n_s] in one copy); model by model each model reads four times: two comparisons,
    the status and the log-determinant."""
    assert _reads(monkeypatch, fake, 2, True) == _reads(monkeypatch, fake, 6, True) == {'cpu': 2}
    for E in (2, 4):
        assert _reads(monkeypatch, fake, E, False) == {'equal': 2 * E, 'item': E, 'cpu': E}
