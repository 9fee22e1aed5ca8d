"""GPU: the lockstep append -- sx_gp_append_table / sx_gp_append_multi, k rows appended to each of E fitted exact GPs in one
launch sequence -- through the C ABI and through update_models_multi with conf.cem_gp_incremental_lockstep.

The contract is bit-equality: problem e's linv, alpha and logdet are those of sx_gp_append for model e alone.  So every case
here is compared with `torch.equal` against the single entry, which tests/test_gpu_gp_append.py checks against the
long-double factorisation; one case is checked against that truth directly, at the fit's own allowance.  The cases mix
sizes inside one call, so that the early exits and the per-problem extents are exercised at the tile (64), strip (16 / 96)
and part (256 = 4 blocks) edges.  The problems are those of tests/warm_path_reference.py; the single-model results are
computed once per problem and shared.  Every output buffer and every workspace ends in a canary."""
import ctypes

import numpy as np
import pytest
import torch

import append_reference as A
import test_gpu_gp_append as SA
import test_gpu_warm_path as WP
import warm_path_reference as R
from safe_exploration_amd import _lib

pytestmark = pytest.mark.gpu
DEV = WP.DEV
QUANTITIES = SA.QUANTITIES
CASES = (((5, 65, 257), 1), ((64, 130), 37), ((97, 1, 193, 346), 64), ((63, 256, 255), 2), ((130,), 37))   # (N_e; k)
SHAPES = ((1, 1), (2, 1), (4, 2), (1, 5))
RATIOS = (1e-2, 1e-6)

_singles = {}


def single(shape, n, k, ratio):
    """(p, fit of the first n rows, sx_gp_append of the k rows after them): computed once per problem, never modified"""
    key = (shape, n, k, ratio)
    if key not in _singles:
        p = R.problem(*shape, n + k, ratio)
        old = SA.fit_head(p, n)
        b = SA.run_append(p, n, SA._old(old))
        assert int(b['status'].t.item()) == 0
        _singles[key] = (p, old, b)
    return _singles[key]


def run_append_multi(items, status=None):
    """sx_gp_append_table + sx_gp_append_multi of `items` = [(p, n, old)]: the rows of p beyond the first n appended to
    `old` = {linv, alpha, logdet} (device tensors).  Returns (per-problem canaried buffers, the status Buf [E])."""
    lib = _lib.lib()
    E, n_s = len(items), items[0][0].n_s
    k = items[0][0].X.shape[0] - items[0][1]
    xs, ys = [WP._dev(p.X) for p, _, _ in items], [WP._dev(p.Y) for p, _, _ in items]
    models = (_lib.SxGpModel * E)(*[WP._struct(p, x) for (p, _, _), x in zip(items, xs)])
    sizes = [int(lib.sx_gp_append_workspace_bytes(n_s, p.X.shape[0], k)) for p, _, _ in items]
    assert min(sizes) > 0 and all(s % 8 == 0 for s in sizes)
    bufs = [dict(linv=WP.Buf(n_s, p.X.shape[0], p.X.shape[0]), alpha=WP.Buf(n_s, p.X.shape[0]), logdet=WP.Buf(n_s),
                 ws=WP.Buf(s // 8)) for (p, _, _), s in zip(items, sizes)]
    status = status if status is not None else WP.Buf(E, dtype=torch.int32)
    arr = lambda ts: (ctypes.c_void_p * E)(*[t.data_ptr() for t in ts])
    host = ctypes.create_string_buffer(int(lib.sx_gp_append_table_bytes(E)))
    _lib.check(lib.sx_gp_append_table(models, E, k, arr(ys), arr([old['linv'] for _, _, old in items]),
                                      arr([old['alpha'] for _, _, old in items]), arr([old['logdet'] for _, _, old in items]),
                                      arr([b['linv'].t for b in bufs]), arr([b['alpha'].t for b in bufs]),
                                      arr([b['logdet'].t for b in bufs]), _lib.ptr(status.t), arr([b['ws'].t for b in bufs]),
                                      (ctypes.c_int64 * E)(*sizes), host), 'sx_gp_append_table')
    table = torch.tensor(np.frombuffer(host.raw, dtype=np.uint8), device=DEV)
    _lib.check(lib.sx_gp_append_multi(models, E, k, _lib.ptr(table), _lib.stream_ptr(torch.device(DEV))),
               'sx_gp_append_multi')
    torch.cuda.synchronize()
    return bufs, status


def _intact(bufs, status, where):
    assert status.intact(), f'{where}: the canary after `status` was overwritten'
    for e, b in enumerate(bufs):
        for key, buf in b.items():
            assert buf.intact(), f'{where}: the canary after `{key}` of problem {e} was overwritten'


def _same_bits(b, want, where):
    for q in QUANTITIES:
        assert torch.equal(b[q].t, want[q].t), f'{where}: `{q}` differs from the single call\'s'


# ---- a. every problem of a call is its single call, bit for bit ----------------------------------------------------------------

@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('ns,k', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_every_problem_is_its_single_call(ns, k, shape, ratio):
    alone = [single(shape, n, k, ratio) for n in ns]
    bufs, status = run_append_multi([(p, n, SA._old(old)) for (p, old, _), n in zip(alone, ns)])
    where = f'{shape} N={ns}+{k} ratio={ratio:g}'
    _intact(bufs, status, where)
    assert status.t.tolist() == [0] * len(ns), where
    for e, (b, (_, old, want)) in enumerate(zip(bufs, alone)):
        _same_bits(b, want, f'{where} problem {e}')
        assert all(old[q].intact() for q in QUANTITIES)


def test_repeated_and_permuted_calls_give_the_same_bits():
    ns, k, shape = (97, 1, 193, 346), 64, (2, 1)
    alone = [single(shape, n, k, 1e-2) for n in ns]
    items = [(p, n, SA._old(old)) for (p, old, _), n in zip(alone, ns)]
    first, s1 = run_append_multi(items)
    again, s2 = run_append_multi(items)
    assert s1.t.tolist() == s2.t.tolist() == [0] * 4
    for b, c in zip(first, again):
        _same_bits(c, b, 'the same call again')
    for perm in ((3, 2, 1, 0), (1, 3, 0, 2)):
        got, s = run_append_multi([items[i] for i in perm])
        _intact(got, s, f'order {perm}')
        assert s.t.tolist() == [0] * 4
        for slot, i in enumerate(perm):
            _same_bits(got[slot], first[i], f'order {perm} problem {i}')
    # ... and a problem is independent of which others share the call
    got, s = run_append_multi([items[2], items[0]])
    _same_bits(got[0], first[2], 'a pair')
    _same_bits(got[1], first[0], 'a pair')


# ---- b. against the long-double factorisation, at the fit's own allowance --------------------------------------------------------

def test_one_call_against_the_long_double_factorisation():
    """(2,1), N = 64 and 130, k = 37, noise / outputscale = 1e-6: error / max(LAPACK's error, 8 eps) <= 32 on linv, alpha and
    logdet and on the two residuals, as test_gpu_gp_append.test_append_products asks of the single entry"""
    ns, k, shape, ratio = (64, 130), 37, (2, 1), 1e-6
    alone = [single(shape, n, k, ratio) for n in ns]
    bufs, status = run_append_multi([(p, n, SA._old(old)) for (p, old, _), n in zip(alone, ns)])
    assert status.t.tolist() == [0, 0]
    for b, (p, _, _), n in zip(bufs, alone, ns):
        case = SA._case(p, n)
        SA._healthy({q: b[q] for q in QUANTITIES}, case)
        got = {q: b[q].np() for q in QUANTITIES}
        WP.forward('sx_gp_append_multi', case, p, QUANTITIES, got)
        WP.residual_rule('sx_gp_append_multi', case, p, R.reference(p), got['linv'], got['alpha'])


# ---- c. not positive definite: the problem's own word, and nothing else -----------------------------------------------------------

def test_not_positive_definite_problem_keeps_to_itself():
    """tests/warm_path_reference.py's not_pd_problem (an arithmetic condition reported in a status word) between two healthy
    problems of its shape: N = 65, 65 and 130, k = 5"""
    bad = R.not_pd_problem(70, 5, 65)
    with pytest.raises(np.linalg.LinAlgError):
        A.append(bad, 65)
    healthy = [single((2, 1), n, 5, 1e-2) for n in (65, 130)]
    items = [(healthy[0][0], 65, SA._old(healthy[0][1])), (bad, 65, SA._old(SA.fit_head(bad, 65))),
             (healthy[1][0], 130, SA._old(healthy[1][1]))]
    bufs, status = run_append_multi(items)
    _intact(bufs, status, 'not PD')
    assert status.t.tolist() == [0, _lib.SX_STATUS_NOT_PD, 0]
    _same_bits(bufs[0], healthy[0][2], 'before the bad problem')
    _same_bits(bufs[2], healthy[1][2], 'after the bad problem')
    # the next call is unaffected
    good, s = run_append_multi([items[0], items[2]])
    assert s.t.tolist() == [0, 0]
    _same_bits(good[0], healthy[0][2], 'the next call')
    _same_bits(good[1], healthy[1][2], 'the next call')
    # the words are or-ed into: a set bit stays, in its own word
    kept, s = run_append_multi([items[2], items[0], items[0]], status=status)
    assert s.t.tolist() == [0, _lib.SX_STATUS_NOT_PD, 0]
    _same_bits(kept[1], healthy[0][2], 'beside a word that was set')


# ---- d. through Python -----------------------------------------------------------------------------------------------------------

class _Conf:
    device, exact_gp_kernel, exact_gp_training_iterations, cem_gp_incremental = DEV, 'rbf', 0, True

    def __init__(self, lockstep):
        self.cem_gp_incremental_lockstep = lockstep


def _gps(probs, first, lockstep):
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    out = []
    for p, n in zip(probs, first):
        ssm = GpCemSSM(_Conf(lockstep), p.n_s, p.n_u)
        ssm.set_hyperparameters(p.ls, p.s, p.noise)
        ssm.update_model(WP._dev(p.X[:n]), WP._dev(p.Y[:n]))
        out.append(ssm)
    return out


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _pack_writes(ssm):
    """Which elements of (a_pack, stage_tab) sx_gp_pack writes for this model: the buffers are sized by a capacity (the stage
    table's streams are padded to the longest), and what lies beyond a stream's end keeps whatever the allocation held.  The
    model is packed twice more into buffers filled with two different patterns; what both hold alike was written."""
    lib, m = _lib.lib(), _lib.SxGpModel.from_buffer_copy(ssm.device_model)
    runs = []
    for fill in (0, 0x01010101):
        a_pack = torch.full_like(_bits(ssm._buffers[1]), fill)
        stage_tab = torch.full_like(ssm._buffers[2], fill)
        m.a_pack, m.stage_tab = a_pack.data_ptr(), stage_tab.data_ptr()
        _lib.check(lib.sx_gp_pack(ctypes.byref(m), _lib.ptr(ssm._fit_ws[1]), _lib.ptr(ssm._alpha),
                                  _lib.stream_ptr(torch.device(DEV))), 'sx_gp_pack')
        runs.append((a_pack, stage_tab))
    torch.cuda.synchronize()
    return [u == v for u, v in zip(*runs)]


def _same_state(a, b, z, where):
    assert torch.equal(a.x_train, b.x_train) and torch.equal(a.y_train, b.y_train), where
    assert torch.equal(a._alpha, b._alpha), where
    assert a._fit_ws[0].shape == b._fit_ws[0].shape and torch.equal(a._fit_ws[1], b._fit_ws[1]), where
    assert len(a._buffers) == len(b._buffers) == 3 and torch.equal(a._buffers[0], b._buffers[0]), where
    for u, v, written in zip(a._buffers[1:], b._buffers[1:], _pack_writes(a)):
        assert u.shape == v.shape and int(written.sum()) > 0
        assert torch.equal(_bits(u)[written], _bits(v)[written]), where
    assert torch.equal(a._fit_state[0], b._fit_state[0]) and torch.equal(a._fit_state[1], b._fit_state[1]), where
    assert np.array_equal(a.information_gain(), b.information_gain()), where
    assert (a._appended, a._append_ok, a._linv_current) == (b._appended, b._append_ok, b._linv_current), where
    assert a.device_model.n_train == b.device_model.n_train and a.device_model.n_pad == b.device_model.n_pad
    for u, v in zip(a.predict_with_jacobians(z[:, :2], z[:, 2:]), b.predict_with_jacobians(z[:, :2], z[:, 2:])):
        assert torch.equal(u, v), where


def test_lockstep_update_equals_single_updates_bit_for_bit(monkeypatch):
    """Three (2,1) models with N = 40, 97 and 130 get one row each, eleven times in a row: update_models_multi with the
    setting on against update_model on twin models"""
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import update_models_multi
    first, steps = (40, 97, 130), 11
    probs = [R.problem(2, 1, n + steps) for n in first]
    z = WP._dev(R.queries(probs[0], 7, far=False))
    alone, together = _gps(probs, first, False), _gps(probs, first, True)
    spy = SA._Spy(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', spy)
    for step in range(steps):
        xs = [WP._dev(p.X[n + step:n + step + 1]) for p, n in zip(probs, first)]
        ys = [WP._dev(p.Y[n + step:n + step + 1]) for p, n in zip(probs, first)]
        for m, x, y in zip(alone, xs, ys):
            m.update_model(x, y)
        spy.calls.clear()
        update_models_multi(together, xs, ys)
        # (the packed buffers are compared on the elements sx_gp_pack writes: `_pack_writes`)
        assert (spy.calls['sx_gp_append_multi'], spy.calls['sx_gp_append_table'], spy.calls['sx_gp_append'],
                spy.calls['sx_gp_fit'], spy.calls['sx_gp_fit_multi'], spy.calls['sx_gp_pack']) == (1, 1, 0, 0, 0, 3), step
        for e, (a, b) in enumerate(zip(alone, together)):
            assert b._appended == step + 1
            _same_state(a, b, z, f'step {step} model {e}')


def test_setting_off_makes_the_calls_it_made(monkeypatch):
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import update_models_multi
    first = (40, 97)
    probs = [R.problem(2, 1, n + 1) for n in first]
    ssms = _gps(probs, first, False)
    spy = SA._Spy(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', spy)
    update_models_multi(ssms, [WP._dev(p.X[n:]) for p, n in zip(probs, first)], [WP._dev(p.Y[n:]) for p, n in zip(probs, first)])
    assert {n: c for n, c in spy.calls.items() if n.startswith(('sx_gp_append', 'sx_gp_fit', 'sx_gp_pack'))} \
        == {'sx_gp_append_workspace_bytes': 2, 'sx_gp_append': 2, 'sx_gp_pack_sizes': 2, 'sx_gp_pack': 2}
    assert [m._appended for m in ssms] == [1, 1]
