"""GPU: both ranking kernels (cem_rank_count_kernel, cem_rank_kernel<4 | 8 | 16>) at every case of tests/rank_reference.py,
in all four output modes -- rows and refit, rows only, refit only, neither.  The launcher chooses the kernel by shape and
mode (rank_reference.expected_kernel restates its rule), and the two kernels promise different elite orders (DESIGN.md
3.4: counting returns rank order, one workgroup the best first and the rest in index order), so `elite_idx` is compared
EXACTLY: a case that silently moves to the other kernel fails.  Rows, best and best_ok are compared bit for bit, mean and
std against a long-double refit within rank_reference.refit_bounds (derived from the f64 format, not measured).

Nothing here sets SX_RANK_PATH: the kernels are forced by shape and mode, as production does."""
import ctypes
import os

import numpy as np
import pytest
import torch

import rank_reference as rr
from oracle import cem as ocem

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# largest |error| / bound seen, per kernel: printed when the module is done (the figures of DESIGN.md 3.4)
WORST = {k: {'mean': 0.0, 'std': 0.0} for k in rr.KERNELS}


def T(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope='module', autouse=True)
def report_refit_errors():
    yield
    for kernel, w in WORST.items():
        print(f'\nrefit error / refit_bounds, largest seen, {kernel}: mean {w["mean"]:.3f}, std {w["std"]:.3f}')


class Reference:
    """Per problem of a case, computed once and shared by the modes: the oracle's order in both kernels' forms and the
    long-double refit (which does not depend on the order of the rows) with its bounds."""

    def __init__(self, con, obj, act, k):
        self.con, self.obj, self.act, self.k = con, obj, act, k
        E = con.shape[0]
        self.count = [rr.expected_order(con[e], obj[e], k, 'count') for e in range(E)]
        self.select = [[o[0]] + sorted(o[1:]) for o in self.count]
        self.hp = [rr.refit_hp(act[e][self.count[e]]) for e in range(E)]
        self.bounds = [rr.refit_bounds(act[e][self.count[e]]) for e in range(E)]

    def order(self, e, kernel):
        return self.count[e] if kernel == 'count' else self.select[e]


def check(out, ref, kernel, rows, refit, plain=False, where=''):
    con, obj, act, k = ref.con, ref.obj, ref.act, ref.k
    E, P = con.shape
    idx = out['elite_idx'].cpu().numpy()
    got_rows = out['elite_rows'].cpu().numpy() if rows else None
    best, best_ok = out['best'].cpu().numpy(), out['best_ok'].cpu().numpy()
    assert (out['elite_rows'] is not None) == rows and (out['mean'] is not None) == refit
    mean, std = (out['mean'].cpu().numpy(), out['std'].cpu().numpy()) if refit else (None, None)
    for e in range(E):
        want = ref.order(e, kernel)
        got = idx[e]
        tag = f'{where} kernel {kernel} problem {e}'
        assert len(set(got.tolist())) == k and got.min() >= 0 and got.max() < P, tag
        np.testing.assert_array_equal(got, want, err_msg=tag)
        if rows:
            np.testing.assert_array_equal(bits(got_rows[e][:, 0]), bits(con[e][want]), err_msg=tag)
            np.testing.assert_array_equal(bits(got_rows[e][:, 1]), bits(obj[e][want]), err_msg=tag)
            np.testing.assert_array_equal(bits(got_rows[e][:, 2:]), bits(act[e][want]), err_msg=tag)
        np.testing.assert_array_equal(bits(best[e]), bits(act[e][want[0]]), err_msg=tag)
        assert int(best_ok[e]) == int(con[e][want[0]] == 0), tag
        if refit:
            (mh, sh), (dm, ds) = ref.hp[e], ref.bounds[e]
            em, es = np.abs(mean[e] - mh), np.abs(std[e] - sh)
            fm = float(np.max(np.where(dm > 0, em / np.where(dm > 0, dm, 1), np.where(em > 0, np.inf, 0))))
            fs = float(np.max(np.where(ds > 0, es / np.where(ds > 0, ds, 1), np.where(es > 0, np.inf, 0))))
            WORST[kernel]['mean'], WORST[kernel]['std'] = max(WORST[kernel]['mean'], fm), max(WORST[kernel]['std'], fs)
            assert fm <= 1 and fs <= 1, f'{tag}: refit error is {fm:.3f} (mean) and {fs:.3f} (std) of refit_bounds'
            if k == 1:
                assert (std[e] == 0).all(), tag
            if plain:
                m, s = ocem.refit(act[e][want])
                np.testing.assert_allclose(mean[e], m, rtol=1e-12, atol=1e-14, err_msg=tag)
                np.testing.assert_allclose(std[e], s, rtol=1e-12, atol=1e-14, err_msg=tag)


def run(case, con, obj, act, rows, refit, rows_out=False):
    from safe_exploration_amd.cem_mpc import cem_rank_refit
    E, P, L, k = case.E, case.P, case.L, case.k
    kw = dict(want_rows=rows and not rows_out, want_refit=refit)
    if rows_out:
        kw['rows_out'] = torch.full((E, k, 2 + L), np.nan, dtype=torch.float64, device=DEV)
    if case.strided:
        flat = T(np.concatenate((con[..., None], obj[..., None], act), axis=2)).reshape(-1)
        return cem_rank_refit(flat, flat[1:], flat[2:], k, cost_stride=2 + L, act_stride=2 + L, row_len=L, num_candidates=P,
                              num_problems=E, **kw)
    return cem_rank_refit(T(con), T(obj), T(act), k, **kw)


@pytest.mark.parametrize('case', rr.CASES, ids=lambda c: c.name)
def test_case_in_all_four_modes(case):
    con, obj, act = case.data()
    ref = Reference(con, obj, act, case.k)
    assert rr.expected_kernel(case.E, case.P, *case.via) == case.kernel
    for rows, refit in rr.MODES:
        kernel = rr.expected_kernel(case.E, case.P, rows, refit)
        check(run(case, con, obj, act, rows, refit), ref, kernel, rows, refit, case.plain, f'{case.name} rows={rows} refit={refit}')
        if case.strided and rows:      # the elite rows into a buffer handed in (the multi-GPU solve's exchange slot)
            check(run(case, con, obj, act, rows, refit, rows_out=True), ref, kernel, rows, refit, case.plain,
                  f'{case.name} rows_out refit={refit}')


def test_regression_fixture_on_the_kernel_it_was_written_for(golden_dir):
    """tests/golden/rank_case_r02.npz (8192 candidates, k = 819, 29 distinct constraint costs) is the input on which round
    1's cem_rank_kernel<8> put a tied elite into a neighbour's slot.  With rows and one problem the launcher now counts
    (tests/test_gpu_parity.py::test_rank_regression_case_round2); here the fixture reaches cem_rank_kernel<8> again: in
    refit-only mode, and as two problems with rows (1024 workgroups would be more than the counting kernel takes).  Once each:
    the cause was fixed in round 2, this pins it."""
    g = np.load(os.path.join(golden_dir, 'rank_case_r02.npz'))
    con, obj, k = g['con'], g['obj'], int(g['k'])
    P = len(con)
    assert (P, k) == (8192, 819)
    act = np.random.default_rng(2).normal(size=(P, 5))
    for E, (rows, refit) in ((1, rr.REFIT_ONLY), (2, rr.ROWS_REFIT)):
        assert rr.expected_kernel(E, P, rows, refit) == 'select8'
        c, o, a = (np.ascontiguousarray(np.broadcast_to(x[None], (E,) + x.shape)) for x in (con, obj, act))
        case = rr.Case(f'r02_E{E}', E, P, k, 5, 'select8', (rows, refit), None)
        check(run(case, c, o, a, rows, refit), Reference(c, o, a, k), 'select8', rows, refit, True, case.name)


def test_ticket_slots_reset_themselves_over_200_launches():
    """The counting kernel's refit is done by the workgroup that takes a problem's last ticket; the ticket cells are 64
    sets in rotation, each wrapped back to zero by the launch that used it.  200 consecutive refit launches on ONE stream
    cycle through five shapes, so every set is reused with other tile counts and problem counts; every mean / std buffer
    starts as NaN and must hold the refit afterwards.  One synchronisation, at the end.  This shows that the tickets reset
    themselves; launches that overlap in time on several streams are not tested here."""
    from safe_exploration_amd.cem_mpc import cem_rank_refit
    shapes = ((1, 16, 7), (2, 130, 40), (64, 5, 2), (3, 1000, 100), (1, 4096, 409))
    L = 6
    given, refs = [], []
    for E, P, k in shapes:
        assert rr.expected_kernel(E, P, True, True) == 'count'
        con, obj, act = rr.generic(E, P, L)(np.random.default_rng(P))
        given.append((T(con), T(obj), T(act), k))
        refs.append(Reference(con, obj, act, k))
    outs = []
    for i in range(200):
        con, obj, act, k = given[i % 5]
        E = con.size(0)
        # (the wrapper allocates mean / std itself: hand-made buffers go through the C entry)
        o = dict(elite_idx=torch.empty((E, k), dtype=torch.int32, device=DEV),
                 elite_rows=torch.empty((E, k, 2 + L), dtype=torch.float64, device=DEV),
                 mean=torch.full((E, L), np.nan, dtype=torch.float64, device=DEV),
                 std=torch.full((E, L), np.nan, dtype=torch.float64, device=DEV),
                 best=torch.empty((E, L), dtype=torch.float64, device=DEV),
                 best_ok=torch.empty((E,), dtype=torch.int32, device=DEV))
        launch(E, con.size(1), k, L, con, obj, act, o)
        outs.append(o)
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert not bool(torch.isnan(o['mean']).any()) and not bool(torch.isnan(o['std']).any()), f'launch {i}: no refit'
        check(o, refs[i % 5], 'count', True, True, True, f'launch {i}')


def launch(E, P, k, L, con, obj, act, o):
    from safe_exploration_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().sx_cem_rank_refit(E, P, k, L, p(con), p(obj), 1, p(act), L, p(o['elite_idx']), p(o['elite_rows']),
                                            p(o['mean']), p(o['std']), p(o['best']), p(o['best_ok']),
                                            _lib.stream_ptr(torch.device(DEV))), 'sx_cem_rank_refit')


# rows-and-refit mode at P = 1025, k = 7, L = 33: two problems count; twelve are 780 workgroups, one more than counting takes
# at this P, and reach cem_rank_kernel<4> with rows; <16> needs more than 8192 candidates
@pytest.mark.parametrize('kernel,E,P', [('count', 2, 1025), ('select4', 12, 1025), ('select16', 2, 8193)])
def test_nothing_is_written_outside_the_outputs(kernel, E, P):
    """Every output of the C entry sits inside a larger tensor with 64 sentinel elements either side: the sentinels are
    untouched and the payload is right."""
    k, L, PAD = 7, 33, 64
    assert rr.expected_kernel(E, P, True, True) == kernel
    con, obj, act = rr.generic(E, P, L)(np.random.default_rng(E + P))
    ref = Reference(con, obj, act, k)
    sizes = dict(elite_idx=(E, k), elite_rows=(E, k, 2 + L), mean=(E, L), std=(E, L), best=(E, L), best_ok=(E,))
    whole, o = {}, {}
    for name, shape in sizes.items():
        integer = name in ('elite_idx', 'best_ok')
        n = int(np.prod(shape))
        whole[name] = (torch.full((n + 2 * PAD,), -77, dtype=torch.int32, device=DEV) if integer
                       else torch.full((n + 2 * PAD,), -77.25, dtype=torch.float64, device=DEV))
        o[name] = whole[name][PAD:PAD + n].view(shape)
    launch(E, P, k, L, T(con), T(obj), T(act), o)
    torch.cuda.synchronize()
    for name, w in whole.items():
        w = w.cpu().numpy()
        assert (w[:PAD] == w.dtype.type(-77.25 if w.dtype == np.float64 else -77)).all(), f'{name}: written in front of it'
        assert (w[-PAD:] == w.dtype.type(-77.25 if w.dtype == np.float64 else -77)).all(), f'{name}: written behind it'
    check(o, ref, kernel, True, True, True, f'{kernel} E={E} P={P}')
