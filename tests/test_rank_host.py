"""CPU: the helpers of tests/rank_reference.py against the oracle, every case of the ranking case table (the kernel it must
reach, the structure it claims, an observable difference between the two kernels' orders), and the refusals of
sx_cem_rank_refit that return before any launch."""
import ctypes
import os

import numpy as np
import pytest

import rank_reference as rr
from oracle import cem as ocem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from safe_exploration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def kernel_choice_is_forced():
    return bool(os.environ.get('SX_RANK_PATH'))


def test_refit_hp_agrees_with_the_oracle():
    rng = np.random.default_rng(0)
    for k, L in ((1, 4), (2, 3), (17, 33), (409, 15), (2048, 5)):
        x = rng.normal(size=(k, L))
        m, s = ocem.refit(x)
        mh, sh = rr.refit_hp(x)
        assert mh.dtype == np.longdouble and sh.dtype == np.longdouble
        np.testing.assert_allclose(mh.astype(np.float64), m, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(sh.astype(np.float64), s, rtol=1e-13, atol=1e-13)
        if k == 1:
            assert (sh == 0).all()
        dm, ds = rr.refit_bounds(x)
        assert (np.abs(m - mh) <= dm).all() and (np.abs(s - sh) <= ds).all()      # numpy's two-pass f64 is inside them


def test_expected_order_is_the_oracles_set_with_the_oracles_best_first():
    rng = np.random.default_rng(1)
    for P, k in ((1, 1), (2, 2), (50, 7), (700, 700), (3000, 300)):
        con = rng.choice([0., 3., 10., np.nan, np.inf], size=P)
        obj = rng.normal(size=P).round(1)
        want = ocem.rank(con, obj, k)
        assert rr.expected_order(con, obj, k, 'count') == want.tolist()
        for kernel in ('select4', 'select8', 'select16'):
            got = rr.expected_order(con, obj, k, kernel)
            assert got[0] == want[0] and sorted(got) == sorted(want.tolist()) and got[1:] == sorted(got[1:])


def test_sortable_key_orders_as_the_oracle():
    """The keys the structural predicates are computed from order doubles as oracle.cem.rank does."""
    rng = np.random.default_rng(2)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1.0, np.nextafter(1.0, 2.0), -1.0, 3.0, 1e300])
    for _ in range(50):
        x = rng.choice(pool, size=40)
        key = rr.sortable_key(x)
        by_key = np.lexsort((np.arange(40), key))
        np.testing.assert_array_equal(by_key, ocem.rank(np.zeros(40), x, 40))
    assert rr.sortable_key([0.0])[0] == rr.sortable_key([-0.0])[0] and rr.sortable_key([np.nan])[0] == np.uint64(2 ** 64 - 1)


def test_the_case_table_covers_what_it_is_there_for():
    by = {k: [c for c in rr.CASES if c.kernel == k] for k in rr.KERNELS}
    assert all(len(v) >= 10 for v in by.values())
    assert {c.P for c in by['select4']} >= {1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096}
    assert {c.P for c in by['select8']} >= {4097, 8192} and {c.P for c in by['select16']} >= {8193, 16384}
    assert {c.P for c in by['count']} >= {1, 15, 16, 17, 127, 128, 129, 1024, 4097}
    for P in (1024, 4097, 16384):
        for E in (1, 3):
            ks = {c.k for c in rr.CASES if c.name.startswith(f'width_P{P}_E{E}_')}
            assert {1, 2, min(P, 2048)} < ks                   # ... and a tie-run boundary
            assert any(c.props.get('cut_in_tie') for c in rr.CASES if c.name.startswith(f'width_P{P}_E{E}_'))


@pytest.mark.parametrize('case', rr.CASES, ids=lambda c: c.name)
def test_case(case, lib):
    con, obj, _ = case.data()
    # (a) the launcher takes the kernel the case names, in the mode the case names
    if not kernel_choice_is_forced():
        assert rr.expected_kernel(case.E, case.P, *case.via) == case.kernel
        # refit-only never counts; more than 8192 candidates or more than 64 problems never count
        assert rr.expected_kernel(case.E, case.P, *rr.REFIT_ONLY) != 'count'
        if case.P > 8192 or case.E > 64:
            assert all(rr.expected_kernel(case.E, case.P, *m) != 'count' for m in rr.MODES)
    # (b) the structure it claims
    assert 1 <= case.k <= min(case.P, 2048)
    rr.check_props(case, con, obj)
    # (c) the two kernels' orders differ on it: which kernel ran is observable
    select = 'select4' if case.kernel == 'count' else case.kernel
    differ = any(rr.expected_order(con[e], obj[e], case.k, 'count') != rr.expected_order(con[e], obj[e], case.k, select)
                 for e in range(case.E))
    assert differ == (not case.same_order and case.k > 2), case.name


def test_the_fuzz_tool_restates_the_same_rule_and_orders():
    """tools/rank_fuzz.py stands alone (it must run without tests/ on its path): its kernel_of / order_of agree with
    rank_reference's on every shape and mode of the case table, and on the orders of its smaller cases."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('rank_fuzz', os.path.join(ROOT, 'tools', 'rank_fuzz.py'))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    assert fuzz.KERNELS == rr.KERNELS and fuzz.MODES == rr.MODES
    for E, P in sorted({(c.E, c.P) for c in rr.CASES}):
        for mode in rr.MODES:
            assert fuzz.kernel_of(E, P, *mode) == rr.expected_kernel(E, P, *mode), (E, P, mode)
    for case in rr.CASES:
        if case.P <= 1500 and case.E <= 3:
            con, obj, _ = case.data()
            for kernel in ('count', case.kernel):
                assert fuzz.order_of(con[0], obj[0], case.k, kernel) == rr.expected_order(con[0], obj[0], case.k, kernel)


def test_a_one_pass_variance_fails_the_offset_case_and_a_two_pass_passes():
    """The 1e8 + N(0, 1) actions are there to catch a refit that gives up the second pass: sum x^2 - k mean^2 in f64 misses
    refit_bounds on them, numpy's two-pass f64 is inside."""
    case = next(c for c in rr.CASES if c.name == 'refit_offset_1e8_k40')
    con, obj, act = case.data()
    x = act[0][rr.expected_order(con[0], obj[0], case.k, 'select4')]
    assert abs(x.mean() - 1e8) < 10
    mh, sh = rr.refit_hp(x)
    dm, ds = rr.refit_bounds(x)
    k = x.shape[0]
    with np.errstate(invalid='ignore'):                                   # (a negative variance gives NaN: a miss too)
        one_pass = np.sqrt(((x * x).sum(axis=0) - k * x.mean(axis=0) ** 2) / (k - 1))
    assert not (np.abs(one_pass - sh) <= ds).any()
    m, s = ocem.refit(x)
    assert (np.abs(m - mh) <= dm).all() and (np.abs(s - sh) <= ds).all()


def rank_refit_args(E=1, P=16, k=4, L=3, con=True, obj=True, act=True):
    """Arguments of sx_cem_rank_refit with host buffers in place of device ones: every call here returns before a launch."""
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return (E, P, k, L, p if con else None, p if obj else None, 1, p if act else None, L, p, None, None, None, p, p, None), buf


def test_rank_refit_refuses_before_any_launch(lib):
    from safe_exploration_amd import _lib

    def call(**kw):
        args, keep = rank_refit_args(**kw)
        return lib.sx_cem_rank_refit(*args)
    assert call(P=16, k=17) == _lib.SX_ERR_ARG                          # k > P
    assert call(P=4096, k=2049) == _lib.SX_ERR_UNSUPPORTED              # more elites than the kernels hold
    assert call(P=16385, k=4) == _lib.SX_ERR_UNSUPPORTED                # more candidates than 16 slots of 1024 threads
    for bad in (0, -1):
        assert call(E=bad) == _lib.SX_ERR_ARG
        assert call(P=bad) == _lib.SX_ERR_ARG
        assert call(k=bad) == _lib.SX_ERR_ARG
        assert call(L=bad) == _lib.SX_ERR_ARG
    for name in ('con', 'obj', 'act'):
        assert call(**{name: False}) == _lib.SX_ERR_ARG
