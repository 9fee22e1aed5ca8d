"""CPU: the subset-selection entries (sx_gp_select_workspace_bytes, sx_gp_select): their symbols and argtypes, the
argument checks -- all answered before any device access -- and the reference of tests/subset_reference.py: the
incremental algorithm equals the from-the-definition oracle on every case the GPU tests use, and every greedy step of
those cases is decided by a gap that float64 cannot blur."""
import ctypes
import os
import re

import numpy as np
import pytest

import subset_reference as S
import warm_path_reference as R
from safe_exploration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000   # a non-null "device" pointer: never dereferenced on the host side


def _model(n_s, n_u, n_train, x=FAKE):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.x_train = x
    for i in range(min(n_s * (n_s + n_u), len(m.inv_ls2))):
        m.inv_ls2[i] = 1.0 + i
    for d in range(min(n_s, len(m.noise))):
        m.outputscale[d], m.noise[d] = 0.5 + d, 0.01 * (d + 1)
    return m


def _models(shapes):
    return (_lib.SxGpModel * len(shapes))(*[_model(*s) for s in shapes])


def _select(models, E, m, seeds=None, n_seed=0, idx=FAKE, sel_var=FAKE, status=FAKE, ws=FAKE, ws_bytes=1 << 60):
    return _lib.lib().sx_gp_select(models, E, m, seeds, n_seed, idx, sel_var, status, ws, ws_bytes, None)


def test_symbols_and_argtypes():
    lib = _lib.lib()
    P, V, I, L = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    want = {'sx_gp_select_workspace_bytes': (L, [I, I, I, I]),
            'sx_gp_select': (I, [P(_lib.SxGpModel), I, I, V, I, V, V, V, V, L, V])}
    for name, (res, args) in want.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name in want:
        assert re.search(r'\b' + name + r'\s*\(', header), name


def test_workspace_bytes():
    ws = _lib.lib().sx_gp_select_workspace_bytes
    # the factor columns dominate: n_s x m x n_max doubles per problem
    for n_s, E, n, m in ((2, 1, 193, 64), (4, 3, 4100, 12), (1, 1, 65536, 4096), (2, 9, 97, 97)):
        got = ws(n_s, E, n, m)
        assert got >= 8 * E * n_s * (m + 1) * n and got < 8 * E * n_s * (m + 1) * n + E * (16 * n + 4096) + 64, (n_s, E, n, m)
    assert ws(2, 2, 300, 64) > ws(2, 1, 300, 64) > ws(2, 1, 300, 63) > ws(2, 1, 299, 63) > ws(1, 1, 299, 63) > 0
    for bad in ((0, 1, 100, 10), (5, 1, 100, 10), (2, 0, 100, 10), (2, 1, 0, 10), (2, 1, 100, 0), (2, 1, 100, 101),
                (2, 1, 65537, 10), (2, 1, 5000, 4097)):
        assert ws(*bad) < 0, bad


def test_argument_errors_before_any_device_access():
    ARG, UNSUP = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
    ok = _models([(2, 1, 60), (2, 1, 200)])
    # null pointers
    assert _select(None, 2, 10) == ARG
    for key in ('idx', 'sel_var', 'status', 'ws'):
        assert _select(ok, 2, 10, **{key: None}) == ARG, key
    assert _select(ok, 2, 10, seeds=None, n_seed=3) == ARG
    no_x = (_lib.SxGpModel * 2)(_model(2, 1, 60), _model(2, 1, 60, x=None))
    assert _select(no_x, 2, 10) == ARG
    # E, m, n_seed
    for E in (0, -1):
        assert _select(ok, E, 10) == ARG
    for m in (0, -3, 61, 200):        # m > n_e of the smaller problem
        assert _select(ok, 2, m) == ARG, m
    for n_seed in (-1, 11):
        assert _select(ok, 2, 10, seeds=FAKE, n_seed=n_seed) == ARG, n_seed
    # mixed or impossible shapes
    for shapes in ([(2, 1, 60), (2, 2, 60)], [(2, 1, 60), (4, 1, 60)], [(2, 1, 60), (2, 1, 0)], [(5, 1, 60)] * 2,
                   [(4, 3, 60)] * 2, [(0, 1, 60)] * 2):
        assert _select(_models(shapes), 2, 10) == ARG, shapes
    # a workspace that is too small, by one byte
    need = _lib.lib().sx_gp_select_workspace_bytes(2, 2, 200, 10)
    assert need > 0
    assert _select(ok, 2, 10, ws_bytes=need - 1) == ARG
    assert _select(ok, 2, 10, ws_bytes=0) == ARG
    # beyond the limits: m <= 4096 (the fit's), n_e <= 65536
    assert _select(_models([(2, 1, 5000)]), 1, 4097) == UNSUP
    assert _select(_models([(2, 1, 65537)]), 1, 10) == UNSUP
    assert _select(_models([(2, 1, 60), (2, 1, 65537)]), 2, 10) == UNSUP
    # ... and m > n_e is an argument error whatever the sizes
    assert _select(_models([(2, 1, 65537)]), 1, 65538) == ARG
    assert _select(_models([(2, 1, 4096)]), 1, 4097) == ARG


def test_python_setting_is_checked_on_the_host():
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM, MAX_TRAINING_POINTS

    class Conf:
        device = 'cpu'
        exact_gp_kernel = 'rbf'

    ssm = GpCemSSM(Conf(), 2, 1)
    assert ssm._subset_size is None and not ssm._selects(10 ** 6)      # off by default, and conf.m is not read
    conf = Conf()
    conf.m = 25
    assert GpCemSSM(conf, 2, 1)._subset_size is None
    conf.cem_gp_subset_size = 64
    ssm = GpCemSSM(conf, 2, 1)
    assert ssm._subset_size == 64 and ssm._selects(65) and not ssm._selects(64)
    ssm._check_pool_size(4100)                                          # a pool beyond the fit's limit is accepted
    with pytest.raises(ValueError, match='65536'):
        ssm._check_pool_size(65537)
    with pytest.raises(ValueError, match='4096'):
        GpCemSSM(Conf(), 2, 1)._check_pool_size(MAX_TRAINING_POINTS + 1)
    for bad in (0, -1, MAX_TRAINING_POINTS + 1):
        conf.cem_gp_subset_size = bad
        with pytest.raises(ValueError, match='cem_gp_subset_size'):
            GpCemSSM(conf, 2, 1)


@pytest.mark.parametrize('name,p,m,seeds', S.gpu_problems(), ids=[c[0] for c in S.gpu_problems()])
def test_incremental_equals_oracle_and_gaps_hold(name, p, m, seeds):
    """The two references agree on every case of the GPU tests, and every greedy step is decided by a gap of at least
    GAP_FLOOR x the prior: a condition on the inputs (the structural ties are exempt: step 0 of an RBF pool, where every
    point has the prior variance, and the duplicate pair of the tie problem, which must tie exactly)."""
    idx, sel, gap = S.oracle(p, m, seeds)
    inc_idx, inc_sel = S.incremental(p, m, seeds)
    prior = S.prior(p)
    greedy = np.arange(m) >= max(1, len(seeds))
    if name == 'tie':
        assert gap[1] == 0.0 and idx[1] == S.TIE_ROWS[0], 'the duplicate pair must tie exactly at step 1'
        greedy[1] = False
    worst = gap[greedy].min() / prior
    err = np.abs(inc_sel - sel).max() / prior
    print(f'SUBSET host {name}: min gap / prior {worst:.2e} at step {int(np.flatnonzero(greedy)[gap[greedy].argmin()])}, '
          f'|incremental - oracle| / prior {err:.2e}')
    assert np.array_equal(inc_idx, idx)
    assert err <= S.SEL_VAR_TOL
    assert gap[0] == (0.0 if not seeds else np.inf)
    assert worst >= S.GAP_FLOOR
    assert len(set(idx.tolist())) == m


def test_oracle_probes():
    """What the selection gives on the tie and the seed problem, as probed when the feature was specified"""
    idx, _, _ = S.oracle(S.tie_problem(), S.TIE_M)
    assert idx[:6].tolist() == [0, 20, 137, 83, 65, 132] and S.TIE_ROWS[1] not in idx
    idx, _, _ = S.oracle(R.problem(2, 1, 193, 1e-2), S.SEEDS_M, S.SEEDS)
    assert idx[:8].tolist() == list(S.SEEDS) + [160, 114, 65]
