"""CPU: the multi-model warm-path entries (sx_gp_fit_table[_bytes], sx_gp_fit_multi, sx_gp_mll_grad_multi): their
symbols and argtypes, the table layout against include/sx_amd.h, and the argument checks, all answered before any device
access."""
import ctypes
import os
import re
import struct

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


def _ptrs(E, base=FAKE, null_at=None):
    return (ctypes.c_void_p * E)(*[None if e == null_at else base + 0x100 * e for e in range(E)])


def _table(lib, models, E, table, null=None):
    """sx_gp_fit_table with fake device pointers; null = {k: problem index or 'all'} nulls array k (y, work, linv, alpha,
    logdet) or one of its entries."""
    null = null or {}
    arrs = [_ptrs(E, base=0x10000 * (k + 1), null_at=null.get(k)) for k in range(5)]
    for k in range(5):
        if null.get(k) == 'all':
            arrs[k] = None
    return lib.sx_gp_fit_table(models, E, *arrs, FAKE, 0x20000, 0x30000, table)


def test_symbols_and_argtypes():
    lib = _lib.lib()
    P, V, I = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int
    want = {'sx_gp_fit_table_bytes': (ctypes.c_int64, [I]),
            'sx_gp_fit_table': (I, [P(_lib.SxGpModel), I] + [P(V)] * 5 + [V] * 4),
            'sx_gp_fit_multi': (I, [P(_lib.SxGpModel), I, V, V]),
            'sx_gp_mll_grad_multi': (I, [P(_lib.SxGpModel), I, V, V])}
    for name, (res, args) in want.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    for name in want:
        assert re.search(r'\b' + name + r'\s*\(', header), name


def test_table_size_matches_the_header():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    entry = int(re.search(r'#define SX_GP_FIT_ENTRY_BYTES (\d+)', header).group(1))
    assert entry == _lib.SX_GP_FIT_ENTRY_BYTES and entry % 8 == 0
    lib = _lib.lib()
    for E in (1, 2, 5, 6, 64):
        assert lib.sx_gp_fit_table_bytes(E) == E * entry
    for E in (0, -1):
        assert lib.sx_gp_fit_table_bytes(E) < 0


def test_table_lays_out_each_problem():
    """The host-side table: problem e's hyper-parameters, pointers (status / mll / grad offset to its rows), N and the
    blocked path's block count (0 for N <= 96, the one-workgroup path)."""
    lib = _lib.lib()
    shapes = [(2, 1, 7), (2, 1, 96), (2, 1, 97), (2, 1, 410)]
    E, entry = len(shapes), _lib.SX_GP_FIT_ENTRY_BYTES
    models = _models(shapes)
    buf = ctypes.create_string_buffer(E * entry)
    assert _table(lib, models, E, buf) == _lib.SX_OK
    raw = buf.raw
    D, n_s = 3, 2
    for e, (_, _, n) in enumerate(shapes):
        t = raw[e * entry:(e + 1) * entry]
        doubles = struct.unpack_from('32d', t, 0)
        assert doubles[:n_s * D] == tuple(models[e].inv_ls2[:n_s * D])
        assert doubles[24:26] == (0.5, 1.5) and doubles[28:30] == (0.01, 0.02)
        x, y, lmat, scratch, linv, alpha, logdet, status, mll, grad = struct.unpack_from('10Q', t, 256)
        assert x == FAKE and y == 0x10000 + 0x100 * e and lmat == scratch == 0x20000 + 0x100 * e
        assert (linv, alpha, logdet) == tuple(0x10000 * k + 0x100 * e for k in (3, 4, 5))
        assert status == FAKE + 4 * e and mll == 0x20000 + 8 * n_s * e and grad == 0x30000 + 8 * n_s * (D + 2) * e
        n_, D_, ns_, nblk, panel = struct.unpack_from('5i', t, 336)
        assert (n_, D_, ns_) == (n, D, n_s)
        assert nblk == (0 if n <= 96 else (n + 63) // 64) and panel == 32


def test_argument_errors_before_any_device_access():
    lib = _lib.lib()
    ok = _models([(2, 1, 60), (2, 1, 200)])
    host = ctypes.create_string_buffer(2 * _lib.SX_GP_FIT_ENTRY_BYTES)
    ARG, UNSUP = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
    # E = 0, null models / table
    assert _table(lib, ok, 0, host) == ARG
    assert _table(lib, None, 2, host) == ARG
    assert _table(lib, ok, 2, None) == ARG
    for call in (lib.sx_gp_fit_multi, lib.sx_gp_mll_grad_multi):
        assert call(ok, 0, FAKE, None) == ARG
        assert call(ok, -1, FAKE, None) == ARG
        assert call(None, 2, FAKE, None) == ARG
        assert call(ok, 2, None, None) == ARG
    # a null pointer array, or one problem's null buffer
    for k in range(5):
        assert _table(lib, ok, 2, host, {k: 'all'}) == ARG
        assert _table(lib, ok, 2, host, {k: 1}) == ARG
    assert lib.sx_gp_fit_table(ok, 2, *[_ptrs(2)] * 5, None, FAKE, FAKE, host) == ARG    # status
    assert lib.sx_gp_fit_table(ok, 2, *[_ptrs(2)] * 5, FAKE, None, FAKE, host) == ARG    # mll
    assert lib.sx_gp_fit_table(ok, 2, *[_ptrs(2)] * 5, FAKE, FAKE, None, host) == ARG    # grad
    no_x = (_lib.SxGpModel * 2)(_model(2, 1, 60), _model(2, 1, 60, x=None))
    assert _table(lib, no_x, 2, host) == ARG
    # N > 4096: unsupported, as sx_gp_fit
    big = _models([(2, 1, 60), (2, 1, 4097)])
    assert _table(lib, big, 2, host) == UNSUP
    assert lib.sx_gp_fit_multi(big, 2, FAKE, None) == UNSUP
    assert lib.sx_gp_mll_grad_multi(big, 2, FAKE, None) == UNSUP
    assert _table(lib, _models([(2, 1, 4096), (2, 1, 60)]), 2, host) == _lib.SX_OK
    # mismatched (n_s, n_u), non-positive N, dimensions beyond the compiled limits
    for shapes in ([(2, 1, 60), (2, 2, 60)], [(2, 1, 60), (4, 1, 60)], [(2, 1, 60), (2, 1, 0)], [(5, 1, 60)] * 2,
                   [(4, 3, 60)] * 2, [(0, 1, 60)] * 2):
        bad = _models(shapes)
        assert _table(lib, bad, 2, host) == ARG, shapes
        assert lib.sx_gp_fit_multi(bad, 2, FAKE, None) == ARG, shapes
        assert lib.sx_gp_mll_grad_multi(bad, 2, FAKE, None) == ARG, shapes
