"""CPU: the exact-GP rollout plan's answers through sx_cem_rollout_form / sx_cem_rollout_workspace_bytes and the large-N
path's tiling through sx_gp_big_tiling (no device access), and the compiled shape list (SX_ROLLOUT_SHAPES) against
ssm_cem.JUNK_FUSED_SHAPES."""
import ctypes
import os
import re

import pytest

from safe_exploration_amd import _lib
from safe_exploration_amd.ssm_cem.ssm_cem import JUNK_FUSED_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SX_FORM_STREAM, SX_FORM_RW, SX_FORM_RH, SX_FORM_BYOUT, SX_FORM_BIG = 0, 1, 2, 3, 4   # include/sx_amd.h


def _model(n_s, n_u, n_train):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.n_pad = (n_train + 1 + n_s + n_u + 15) // 16 * 16   # sx_gp.hpp: gp_n_pad
    return m


@pytest.mark.skipif(bool(os.environ.get('SX_ROLLOUT')), reason='SX_ROLLOUT forces a form')
@pytest.mark.parametrize('n_s,n_u,N,form,ws', [
    (2, 1, 200, SX_FORM_RH, 0),
    (2, 1, 260, SX_FORM_STREAM, 0),
    (2, 1, 600, SX_FORM_BYOUT, 0),
    (2, 1, 1100, SX_FORM_BIG, 74_088_448),
    (3, 1, 77, SX_FORM_RW, 0),
    (4, 1, 128, SX_FORM_STREAM, 0),
    (4, 1, 260, SX_FORM_BYOUT, 0),
])
def test_rollout_form_and_workspace(n_s, n_u, N, form, ws):
    lib, m, H = _lib.lib(), _model(n_s, n_u, N), 15
    assert lib.sx_cem_rollout_form(ctypes.byref(m), H) == form
    assert lib.sx_cem_rollout_workspace_bytes(ctypes.byref(m), 1, 4096, H) == ws


def test_rollout_form_of_a_shape_without_a_kernel():
    """(3, 2) -- the widened real-output model of a junk (3, 1, shift 1) wrapper -- has no plain rollout: the form query
    says so, while the workspace query still answers for the training set."""
    lib, m = _lib.lib(), _model(3, 2, 77)
    assert lib.sx_cem_rollout_form(ctypes.byref(m), 15) < 0
    assert lib.sx_cem_rollout_workspace_bytes(ctypes.byref(m), 1, 4096, 15) == 0
    assert lib.sx_cem_rollout_workspace_bytes(ctypes.byref(_model(3, 2, 1100)), 1, 4096, 15) > 0


TRMM_SETTINGS = [v for v in ('SX_TRMM_ORDER', 'SX_TRMM_VARIANT', 'SX_TRMM_PT') if os.environ.get(v)]


@pytest.mark.skipif(bool(TRMM_SETTINGS), reason='SX_TRMM_* force a tiling')
@pytest.mark.parametrize('n_s,n_u,N,particles,pt,order,grid', [
    (2, 1, 1100, 130, 4, 8, 72),
    (2, 1, 1100, 1100, 4, 16, 180),       # paired, odd row_tiles (9)
    (2, 1, 1100, 4096, 4, 8, 1152),
    (2, 1, 1149, 1153, 4, 16, 200),       # the last row tile holds Jacobian rows only
    (1, 1, 1022, 2100, 4, 16, 170),
    (4, 2, 1100, 130, 4, 8, 144),
    (4, 2, 1100, 600, 4, 16, 200),
    (4, 2, 1100, 5400, 8, 16, 860),
    (4, 2, 1100, 6200, 8, 8, 1764),
    (4, 1, 2000, 3200, 8, 8, 1600),
    (4, 1, 2000, 4096, 8, 16, 1024),      # paired, even row_tiles (16)
    (4, 1, 2000, 16384, 8, 8, 8192),      # BASELINE config 4
    (4, 1, 1010, 6200, 8, 8, 1568),
])
def test_big_tiling_of_the_default_routes(n_s, n_u, N, particles, pt, order, grid):
    """sx_gp_big_tiling, the tiling launch_trmm acts on (plan_big_tiling, sx_big_launch.hpp), without a device: the four
    default routes -- 128 x 64 or 128 x 128 tiles, longest-first (8) or paired (16) order -- at the sizes the GPU tests of
    tests/test_gpu_big_path.py run and at config 4's.  The rows were confirmed against the launcher's decision code as it
    stood before it moved into plan_big_tiling."""
    got = _lib.big_tiling(_model(n_s, n_u, N), particles)
    assert got == {'pt': pt, 'order': order, 'variant': 13, 'grid': grid}


def test_big_tiling_rejects_bad_arguments():
    lib, m = _lib.lib(), _model(2, 1, 1100)
    pt, order, variant, grid = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    outs = [ctypes.byref(pt), ctypes.byref(order), ctypes.byref(variant), ctypes.byref(grid)]
    assert lib.sx_gp_big_tiling(ctypes.byref(m), 130, *outs) == _lib.SX_OK
    assert lib.sx_gp_big_tiling(None, 130, *outs) == _lib.SX_ERR_ARG
    assert lib.sx_gp_big_tiling(ctypes.byref(m), -1, *outs) == _lib.SX_ERR_ARG
    for i in range(4):
        assert lib.sx_gp_big_tiling(ctypes.byref(m), 130, *(outs[:i] + [None] + outs[i + 1:])) == _lib.SX_ERR_ARG
    assert lib.sx_gp_big_tiling(ctypes.byref(_lib.SxGpModel()), 130, *outs) == _lib.SX_ERR_ARG   # no sizes


def test_junk_fused_shapes_match_the_compiled_list():
    src = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'sx_stream_launch.hpp')).read()
    body = re.search(r'#define SX_ROLLOUT_SHAPES\(X, \.\.\.\)((?:.*\\\n)*.*\n)', src).group(1)
    shapes = {tuple(map(int, t)) for t in re.findall(r'X\((\d+), (\d+), (\d+), __VA_ARGS__\)', body)}
    assert len(shapes) == body.count('X(')
    assert shapes == set(JUNK_FUSED_SHAPES)
