"""CPU: the exact-GP rollout plan's answers through sx_cem_rollout_form / sx_cem_rollout_workspace_bytes (no device
access), and the compiled shape list (SX_ROLLOUT_SHAPES) against ssm_cem.JUNK_FUSED_SHAPES."""
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


def test_junk_fused_shapes_match_the_compiled_list():
    src = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'sx_stream_launch.hpp')).read()
    body = re.search(r'#define SX_ROLLOUT_SHAPES\(X, \.\.\.\)((?:.*\\\n)*.*\n)', src).group(1)
    shapes = {tuple(map(int, t)) for t in re.findall(r'X\((\d+), (\d+), (\d+), __VA_ARGS__\)', body)}
    assert len(shapes) == body.count('X(')
    assert shapes == set(JUNK_FUSED_SHAPES)
