"""CPU: the multi-model entries of the feature-GP and MC-dropout families (sx_feat_model_table[_bytes],
sx_cem_rollout_feat_multi, sx_mlp_model_table[_bytes], sx_cem_rollout_mlp_multi): declarations, table sizes, argument
checks answered before any device access, and which solves MultiModelCemMpc / get_actions_multi fuse.  The models here
carry fake device pointers that no call below dereferences."""
import ctypes
import re
from pathlib import Path

import pytest

from safe_exploration_amd import _lib
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc
from safe_exploration_amd.safempc_cem import multi_solve_applies

ENTRIES = ('sx_feat_model_table_bytes', 'sx_feat_model_table', 'sx_cem_rollout_feat_multi',
           'sx_mlp_model_table_bytes', 'sx_mlp_model_table', 'sx_cem_rollout_mlp_multi')
HEADER = Path(__file__).resolve().parents[1] / 'include' / 'sx_amd.h'
FAKE = ctypes.c_void_p(0x1000)   # a non-null "device" pointer the checks reject before using it


def feat(n_s=2, n_u=1, layers=(8, 6), normalise=1, ptrs=True):
    m = _lib.SxFeatModel()
    m.n_s, m.n_u, m.n_layers, m.normalise = n_s, n_u, len(layers), normalise
    m.width[0] = n_s + n_u
    for i, w in enumerate(layers):
        m.width[i + 1] = w
    m.n_feat = layers[-1] if layers else n_s + n_u
    m.prelu = 0.25
    if ptrs:
        m.net = m.wbar = m.minv = 0x1000
    return m


def mlp(n_s=2, n_u=1, hidden=(16, 16), samples=11, predict_std=0, n_out=None):
    m = _lib.SxMlpModel()
    m.n_s, m.n_u, m.n_hidden = n_s, n_u, len(hidden)
    m.n_out = n_out if n_out is not None else (2 * n_s if predict_std else n_s)
    m.n_samples, m.predict_std = samples, predict_std
    m.width[0] = n_s + n_u
    for i, w in enumerate(hidden):
        m.width[i + 1] = w
    m.net = m.masks = 0x1000
    return m


def array(models):
    return (type(models[0]) * len(models))(*models)


def env(n_s=2, n_u=1):
    e = _lib.SxEnv()
    e.n_s, e.n_u, e.m = n_s, n_u, 4
    return e


# family -> (model factory, table-bytes entry, table entry, rollout entry, architecture variants that may not share a launch)
FAMILIES = {
    'feature': (feat, 'sx_feat_model_table_bytes', 'sx_feat_model_table', 'sx_cem_rollout_feat_multi',
                [dict(layers=(8,)), dict(layers=(8, 7)), dict(layers=(10, 6)), dict(layers=(8, 6, 6)), dict(normalise=0),
                 dict(layers=())]),
    'mlp': (mlp, 'sx_mlp_model_table_bytes', 'sx_mlp_model_table', 'sx_cem_rollout_mlp_multi',
            [dict(hidden=(16,)), dict(hidden=(16, 12)), dict(hidden=(24, 16)), dict(hidden=(16, 16, 16)),
             dict(samples=10), dict(predict_std=1), dict(n_out=3)]),
}


def test_entries_are_declared_exported_and_typed():
    header = HEADER.read_text()
    lib = _lib.lib()
    for name in ENTRIES:
        assert re.search(r'\b' + name + r'\(', header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_table_bytes_scale_with_the_problem_count(family):
    make, nbytes, *_ = FAMILIES[family]
    fn = getattr(_lib.lib(), nbytes)
    one = fn(array([make()]), 1)
    assert one > 0 and one % 8 == 0
    for E in (2, 3, 6, 8):
        assert fn(array([make() for _ in range(E)]), E) == E * one
    assert fn(array([make(4, 1), make(4, 1), make(4, 1)]), 3) == 3 * one   # (the entry's size does not depend on the shape)
    assert fn(array([make(2, 2)]), 1) == one


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_table_bytes_are_negative_where_one_launch_does_not_serve_the_models(family):
    make, nbytes, _, _, variants = FAMILIES[family]
    fn = getattr(_lib.lib(), nbytes)
    two = array([make(), make()])
    assert fn(two, 0) < 0 and fn(two, -2) < 0                                  # E <= 0
    assert fn(None, 2) < 0                                                     # null models
    assert fn(array([make(2, 1), make(2, 2)]), 2) < 0                         # (n_s, n_u) differ
    assert fn(array([make(2, 1), make(4, 1)]), 2) < 0
    assert fn(array([make(3, 2)]), 1) < 0                                     # (3, 2): no rollout kernel
    for v in variants:                                                         # one architecture field differs
        assert fn(array([make(**v)]), 1) > 0, v
        assert fn(array([make(), make(), make(**v)]), 3) < 0, v


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_table_entry_rejects_bad_arguments_before_any_device_access(family):
    make, _, table, _, variants = FAMILIES[family]
    fn = getattr(_lib.lib(), table)
    ok = array([make(), make()])
    assert fn(ok, 2, None, None) == _lib.SX_ERR_ARG                           # null table
    assert fn(None, 2, FAKE, None) == _lib.SX_ERR_ARG                         # null models
    assert fn(ok, 0, FAKE, None) == _lib.SX_ERR_ARG                           # E <= 0
    assert fn(array([make(2, 1), make(2, 2)]), 2, FAKE, None) == _lib.SX_ERR_ARG
    for v in variants:
        assert fn(array([make(), make(**v)]), 2, FAKE, None) == _lib.SX_ERR_UNSUPPORTED, v
    assert fn(array([make(3, 2)]), 1, FAKE, None) == _lib.SX_ERR_UNSUPPORTED
    if family == 'feature':
        assert fn(array([make(), make(ptrs=False)]), 2, FAKE, None) == _lib.SX_ERR_ARG   # a model without buffers


def _rollout(fn, models, E, e, P=37, H=5, table=FAKE, status=FAKE, noise=None, mean=None, std=None, x0=FAKE):
    return fn(models, table, ctypes.byref(e), E, P, H, x0, None, mean, std, noise, FAKE, None, None, FAKE, FAKE, status, None)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_rollout_entry_rejects_bad_arguments_before_any_device_access(family):
    make, _, _, rollout, variants = FAMILIES[family]
    fn = getattr(_lib.lib(), rollout)
    ok, e = array([make(), make(), make()]), env()
    assert _rollout(fn, ok, 3, e, table=None) == _lib.SX_ERR_ARG              # null table
    assert _rollout(fn, None, 3, e) == _lib.SX_ERR_ARG                        # null models
    assert _rollout(fn, ok, 3, e, status=None) == _lib.SX_ERR_ARG             # null status words
    assert _rollout(fn, ok, 3, e, x0=None) == _lib.SX_ERR_ARG
    assert _rollout(fn, ok, 0, e) == _lib.SX_ERR_ARG                          # E <= 0
    assert _rollout(fn, ok, -1, e) == _lib.SX_ERR_ARG
    assert _rollout(fn, ok, 3, e, P=0) == _lib.SX_ERR_ARG
    assert _rollout(fn, ok, 3, e, H=0) == _lib.SX_ERR_ARG
    assert _rollout(fn, ok, 3, e, noise=FAKE) == _lib.SX_ERR_ARG              # noise without a distribution
    assert _rollout(fn, array([make(), make(2, 2), make()]), 3, e) == _lib.SX_ERR_ARG   # models differ
    assert _rollout(fn, ok, 3, env(2, 2)) == _lib.SX_ERR_ARG                 # models vs env
    assert _rollout(fn, ok, 3, env(4, 1)) == _lib.SX_ERR_ARG
    for v in variants:                                                         # architectures differ: before any launch
        assert _rollout(fn, array([make(), make(**v), make()]), 3, e) == _lib.SX_ERR_UNSUPPORTED, v
    assert _rollout(fn, array([make(3, 2)]), 1, env(3, 2)) == _lib.SX_ERR_UNSUPPORTED   # no kernel for (3, 2)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_rollout_entry_answers_argument_errors_before_unsupported_cases(family):
    make, _, _, rollout, variants = FAMILIES[family]
    fn = getattr(_lib.lib(), rollout)
    ok, mixed = array([make(), make(), make()]), array([make(), make(**variants[0]), make()])
    assert _rollout(fn, mixed, 3, env(), x0=None) == _lib.SX_ERR_ARG
    assert _rollout(fn, mixed, 3, env(), noise=FAKE, mean=FAKE) == _lib.SX_ERR_ARG
    assert _rollout(fn, array([make(3, 2)]), 1, env(3, 2), P=0) == _lib.SX_ERR_ARG
    for m_bad in (0, _lib.SX_MAX_M + 1):                                # constraint rows outside 1 .. SX_MAX_M
        e = env()
        e.m = m_bad
        assert _rollout(fn, ok, 3, e) == _lib.SX_ERR_UNSUPPORTED
        assert _rollout(fn, ok, 3, e, status=None) == _lib.SX_ERR_ARG
        assert _rollout(fn, mixed, 3, e) == _lib.SX_ERR_UNSUPPORTED


class Model:
    """A stand-in for a model of the given kernel_family with a fixed struct (what fused_applies reads)."""

    def __init__(self, family, struct, n_s=2, n_u=1):
        self.kernel_family, self.num_states, self.num_actions = family, n_s, n_u
        self.feat_model = self.mlp_model = struct


def _multi(models):
    return MultiModelCemMpc(models, env(), 5, 64, 8, 3, device='cpu')


def test_fused_applies_for_one_family_and_one_architecture():
    assert _multi([Model('feature', feat()) for _ in range(4)]).fused_applies()
    assert _multi([Model('feature', feat(layers=())) for _ in range(3)]).fused_applies()        # 'linear'
    assert _multi([Model('mlp', mlp()) for _ in range(5)]).fused_applies()
    assert _multi([Model('mlp', mlp(hidden=(64, 64), samples=30)) for _ in range(6)]).fused_applies()
    assert _multi([Model('mlp', mlp(hidden=(24,), samples=6, predict_std=1)) for _ in range(3)]).fused_applies()


def test_fused_applies_is_false_for_mixed_families_architectures_and_junk_wrappers():
    assert not _multi([Model('feature', feat()), Model('mlp', mlp())]).fused_applies()
    assert not _multi([Model('feature', feat()), Model('feature', feat(layers=(8, 7)))]).fused_applies()
    assert not _multi([Model('mlp', mlp()), Model('mlp', mlp(samples=12))]).fused_applies()
    assert not _multi([Model('feature_junk', feat()), Model('feature_junk', feat())]).fused_applies()
    assert not _multi([Model('mlp_junk', mlp()), Model('mlp_junk', mlp())]).fused_applies()
    assert not _multi([Model('stepwise', None), Model('stepwise', None)]).fused_applies()


def _mpcs(models):
    return [FusedCemMpc(m, env(), 5, 64, 8, 3, device='cpu', seed=e) for e, m in enumerate(models)]


def test_get_actions_multi_dispatch():
    """multi_solve_applies: get_actions_multi's choice between one MultiModelCemMpc and a solve per solver."""
    assert multi_solve_applies(_mpcs([Model('feature', feat()) for _ in range(3)]))
    assert multi_solve_applies(_mpcs([Model('mlp', mlp()) for _ in range(3)]))
    # (a differing architecture goes to MultiModelCemMpc, whose fused_applies then answers: one solve per model)
    mixed_arch = _mpcs([Model('mlp', mlp()), Model('mlp', mlp(hidden=(16,)))])
    assert multi_solve_applies(mixed_arch) and not MultiModelCemMpc.from_solvers(mixed_arch).fused_applies()
    assert not multi_solve_applies(_mpcs([Model('feature', feat()), Model('mlp', mlp())]))
    assert not multi_solve_applies(_mpcs([Model('feature_junk', feat()), Model('feature_junk', feat())]))
    assert not multi_solve_applies(_mpcs([Model('mlp_junk', mlp()), Model('mlp_junk', mlp())]))
    hooked = _mpcs([Model('feature', feat()) for _ in range(2)])
    hooked[1]._objective_hook = lambda *a: None
    assert not multi_solve_applies(hooked)
