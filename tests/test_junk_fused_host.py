"""CPU: the fused junk-dimension rollout's host side -- the C entry points sx_cem_rollout_junk /
sx_cem_rollout_elites_junk (declared, exported, argument checks that answer before any device access) and
JunkDimensionsSSM's kept columns, query shift, kernel family and lazily built real-output model (mock inner models)."""
import ctypes
import os
import re
from unittest import mock

import pytest
import torch

from safe_exploration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sx_cem_rollout_junk', 'sx_cem_rollout_elites_junk')


def test_junk_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'\bint ' + name + r'\(', header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)


def _structs(n_s, n_u_model, n_u_env):
    model, env = _lib.SxGpModel(), _lib.SxEnv()
    model.n_s, model.n_u, model.n_train, model.n_pad = n_s, n_u_model, 10, 16
    env.n_s, env.n_u, env.m = n_s, n_u_env, 4
    return model, env


# non-null placeholders: every call below must be refused before anything is dereferenced
_P = ctypes.c_void_p(16)


def _rollout(model, env, shift, x0=_P, actions=_P, status=_P):
    return _lib.lib().sx_cem_rollout_junk(ctypes.byref(model) if model is not None else None,
                                          ctypes.byref(env) if env is not None else None, shift, 1, 16, 3, x0, None,
                                          None, None, None, actions, None, None, _P, _P, status, None, 0, None)


def _elites(model, env, shift, rows=_P, noise=_P):
    return _lib.lib().sx_cem_rollout_elites_junk(ctypes.byref(model) if model is not None else None,
                                                 ctypes.byref(env) if env is not None else None, shift, 1, 16, 3, _P, None,
                                                 rows, 4, noise, _P, None, None, _P, _P, _P, None, None, None)


@pytest.mark.parametrize('call', [_rollout, _elites])
def test_junk_entries_refuse_bad_shapes_without_a_gpu(call):
    model, env = _structs(2, 2, 1)
    assert call(model, env, 2) == _lib.SX_ERR_ARG                       # shift > env n_u
    assert call(model, env, -1) == _lib.SX_ERR_ARG
    assert call(model, env, 0) == _lib.SX_ERR_ARG                       # model n_u != env n_u + shift
    bad_ns, env_ns = _structs(3, 2, 1)
    env_ns.n_s = 2
    assert call(bad_ns, env_ns, 1) == _lib.SX_ERR_ARG                   # n_s differs
    wide, env2 = _structs(2, 4, 2)
    assert call(wide, env2, 1) == _lib.SX_ERR_ARG                       # 4 != 2 + 1
    assert call(None, env, 1) == _lib.SX_ERR_ARG
    assert call(model, None, 1) == _lib.SX_ERR_ARG


def test_junk_entries_refuse_null_buffers_without_a_gpu():
    model, env = _structs(2, 2, 1)
    assert _rollout(model, env, 1, x0=None) == _lib.SX_ERR_ARG
    assert _rollout(model, env, 1, actions=None) == _lib.SX_ERR_ARG
    assert _rollout(model, env, 1, status=None) == _lib.SX_ERR_ARG
    assert _elites(model, env, 1, rows=None) == _lib.SX_ERR_ARG
    assert _elites(model, env, 1, noise=None) == _lib.SX_ERR_ARG


def test_junk_entries_refuse_bad_sizes_and_answer_the_constraint_count_last_without_a_gpu():
    model, env = _structs(2, 2, 1)
    lib, m, e = _lib.lib(), ctypes.byref(model), ctypes.byref(env)

    def roll(E=1, P=16, H=3, x0=_P, mean=None, std=None, noise=None, con=_P):
        return lib.sx_cem_rollout_junk(m, e, 1, E, P, H, x0, None, mean, std, noise, _P, None, None, _P, con, _P, None, 0,
                                       None)

    def elites(E=1, P=16, H=3, x0=_P, k=4, mean_out=None, std_out=None):
        return lib.sx_cem_rollout_elites_junk(m, e, 1, E, P, H, x0, None, _P, k, _P, _P, None, None, _P, _P, _P, mean_out,
                                              std_out, None)

    for call in (roll, elites):
        assert call(E=0) == _lib.SX_ERR_ARG
        assert call(P=0) == _lib.SX_ERR_ARG
        assert call(H=-1) == _lib.SX_ERR_ARG
    assert roll(con=None) == _lib.SX_ERR_ARG
    assert roll(noise=_P, mean=_P) == _lib.SX_ERR_ARG                   # noise without a whole distribution
    assert roll(noise=_P, std=_P) == _lib.SX_ERR_ARG
    assert elites(k=0) == _lib.SX_ERR_ARG
    assert elites(mean_out=_P) == _lib.SX_ERR_ARG                       # one refit output without the other
    for m_bad in (0, _lib.SX_MAX_M + 1):                                # constraint rows outside 1 .. SX_MAX_M
        env.m = m_bad
        assert roll() == _lib.SX_ERR_UNSUPPORTED
        assert elites() == _lib.SX_ERR_UNSUPPORTED
        assert roll(x0=None) == _lib.SX_ERR_ARG                         # argument errors answer first
        assert elites(k=0) == _lib.SX_ERR_ARG


def _inner(family):
    inner = mock.Mock()
    inner.kernel_family = family
    return inner


def _wrapper(n_s, n_u, js, ja, family='rbf', limit=(4, 2)):
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    calls = []

    def constructor(state_dimen, action_dimen):
        calls.append((state_dimen, action_dimen))
        if state_dimen > limit[0] or action_dimen > limit[1]:
            raise ValueError('beyond the compiled limits')
        return _inner(family)

    return JunkDimensionsSSM(constructor, state_dimen=n_s, action_dimen=n_u, junk_states=js, junk_actions=ja), calls


@pytest.mark.parametrize('n_s', [1, 2, 3, 4])
@pytest.mark.parametrize('n_u', [1, 2])
@pytest.mark.parametrize('js', [0, 1, 2, 3, 5])
@pytest.mark.parametrize('ja', [0, 1, 2])
def test_kept_columns_query_shift_and_kernel_family(n_s, n_u, js, ja):
    try:
        ssm, calls = _wrapper(n_s, n_u, js, ja)
    except ValueError:
        # neither the padded nor the folded sizes fit the inner model: the wrapper refuses, as before
        assert n_s + js > 4 or n_u + ja > 2
        assert n_u + min(js, n_u) > 2
        return
    s = min(js, n_u)
    kept = ssm._kept_columns()
    assert kept == tuple(sorted(set(range(n_s + n_u)) | set(range(n_s + js, n_s + js + n_u))))
    assert len(kept) == n_s + n_u + s and ssm.query_shift == s
    # construction calls and folding are those of the wrapper without the fused path
    assert calls[0] == (n_s + js, n_u + ja)
    if ssm.folded_columns is not None:
        assert ssm.folded_columns == kept and calls[1] == (n_s, n_u + s)
    # the fused shapes: sx_cem_rollout's for s = 0, the query-shifted instantiations (D = n_s + n_u + s <= 6) otherwise
    fused = {(1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (2, 2, 0), (4, 2, 0),
             (1, 1, 1), (2, 1, 1), (3, 1, 1), (4, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 1)}
    assert ssm.kernel_family == ('rbf_junk' if (n_s, n_u, s) in fused else 'stepwise')


@pytest.mark.parametrize('family', ['feature', 'mlp', 'stepwise'])
def test_other_inner_models_stay_stepwise(family):
    ssm, _ = _wrapper(2, 1, 2, 1, family=family)
    assert ssm.kernel_family == 'stepwise'


def test_wide_shapes_stay_stepwise():
    ssm, _ = _wrapper(4, 2, 1, 0, limit=(5, 2))       # D = 4 + 2 + 1 > 6
    assert ssm.query_shift == 1 and ssm.kernel_family == 'stepwise'
    ssm, _ = _wrapper(4, 2, 0, 0)                     # no junk state: the plain (4, 2) rollout
    assert ssm.query_shift == 0 and ssm.kernel_family == 'rbf_junk'


def test_real_output_view_is_built_lazily_from_the_sliced_hyper_parameters():
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    n_s, n_u, js, ja = 2, 1, 2, 1
    d_pad = n_s + js + n_u + ja
    inner = _inner('rbf')
    raw_ls = torch.arange((n_s + js) * d_pad, dtype=torch.float64).view(n_s + js, d_pad)
    inner.state_dict.return_value = {
        'gp_model': {'raw_lengthscale': raw_ls, 'raw_outputscale': torch.tensor([1., 2., 3., 4.], dtype=torch.float64)},
        'gp_likelihood': {'raw_noise': torch.tensor([5., 6., 7., 8.], dtype=torch.float64), 'noise_floor': torch.tensor(1e-4)}}
    views = []

    def constructor(state_dimen, action_dimen, **kw):
        if not kw:
            return inner
        view = mock.Mock()
        views.append(((state_dimen, action_dimen), kw, view))
        return view

    ssm = JunkDimensionsSSM(constructor, state_dimen=n_s, action_dimen=n_u, junk_states=js, junk_actions=ja)
    assert not views and ssm.folded_columns is None and ssm.kernel_family == 'rbf_junk'
    x = torch.tensor([[1., 2., 3.], [4., 5., 6.]], dtype=torch.float64)
    y = torch.ones((2, 2), dtype=torch.float64)
    ssm.update_model(x, y, replace_old=True)
    assert not views                                                  # nothing is built before the solver asks
    inner.device_model = object()
    view = ssm.real_output_view()
    assert len(views) == 1 and views[0][:2] == ((2, 2), {'wide_inputs': True})
    state = view.load_state_dict.call_args[0][0]
    kept = [0, 1, 2, 4]                                               # [x, u(train), u(query)] of [x, j, j, u, j]
    assert torch.equal(state['gp_model']['raw_lengthscale'], raw_ls[:2][:, kept])
    assert torch.equal(state['gp_model']['raw_outputscale'], torch.tensor([1., 2.], dtype=torch.float64))
    assert torch.equal(state['gp_likelihood']['raw_noise'], torch.tensor([5., 6.], dtype=torch.float64))
    vx, vy = view.update_model.call_args[0][:2]
    assert torch.equal(vx, torch.tensor([[1., 2., 3., 0.], [4., 5., 6., 0.]], dtype=torch.float64))   # [x, u, 0_s]
    assert torch.equal(vy, y) and view.update_model.call_args[1] == {'opt_hyp': False, 'replace_old': True}
    assert ssm.real_output_view() is view and len(views) == 1        # unchanged inner model: kept
    inner.device_model = object()                                     # new data or hyper-parameters: rebuilt
    assert ssm.real_output_view() is not view and len(views) == 2


def test_folded_wrapper_view_is_the_inner_model():
    ssm, calls = _wrapper(2, 1, 5, 0)
    assert ssm.folded_columns == (0, 1, 2, 7) and ssm.query_shift == 1 and ssm.kernel_family == 'rbf_junk'
    assert ssm.real_output_view() is ssm._ssm and calls == [(7, 1), (2, 2)]
