"""CPU: the fused junk-dimension rollout over feature-space GPs and MC-dropout models, host side -- the C entry points
sx_cem_rollout_feat_junk / sx_cem_rollout_mlp_junk (declared, exported, argument checks that answer before any device
access), the shape list they are instantiated for, JunkDimensionsSSM's kernel family and query shift over REAL inner models
(FeatureGpCemSSM 'linear' / 'nn', McDropoutSSM, GalConcreteDropoutSSM, built on the CPU), and the kept-column MC-dropout
model against the padded one, evaluated in torch on CPU tensors."""
import ctypes
import functools
import os
import re

import pytest
import torch

from safe_exploration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sx_cem_rollout_feat_junk', 'sx_cem_rollout_mlp_junk')
# (n_s, n_u, s): the plain feature / MLP rollout shapes (s = 0) and every shape a padded inner model can be built for
FUSED = {(1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (2, 2, 0), (4, 2, 0),
         (1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 1)}


def test_model_junk_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'\bint ' + name + r'\(', header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)


def test_model_junk_shapes_match_the_instantiations():
    from safe_exploration_amd.ssm_cem.ssm_cem import JUNK_FUSED_SHAPES, JUNK_MODEL_FUSED_SHAPES
    src = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'sx_model_shapes.hpp')).read()
    block = src[src.index('#define SX_MODEL_JUNK_SHAPES'):]
    block = block[:block.index('\n\n') if '\n\n' in block else len(block)]
    block = block[:block.index('//')]
    shifted = {tuple(int(v) for v in m) for m in re.findall(r'X\((\d), (\d), (\d), __VA_ARGS__\)', block)}
    shift0 = {(ns, nu, 0) for (ns, nu, sh) in JUNK_FUSED_SHAPES if sh == 0}     # SX_DISPATCH's shapes
    assert shifted | shift0 == JUNK_MODEL_FUSED_SHAPES == FUSED


def _feat(n_s, n_u):
    m = _lib.SxFeatModel()
    m.n_s, m.n_u, m.n_feat, m.n_layers, m.normalise = n_s, n_u, n_s + n_u, 0, 0
    m.width[0] = n_s + n_u
    m.wbar, m.minv = 16, 16
    return m


def _mlp(n_s, n_u):
    m = _lib.SxMlpModel()
    m.n_s, m.n_u, m.n_hidden, m.n_out, m.n_samples, m.predict_std = n_s, n_u, 1, n_s, 4, 0
    m.width[0], m.width[1] = n_s + n_u, 8
    m.net, m.masks = 16, 16
    return m


def _env(n_s, n_u):
    env = _lib.SxEnv()
    env.n_s, env.n_u, env.m = n_s, n_u, 4
    return env


# non-null placeholders: every call below must be refused before anything is dereferenced
_P = ctypes.c_void_p(16)


def _call(entry, model, env, shift, E=1, x0=_P, actions=_P, status=_P, obj=_P):
    return getattr(_lib.lib(), entry)(ctypes.byref(model) if model is not None else None,
                                      ctypes.byref(env) if env is not None else None, shift, E, 16, 3, x0, None, None, None,
                                      None, actions, None, None, obj, _P, status, None)


@pytest.mark.parametrize('entry,make', [('sx_cem_rollout_feat_junk', _feat), ('sx_cem_rollout_mlp_junk', _mlp)])
def test_model_junk_entries_refuse_bad_shapes_without_a_gpu(entry, make):
    env = _env(2, 1)
    assert _call(entry, make(2, 2), env, 2) == _lib.SX_ERR_ARG          # shift > env n_u
    assert _call(entry, make(2, 2), env, -1) == _lib.SX_ERR_ARG
    assert _call(entry, make(2, 2), env, 0) == _lib.SX_ERR_ARG          # model n_u != env n_u + shift
    assert _call(entry, make(3, 2), env, 1) == _lib.SX_ERR_ARG          # n_s differs
    assert _call(entry, make(2, 5), _env(2, 2), 3) == _lib.SX_ERR_ARG   # n_s + n_u > SX_MAX_D, shift > n_u
    assert _call(entry, make(2, 3), _env(2, 3), 0) == _lib.SX_ERR_ARG   # the plain model keeps n_u <= SX_MAX_NU
    assert _call(entry, make(2, 2), env, 1, E=0) == _lib.SX_ERR_ARG
    assert _call(entry, None, env, 1) == _lib.SX_ERR_ARG
    assert _call(entry, make(2, 2), None, 1) == _lib.SX_ERR_ARG
    # consistent, but no kernel for (n_s, n_u, s) = (1, 2, 1): the plain (1, 2) model has none either
    assert _call(entry, make(1, 3), _env(1, 2), 1) == _lib.SX_ERR_UNSUPPORTED


@pytest.mark.parametrize('entry,make', [('sx_cem_rollout_feat_junk', _feat), ('sx_cem_rollout_mlp_junk', _mlp)])
def test_model_junk_entries_refuse_null_buffers_without_a_gpu(entry, make):
    env = _env(2, 1)
    assert _call(entry, make(2, 2), env, 1, x0=None) == _lib.SX_ERR_ARG
    assert _call(entry, make(2, 2), env, 1, actions=None) == _lib.SX_ERR_ARG
    assert _call(entry, make(2, 2), env, 1, status=None) == _lib.SX_ERR_ARG
    assert _call(entry, make(2, 2), env, 1, obj=None) == _lib.SX_ERR_ARG
    bad = make(2, 2)
    if entry == 'sx_cem_rollout_feat_junk':
        bad.wbar = None
    else:
        bad.masks = None
    assert _call(entry, bad, env, 1) == _lib.SX_ERR_ARG


@pytest.mark.parametrize('entry,make', [('sx_cem_rollout_feat_junk', _feat), ('sx_cem_rollout_mlp_junk', _mlp)])
def test_model_junk_entries_refuse_bad_sizes_and_answer_the_constraint_count_last_without_a_gpu(entry, make):
    model, env = make(2, 2), _env(2, 1)
    fn = getattr(_lib.lib(), entry)

    def call(P=16, H=3, x0=_P, mean=None, std=None, noise=None, con=_P):
        return fn(ctypes.byref(model), ctypes.byref(env), 1, 1, P, H, x0, None, mean, std, noise, _P, None, None, _P, con, _P,
                  None)

    assert call(P=0) == _lib.SX_ERR_ARG
    assert call(H=0) == _lib.SX_ERR_ARG
    assert call(con=None) == _lib.SX_ERR_ARG
    assert call(noise=_P, mean=_P) == _lib.SX_ERR_ARG                   # noise without a whole distribution
    if entry == 'sx_cem_rollout_feat_junk':
        model.minv = None
        assert call() == _lib.SX_ERR_ARG
        model.minv = 16
    for m_bad in (0, _lib.SX_MAX_M + 1):                                # constraint rows outside 1 .. SX_MAX_M
        env.m = m_bad
        assert call() == _lib.SX_ERR_UNSUPPORTED
        assert call(x0=None) == _lib.SX_ERR_ARG                         # argument errors answer first
        assert call(noise=_P) == _lib.SX_ERR_ARG


class FeatConf:
    exact_gp_training_iterations = 0
    nn_kernel_layers = [6, 5]
    device = 'cpu'


class DropoutConf:
    mc_dropout_training_iterations = 0
    mc_dropout_hidden_features = [8, 6]
    mc_dropout_num_samples = 5
    mc_dropout_predict_std = False
    mc_dropout_reinitialize = False
    mc_dropout_type = 'fixed'
    mc_dropout_concrete_initial_probability = 0.1
    mc_dropout_fixed_probability = 0.2
    mc_dropout_on_input = True
    mc_dropout_lengthscale = 1e-4
    device = 'cpu'


def _constructor(kind):
    from safe_exploration_amd.ssm_cem.dropout_ssm_cem import McDropoutSSM
    from safe_exploration_amd.ssm_cem.gal_concrete_dropout import GalConcreteDropoutSSM
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    if kind in ('linear', 'nn'):
        return functools.partial(GpCemSSM, type('C', (FeatConf,), {'exact_gp_kernel': kind})())
    if kind == 'mc_dropout':
        return functools.partial(McDropoutSSM, type('C', (DropoutConf,), {'mc_dropout_type': 'concrete',
                                                                           'mc_dropout_predict_std': True})())
    return functools.partial(GalConcreteDropoutSSM, type('C', (DropoutConf,), {
        'mc_dropout_type': 'concrete', 'mc_dropout_predict_std': True, 'mc_dropout_hidden_features': [7, 5]})())


def _wrap(kind, n_s, n_u, js, ja):
    from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM
    return JunkDimensionsSSM(_constructor(kind), state_dimen=n_s, action_dimen=n_u, junk_states=js, junk_actions=ja)


@pytest.mark.parametrize('kind', ['linear', 'nn', 'mc_dropout', 'gal'])
@pytest.mark.parametrize('n_s', [1, 2, 3, 4])
@pytest.mark.parametrize('n_u', [1, 2])
def test_kernel_family_and_query_shift_of_real_inner_models(kind, n_s, n_u):
    family = 'feature_junk' if kind in ('linear', 'nn') else 'mlp_junk'
    for js in range(0, 5 - n_s):
        for ja in range(0, 3 - n_u):
            ssm = _wrap(kind, n_s, n_u, js, ja)
            s = min(js, n_u)
            assert ssm.query_shift == s and ssm.folded_columns is None
            assert len(ssm._kept_columns()) == n_s + n_u + s
            # (1, 2) has no plain feature / MLP rollout instantiation, and hence no shifted one either
            assert ssm.kernel_family == (family if (n_s, n_u, s) in FUSED else 'stepwise'), (js, ja)


@pytest.mark.parametrize('kind', ['linear', 'nn', 'mc_dropout'])
def test_shapes_beyond_the_inner_limits_stay_out(kind):
    """Padded sizes beyond the inner model's limits: feature GPs and MC-dropout models do not fold, the wrapper refuses."""
    with pytest.raises(ValueError):
        _wrap(kind, 2, 1, 3, 0)
    with pytest.raises(ValueError):
        _wrap(kind, 2, 2, 0, 1)
    assert _wrap(kind, 1, 2, 2, 0).kernel_family == 'stepwise'
    assert _wrap(kind, 3, 2, 0, 0).kernel_family == 'stepwise'


def _ensemble(net_buf, masks, widths, n_out, S, z):
    """mean over the members of the ReLU network (csrc/sx_mlp.hpp's model) in torch: z [N x D] -> [N x n_out]."""
    off, moff, a = 0, 0, z.unsqueeze(0).expand(S, -1, -1) * masks[:, None, :widths[0]]
    moff = widths[0]
    dims = list(widths) + [n_out]
    for l in range(1, len(dims)):
        win, wout = dims[l - 1], dims[l]
        W = net_buf[off:off + wout * win].view(wout, win)
        b = net_buf[off + wout * win:off + wout * win + wout]
        off += wout * win + wout
        a = a @ W.t() + b
        if l < len(dims) - 1:
            a = torch.relu(a) * masks[:, None, moff:moff + wout]
            moff += wout
    return a


@pytest.mark.parametrize('kind', ['mc_dropout', 'gal'])
@pytest.mark.parametrize('n_s,n_u,js,ja', [(2, 1, 1, 0), (2, 1, 2, 1), (2, 2, 2, 0), (1, 1, 3, 1), (3, 2, 1, 0)])
def test_kept_column_mlp_view_equals_the_padded_ensemble_on_cpu(kind, n_s, n_u, js, ja):
    ssm = _wrap(kind, n_s, n_u, js, ja)
    inner = ssm._ssm
    assert ssm.kernel_family == 'mlp_junk'
    view = ssm.real_output_view()
    assert ssm.real_output_view() is view                                 # built once per device model
    s, D = ssm.query_shift, n_s + n_u + ssm.query_shift
    m = view.mlp_model
    assert (m.n_s, m.n_u, m.width[0]) == (n_s, n_u + s, D)
    g = torch.Generator().manual_seed(3)
    N = 7
    x, u = torch.randn(N, n_s, generator=g, dtype=torch.float64), torch.randn(N, n_u, generator=g, dtype=torch.float64)
    pad = torch.zeros(N, n_s + js + n_u + ja, dtype=torch.float64)       # the wrapper's query [x, 0, u, 0]
    pad[:, :n_s], pad[:, n_s + js:n_s + js + n_u] = x, u
    kept = torch.cat((x, torch.zeros(N, s, dtype=torch.float64), u), 1)  # the view's query [x, 0_s, u]
    im, S = inner.mlp_model, inner.mlp_model.n_samples
    widths_pad = [im.width[i] for i in range(im.n_hidden + 1)]
    net_pad, mask_pad = inner._buffers
    out_pad = _ensemble(net_pad, mask_pad, widths_pad, im.n_out, S, pad)
    widths = [m.width[i] for i in range(m.n_hidden + 1)]
    out = _ensemble(view._buffers[0], view._buffers[1], widths, m.n_out, S, kept)
    n_s_pad = n_s + js
    rows = list(range(n_s)) + (list(range(n_s_pad, n_s_pad + n_s)) if m.predict_std else [])
    assert m.n_out == len(rows) and m.predict_std == im.predict_std
    torch.testing.assert_close(out, out_pad[:, :, rows], rtol=0, atol=1e-12)
    # a new ensemble (re-frozen masks) is a new device model: the view follows
    inner._freeze()
    assert ssm.real_output_view() is not view
