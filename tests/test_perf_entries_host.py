"""CPU: the argument checks the six performance-rollout entries have in common -- sx_cem_perf_rollout[_multi],
sx_cem_perf_rollout_var[_multi], sx_cem_perf_rollout_taylor[_multi] -- as one table of refusals per entry, the order of the
checks where two faults meet, and the four form queries past the largest (n_s, n_u).  Every call is answered before any
device access (the pointers are the fake 16).  The expected codes are literals, recorded from the library as it was before
the entries shared their checks."""
import ctypes
from collections import namedtuple

import pytest

from safe_exploration_amd import _lib
from test_perf_multi_host import ABS, VAR, _env, _model, _models

ARG, UNSUPPORTED = _lib.SX_ERR_ARG, _lib.SX_ERR_UNSUPPORTED
SX_MAX_NS, SX_MAX_NU, SX_MAX_M = 4, 2, 16

# multi: E models and a device table | second: the pointer behind the model(s) (alpha, or the table) | outs: the optional
# output pointers | packed: needs the model of sx_gp_pack | taylor: takes terminal_safety
Entry = namedtuple('Entry', 'multi second outs packed taylor')
ENTRIES = {
    'sx_cem_perf_rollout': Entry(False, True, 1, False, False),
    'sx_cem_perf_rollout_multi': Entry(True, True, 1, False, False),
    'sx_cem_perf_rollout_var': Entry(False, False, 2, True, False),
    'sx_cem_perf_rollout_var_multi': Entry(True, True, 2, True, False),
    'sx_cem_perf_rollout_taylor': Entry(False, False, 3, True, True),
    'sx_cem_perf_rollout_taylor_multi': Entry(True, True, 3, True, True),
}
MEAN_ONLY = [name for name, e in ENTRIES.items() if not e.packed]
PACKED = [name for name, e in ENTRIES.items() if e.packed]
TAYLOR = [name for name, e in ENTRIES.items() if e.taylor]
FORMS = ['sx_cem_perf_rollout_var_form', 'sx_cem_perf_rollout_var_multi_form', 'sx_cem_perf_rollout_taylor_form',
         'sx_cem_perf_rollout_taylor_multi_form']


def _call(entry, *, model=None, env=None, models=16, second=16, no_env=False, E=2, P=4, H=5, n_perf=8, r=1, x0=16, safe=16,
          mean=16, std=16, noise=16, rows=16, obj=16, con=16, status=16, terminal=0):
    """One call of `entry` over two models built by _model(**model) (the first of them for a single-model entry) and
    _env(**env); `models=None`, `second=None`, `no_env` pass a null pointer in their place."""
    kind = ENTRIES[entry]
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    ms = [_model(**(model or {})), _model(**(model or {}))]
    sx_env = _env(**{k: v for k, v in (env or {}).items() if k != 'm'})
    if env and 'm' in env:
        sx_env.m = env['m']
    first = None if models is None else _models(*ms) if kind.multi else ctypes.byref(ms[0])
    head = (first,) + ((p(second),) if kind.second else ()) + (None if no_env else ctypes.byref(sx_env),)
    outs = (None,) * kind.outs + ((terminal,) if kind.taylor else ())
    return getattr(_lib.lib(), entry)(*head, E, P, H, n_perf, r, p(x0), p(safe), p(mean), p(std), p(noise), p(rows), p(obj),
                                      p(con), *outs, p(status), None)


UNCOMPILED = dict(model=dict(n_s=3, n_u=2), env=dict(n_s=3, n_u=2))     # a shape of the ABI without a rollout kernel

# (what is wrong, the call, the code): refused alike by all six entries
COMMON = [
    ('models null', dict(models=None), ARG),
    ('env null', dict(no_env=True), ARG),
    ('x0 null', dict(x0=None), ARG),
    ('safe_actions null', dict(safe=None), ARG),
    ('rows null', dict(rows=None), ARG),
    ('obj_cost null', dict(obj=None), ARG),
    ('con_cost null', dict(con=None), ARG),
    ('status null', dict(status=None), ARG),
    ('E = 0', dict(E=0), ARG),
    ('P = 0', dict(P=0), ARG),
    ('H = 0', dict(H=0), ARG),
    ('r = 0', dict(r=0), ARG),
    ('r = H + 1', dict(r=6), ARG),
    ('n_perf = r', dict(n_perf=3, r=3), ARG),
    ('tail_noise without tail_mean', dict(mean=None), ARG),
    ('tail_noise without tail_std', dict(std=None), ARG),
    ('model and env disagree on the shape', dict(model=dict(n_s=2, n_u=2)), ARG),
    ('n_train = 0', dict(model=dict(n_train=0)), ARG),
    ('obj_mode = 7', dict(env=dict(obj_mode=7)), ARG),
    # each fault of the pairs below alone, where all entries answer it alike
    ('an uncompiled shape', UNCOMPILED, UNSUPPORTED),
]


@pytest.mark.parametrize('what,kw,code', COMMON, ids=[row[0] for row in COMMON])
@pytest.mark.parametrize('entry', list(ENTRIES))
def test_common_refusals(entry, what, kw, code):
    assert _call(entry, **kw) == code


@pytest.mark.parametrize('entry', [name for name, e in ENTRIES.items() if e.second])
def test_the_second_pointer_is_required(entry):
    """alpha of the single-model mean-only entry, the device table of the multi-model ones"""
    assert _call(entry, second=None) == ARG


# ---- the order of the checks: two faults in one call --------------------------------------------------------------------------
@pytest.mark.parametrize('null', ['models', 'x0', 'status'])
@pytest.mark.parametrize('entry', list(ENTRIES))
def test_a_null_pointer_comes_before_an_uncompiled_shape(entry, null):
    assert _call(entry, **UNCOMPILED, **{null: None}) == ARG


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_an_unknown_objective_comes_before_an_uncompiled_shape(entry):
    assert _call(entry, model=UNCOMPILED['model'], env=dict(n_s=3, n_u=2, obj_mode=7)) == ARG


@pytest.mark.parametrize('entry', MEAN_ONLY)
def test_mean_only_entries_answer_the_variance_objective_unsupported(entry):
    assert _call(entry, env=dict(obj_mode=VAR)) == UNSUPPORTED
    assert _call(entry, model=UNCOMPILED['model'], env=dict(n_s=3, n_u=2, obj_mode=VAR)) == UNSUPPORTED
    assert _call(entry, env=dict(obj_mode=VAR), x0=None) == ARG            # ... after the pointers
    assert _call(entry, env=dict(obj_mode=VAR), model=dict(n_train=0)) == ARG   # ... and after the models


@pytest.mark.parametrize('obj_mode', [ABS, VAR])
@pytest.mark.parametrize('entry', PACKED)
def test_an_unpacked_model_comes_before_a_training_set_without_a_form(entry, obj_mode):
    env = dict(obj_mode=obj_mode)
    assert _model(n_train=1100).n_pad > 1024
    assert _call(entry, env=env, model=dict(n_train=1100)) == UNSUPPORTED       # packed: no form, before any launch
    assert _call(entry, env=env, model=dict(packed=False)) == ARG
    assert _call(entry, env=env, model=dict(n_train=1100, packed=False)) == ARG


@pytest.mark.parametrize('entry', TAYLOR)
def test_taylor_entries_check_terminal_safety_then_the_polytope_rows(entry):
    assert _call(entry, env=dict(m=SX_MAX_M + 1)) == UNSUPPORTED
    assert _call(entry, env=dict(m=SX_MAX_M + 1), terminal=1) == UNSUPPORTED
    assert _call(entry, terminal=1, n_perf=6) == ARG                               # n_perf < H + 2
    assert _call(entry, env=dict(m=SX_MAX_M + 1), terminal=1, n_perf=6) == ARG     # ... first
    assert _call(entry, env=dict(m=0), terminal=1) == ARG and _call(entry, env=dict(m=-1)) == ARG
    assert _call(entry, env=dict(m=SX_MAX_M + 1, obj_mode=7)) == ARG               # obj_mode before m
    assert _call(entry, env=dict(m=SX_MAX_M + 1), model=dict(packed=False)) == ARG
    # m is checked before the form: too many rows and no form answer alike, a negative m does not
    assert _call(entry, env=dict(m=-1), model=dict(n_train=1100)) == ARG


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_a_shape_past_the_largest_of_the_abi(entry):
    """Models and env agree on n_s = SX_MAX_NS + 1.  The entries that bound the shape themselves call it an argument error;
    the single-model mean-only and variance entries leave it to the dispatch, which has no kernel for it."""
    m = dict(n_train=36)
    ms = [_model(**m), _model(**m)]
    env = _env()
    for x in ms + [env]:
        x.n_s = SX_MAX_NS + 1
    kind = ENTRIES[entry]
    p = ctypes.c_void_p(16)
    head = (_models(*ms) if kind.multi else ctypes.byref(ms[0]),) + ((p,) if kind.second else ()) + (ctypes.byref(env),)
    outs = (None,) * kind.outs + ((0,) if kind.taylor else ())
    code = getattr(_lib.lib(), entry)(*head, 2, 4, 5, 8, 1, *([p] * 8), *outs, p, None)
    assert code == (UNSUPPORTED if entry in ('sx_cem_perf_rollout', 'sx_cem_perf_rollout_var') else ARG)


# ---- the form queries past the largest shape ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_s,n_u', [(SX_MAX_NS + 1, 1), (2, SX_MAX_NU + 1), (SX_MAX_NS + 1, SX_MAX_NU + 1)])
@pytest.mark.parametrize('form', FORMS)
def test_form_queries_refuse_a_shape_past_the_largest(form, n_s, n_u):
    m = _model(n_train=36)           # a packed model whose padding also holds the rows of the larger shape
    m.n_s, m.n_u = n_s, n_u
    assert m.n_pad % 16 == 0 and m.n_pad > m.n_train + n_s + n_u
    lib = _lib.lib()
    for n_perf in (2, 8):
        if form.endswith('_multi_form'):
            assert int(getattr(lib, form)(_models(m, m), 2, n_perf)) == -1
        else:
            assert int(getattr(lib, form)(ctypes.byref(m), n_perf)) == -1
    ok = _model(n_train=36)          # the same model at a compiled shape has a form
    assert int(getattr(lib, form)(*((_models(ok, ok), 2) if form.endswith('_multi_form') else (ctypes.byref(ok),)), 8)) == 0


# ---- the wrappers: a fresh device table lives until the launch ------------------------------------------------------------------
@pytest.mark.parametrize('wrapper,kw', [('cem_perf_rollout_multi', dict(variance=False)),
                                        ('cem_perf_rollout_multi', dict(variance=True)),
                                        ('cem_perf_rollout_taylor_multi', dict())])
def test_a_fresh_device_table_is_alive_when_the_entry_is_called(monkeypatch, wrapper, kw):
    """Without `table=` the wrapper builds a table nobody else owns: freed before the launch, its memory goes to the
    launch's own output buffers and the first workgroups overwrite what the others still read."""
    import weakref

    import torch

    from safe_exploration_amd import cem_mpc
    seen = {}

    def get(self, ssms, dev):
        tensor = torch.zeros(4, dtype=torch.float64)
        seen['table'] = weakref.ref(tensor)
        return 'models', tensor

    def launch(entry, head, *args, **kwargs):
        seen['alive'] = seen['table']() is not None
        return {}

    monkeypatch.setattr(cem_mpc.GpModelTable, 'get', get)
    monkeypatch.setattr(cem_mpc.PerfModelTable, 'get', get)
    monkeypatch.setattr(cem_mpc, '_require_rbf', lambda ssms, x0: None)
    monkeypatch.setattr(cem_mpc, '_perf_rollout', launch)
    getattr(cem_mpc, wrapper)([object(), object()], _env(), torch.zeros((2, 2), dtype=torch.float64), 5, 8, 1,
                              safe_actions=None, obj_cost=None, con_cost=None, status=None, **kw)
    assert seen['alive'] is True and seen['table']() is None      # ... and it is released afterwards
