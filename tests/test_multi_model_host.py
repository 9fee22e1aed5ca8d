"""CPU: the multi-model rollout entries' argument checks and plan (sx_gp_model_table[_bytes], sx_cem_rollout[_elites]_multi,
sx_cem_rollout_multi_form).  Everything here is answered before any device access."""
import ctypes
import os

import pytest

from safe_exploration_amd import _lib

SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3   # include/sx_amd.h


def _model(n_s, n_u, n_train, dev_ptrs=False):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.n_pad = (n_train + 1 + n_s + n_u + 15) // 16 * 16   # sx_gp.hpp: gp_n_pad
    if dev_ptrs:   # never dereferenced: every call below fails its checks first
        m.x_train = m.a_pack = m.stage_tab = 0x1000
    return m


def _models(shapes, dev_ptrs=False):
    return (_lib.SxGpModel * len(shapes))(*[_model(*s, dev_ptrs=dev_ptrs) for s in shapes])


def _env(n_s, n_u):
    env = _lib.SxEnv()
    env.n_s, env.n_u, env.m = n_s, n_u, 4
    return env


FAKE = ctypes.c_void_p(0x1000)   # a non-null "device" pointer the checks reject before using it


def _rollout(lib, models, E, env, P=32, H=5, table=FAKE, status=FAKE):
    return lib.sx_cem_rollout_multi(models, table, ctypes.byref(env), E, P, H, FAKE, None, None, None, None, FAKE, None,
                                    None, FAKE, FAKE, status, None)


def _elites(lib, models, E, env, P=32, H=5, table=FAKE, k=3):
    return lib.sx_cem_rollout_elites_multi(models, table, ctypes.byref(env), E, P, H, FAKE, None, FAKE, k, FAKE, FAKE, None,
                                           None, FAKE, FAKE, FAKE, None, None, None)


def test_table_bytes_scale_with_the_problem_count():
    lib = _lib.lib()
    one = lib.sx_gp_model_table_bytes(2, 1, 1)
    assert one > 0 and one % 8 == 0
    for E in (2, 3, 6, 8, 64):
        assert lib.sx_gp_model_table_bytes(2, 1, E) == E * one
    assert lib.sx_gp_model_table_bytes(4, 2, 6) == 6 * lib.sx_gp_model_table_bytes(4, 2, 1) > 6 * one
    for bad in ((2, 1, 0), (2, 1, -3), (0, 1, 4), (5, 1, 4), (2, 3, 4), (3, 2, 4)):   # (3, 2): no rollout kernel
        assert lib.sx_gp_model_table_bytes(*bad) < 0


def test_table_rejects_bad_arguments_before_any_device_access():
    lib = _lib.lib()
    ok = _models([(2, 1, 60), (2, 1, 200)], dev_ptrs=True)
    assert lib.sx_gp_model_table(ok, 2, None, None) == _lib.SX_ERR_ARG                  # null table
    assert lib.sx_gp_model_table(None, 2, FAKE, None) == _lib.SX_ERR_ARG                # null models
    assert lib.sx_gp_model_table(ok, 0, FAKE, None) == _lib.SX_ERR_ARG                  # E <= 0
    assert lib.sx_gp_model_table(ok, -1, FAKE, None) == _lib.SX_ERR_ARG
    mixed = _models([(2, 1, 60), (2, 2, 60)], dev_ptrs=True)
    assert lib.sx_gp_model_table(mixed, 2, FAKE, None) == _lib.SX_ERR_ARG               # (n_s, n_u) differ
    mixed = _models([(2, 1, 60), (4, 1, 60)], dev_ptrs=True)
    assert lib.sx_gp_model_table(mixed, 2, FAKE, None) == _lib.SX_ERR_ARG
    no_ptrs = _models([(2, 1, 60), (2, 1, 200)])
    assert lib.sx_gp_model_table(no_ptrs, 2, FAKE, None) == _lib.SX_ERR_ARG             # a model without device buffers


def test_rollout_entries_reject_bad_arguments_before_any_device_access():
    lib = _lib.lib()
    ok, env = _models([(2, 1, 60), (2, 1, 200), (2, 1, 90)]), _env(2, 1)
    for call in (_rollout, _elites):
        assert call(lib, ok, 3, env, table=None) == _lib.SX_ERR_ARG                       # null table
        assert call(lib, None, 3, env) == _lib.SX_ERR_ARG                                 # null models
        assert call(lib, ok, 0, env) == _lib.SX_ERR_ARG                                   # E <= 0
        assert call(lib, ok, -2, env) == _lib.SX_ERR_ARG
        assert call(lib, ok, 3, env, P=0) == _lib.SX_ERR_ARG
        assert call(lib, ok, 3, env, H=0) == _lib.SX_ERR_ARG
        assert call(lib, _models([(2, 1, 60), (2, 2, 60), (2, 1, 60)]), 3, env) == _lib.SX_ERR_ARG   # models differ
        assert call(lib, ok, 3, _env(2, 2)) == _lib.SX_ERR_ARG                           # models vs env
        assert call(lib, ok, 3, _env(4, 1)) == _lib.SX_ERR_ARG
    assert _rollout(lib, ok, 3, env, status=None) == _lib.SX_ERR_ARG                       # null status words
    assert _elites(lib, ok, 3, env, k=0) == _lib.SX_ERR_ARG
    # noise without a sampling distribution
    assert lib.sx_cem_rollout_multi(ok, FAKE, ctypes.byref(env), 3, 32, 5, FAKE, None, None, None, FAKE, FAKE, None, None,
                                    FAKE, FAKE, FAKE, None) == _lib.SX_ERR_ARG


def test_rollout_entries_answer_the_constraint_count_after_the_arguments():
    lib = _lib.lib()
    ok, env = _models([(2, 1, 60)] * 3), _env(2, 1)
    assert lib.sx_cem_rollout_multi(ok, FAKE, ctypes.byref(env), 3, 32, 5, None, None, None, None, None, FAKE, None, None,
                                    FAKE, FAKE, FAKE, None) == _lib.SX_ERR_ARG                    # null x0
    assert lib.sx_cem_rollout_multi(ok, FAKE, ctypes.byref(env), 3, 32, 5, FAKE, None, None, None, None, FAKE, None, None,
                                    None, FAKE, FAKE, None) == _lib.SX_ERR_ARG                    # null objective costs
    assert lib.sx_cem_rollout_elites_multi(ok, FAKE, ctypes.byref(env), 3, 32, 5, FAKE, None, FAKE, 3, FAKE, FAKE, None,
                                           None, FAKE, FAKE, FAKE, FAKE, None, None) == _lib.SX_ERR_ARG   # mean_out alone
    for m_bad in (0, _lib.SX_MAX_M + 1):                                # constraint rows outside 1 .. SX_MAX_M
        env.m = m_bad
        assert _rollout(lib, ok, 3, env) == _lib.SX_ERR_UNSUPPORTED
        assert _elites(lib, ok, 3, env) == _lib.SX_ERR_UNSUPPORTED
        assert _rollout(lib, ok, 3, env, status=None) == _lib.SX_ERR_ARG   # argument errors answer first
        assert _elites(lib, ok, 3, env, k=0) == _lib.SX_ERR_ARG


@pytest.mark.skipif(bool(os.environ.get('SX_ROLLOUT')), reason='SX_ROLLOUT forces a form')
def test_workspace_path_models_make_the_multi_form_negative():
    """The multi form is negative exactly where some model needs the workspace path (sx_cem_rollout_workspace_bytes > 0);
    otherwise it is the streaming kernel, output by output as soon as one model needs that."""
    lib, H = _lib.lib(), 15
    for n_s, n_u, sizes in ((2, 1, (60, 200, 260, 600, 1000, 1100, 2000)), (4, 1, (60, 128, 260, 400, 700)),
                            (2, 2, (60, 300, 900, 1100)), (3, 1, (77, 500, 1200))):
        for N in sizes:
            for others in ((), (60,), (60, 200)):
                ms = _models([(n_s, n_u, n) for n in others + (N,)])
                E = len(ms)
                big = [lib.sx_cem_rollout_workspace_bytes(ctypes.byref(ms[i]), E, 4096, H) > 0 for i in range(E)]
                form = lib.sx_cem_rollout_multi_form(ms, E, H)
                assert (form < 0) == any(big), (n_s, n_u, others, N, form)
                if form >= 0:
                    single = [lib.sx_cem_rollout_form(ctypes.byref(ms[i]), H) for i in range(E)]
                    assert form == (SX_FORM_BYOUT if SX_FORM_BYOUT in single else SX_FORM_STREAM), (single, form)


def test_multi_form_rejects_bad_arguments_and_shapes_without_a_kernel():
    lib = _lib.lib()
    ms = _models([(2, 1, 60), (2, 1, 200)])
    assert lib.sx_cem_rollout_multi_form(ms, 2, 15) == SX_FORM_STREAM
    assert lib.sx_cem_rollout_multi_form(ms, 0, 15) < 0
    assert lib.sx_cem_rollout_multi_form(ms, 2, 0) < 0
    assert lib.sx_cem_rollout_multi_form(None, 2, 15) < 0
    assert lib.sx_cem_rollout_multi_form(_models([(2, 1, 60), (2, 2, 60)]), 2, 15) < 0
    assert lib.sx_cem_rollout_multi_form(_models([(3, 2, 77)]), 1, 15) < 0       # (3, 2): no rollout kernel


# ---- the host layer: one base class, one comparison of the solvers' settings ---------------------------------------------------------
def _fused_solvers(cls, n=2):
    """Solvers of the kind `cls` solves over (a FusedCemMpc each), equal in every setting."""
    from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelConsCemMpc, MultiModelPerfCemMpc
    from test_conset_host import _set
    from test_perf_multi_host import _Ssm, _env as solver_env
    kw = dict(con_set=_set()) if cls is MultiModelConsCemMpc else dict(n_perf=6) if cls is MultiModelPerfCemMpc else {}
    return [FusedCemMpc(_Ssm(20 + 50 * e), solver_env(), 5, 64, 8, 3, device='cpu', init_std=0.2, seed=e, **kw)
            for e in range(n)]


def _cem_classes():
    from safe_exploration_amd.cem_mpc import MultiModelCemMpc, MultiModelConsCemMpc, MultiModelPerfCemMpc
    return [MultiModelCemMpc, MultiModelConsCemMpc, MultiModelPerfCemMpc]


@pytest.mark.parametrize('cls', _cem_classes())
def test_check_solvers_names_the_setting_and_the_solver(cls):
    import re
    import torch
    from safe_exploration_amd import cem_mpc
    from test_perf_multi_host import _env as solver_env
    cls.check_solvers(_fused_solvers(cls))
    cls.from_solvers(_fused_solvers(cls))
    assert len(cls._SHARED) == 12 and {'__class__', '_init_std', '_env', cem_mpc.perf_spec_of} < {attr for _, attr in cls._SHARED}

    def refused(solvers, name):
        named = re.escape(name) + r': solver (0 has .*, solver 1 has|1 differs from solver 0)'
        with pytest.raises(ValueError, match='CEM settings.*of these, ' + named):
            cls.check_solvers(solvers)

    # every entry of the table, solver 1 holding another value than solver 0
    for name, attr in cls._SHARED:
        solvers = _fused_solvers(cls)
        if attr == '__class__':
            solvers[1].__class__ = type('Other', (type(solvers[1]),), {})
        elif attr is cem_mpc.perf_spec_of:      # the five settings of the performance trajectory: one row, one value
            for field in cem_mpc.PerfSpec._fields:
                solvers = _fused_solvers(cls)
                solvers[1]._perf = solvers[1]._perf._replace(**{field: object()})
                refused(solvers, name)
                assert all(n in name for n in cem_mpc.KEYWORD_NAMES[:5])
            continue
        else:
            setattr(solvers[1], attr, object())
        refused(solvers, name)
    # init_std and the environment by their values
    solvers = _fused_solvers(cls)
    solvers[1]._init_std = solvers[1]._init_std + 0.25
    refused(solvers, 'init_std')
    solvers = _fused_solvers(cls)
    moved = solver_env()
    moved.beta = 7.0
    solvers[1].set_env(moved)
    refused(solvers, 'the environment constants (sx_env)')
    # what differs is printed where it prints
    solvers = _fused_solvers(cls)
    solvers[1]._num_rollouts = 128
    with pytest.raises(ValueError, match='num_rollouts: solver 0 has 64, solver 1 has 128'):
        cls.check_solvers(solvers)
    third = _fused_solvers(cls, 3)
    third[2]._init_std = torch.full_like(third[2]._init_std, 0.5)
    with pytest.raises(ValueError, match='init_std: solver 2 differs from solver 0'):
        cls.check_solvers(third)


def _all_classes():
    from safe_exploration_amd.cem_mpc import MultiModelCautiousCemMpc, MultiModelStaticCemMpc
    return _cem_classes() + [MultiModelStaticCemMpc, MultiModelCautiousCemMpc]


@pytest.mark.parametrize('cls', _all_classes())
def test_every_multi_model_class_stands_on_the_one_base(cls):
    import inspect
    from safe_exploration_amd import cem_mpc
    base = cem_mpc.MultiModelCem
    assert issubclass(cls, base) and cls is not base
    for name in ('solvers', 'last_status', 'check_solvers'):
        assert all(name not in vars(k) for k in cls.__mro__ if k not in (base, object)), name
    assert cls.solvers is base.solvers and cls.last_status is base.last_status
    assert cls.check_solvers.__func__ is base.check_solvers.__func__
    assert cls._SHARED and cls._POLICY.what
    # the counters are the base constructor's: no subclass sets them
    for k in cls.__mro__[:-2]:
        assert all(name not in inspect.getsource(k) for name in ('per_model_solves = ', 'stepwise_fallbacks = ')), k.__name__
    if cls is cem_mpc.MultiModelStaticCemMpc:
        from test_static_multi_host import _solver
        solvers = [_solver(20), _solver(70)]
    elif cls is cem_mpc.MultiModelCautiousCemMpc:
        from test_cautious_multi_host import _solvers
        solvers = _solvers(2)
    else:
        solvers = _fused_solvers(cls)
    mpc = cls.from_solvers(solvers)
    assert mpc.per_model_solves == 0 and mpc.stepwise_fallbacks == 0
    assert mpc.solvers is mpc._solvers and mpc.solvers == solvers and mpc.last_status == [0, 0]
