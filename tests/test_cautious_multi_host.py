"""CPU: Cautious MPC over a GP per problem, host side -- sx_cem_cautious_rollout_multi, sx_cem_cautious_rollout_sat_multi and
sx_cem_cautious_rollout_multi_form are declared, exported and check their arguments before any device access; the form query
against the streaming plan's rule; the multi-model kernels of every compiled shape are in the library;
MultiModelCautiousCemMpc.check_solvers; the runner's refusal of a mixed list; the separate ladders of
cautious_mpc.get_actions_multi over injected fake optimisers."""
import ctypes
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from safe_exploration_amd import _lib, cautious_mpc, cem_mpc, episode_runner
from safe_exploration_amd.cem_mpc import CautiousCemMpc, MultiModelCautiousCemMpc
from safe_exploration_amd.costs import SaturatingCost
from safe_exploration_amd.safempc_cem import MpcResult
from test_cautious_host import Conf, FakeMpc, _cautious
from test_perf_var_host import _env, _model, _Ssm
from test_stream_plan_host import rule_with_extra, taylor_extra_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI, SAT_MULTI, FORM = ('sx_cem_cautious_rollout_multi', 'sx_cem_cautious_rollout_sat_multi',
                          'sx_cem_cautious_rollout_multi_form')
VAR, ABS = _lib.SX_OBJ_NEG_VARIANCE, _lib.SX_OBJ_AFFINE_ABS
SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3


def _models(*models):
    return (_lib.SxGpModel * len(models))(*models)


def _cost():
    cost = _lib.SxSatCost()
    cost.trig_idx, cost.rank = -1, 1
    cost.v[0] = 1.0
    return cost


# ---- the entries -----------------------------------------------------------------------------------------------------------
def _declared_arguments(header, name):
    decl = header[header.index('int ' + name + '('):]
    return decl[decl.index('(') + 1:decl.index(');')].count(',') + 1


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sx_amd.h')).read()
    lib = _lib.lib()
    for name, count in ((MULTI, 20), (SAT_MULTI, 21), (FORM, 3)):
        assert re.search(r'\bint ' + name + r'\(', header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == count == _declared_arguments(header, name), name
        doc = header[:header.index('int ' + name + '(')].rsplit('/*', 1)[1]
        assert 'cautious_mpc.py' in doc or 'episode_runner.py' in doc, name       # what the entry replaces in the reference
    # the single-model entries' arguments with the table behind the models
    for multi, single in ((MULTI, 'sx_cem_cautious_rollout'), (SAT_MULTI, 'sx_cem_cautious_rollout_sat')):
        one = _lib.SIGNATURES[single][1]
        assert _lib.SIGNATURES[multi][1] == one[:1] + [ctypes.c_void_p] + one[1:]
    assert _lib.SIGNATURES[FORM][1][1:] == [ctypes.c_int, ctypes.c_int]
    assert callable(cem_mpc.cem_cautious_rollout_multi)


def _call(models, env, *, sat=False, cost='default', table=16, E=None, P=4, T=8, x0=16, mean=16, std=16, noise=16, rows=16,
          obj=16, con=16, status=16):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    E = len(models) if E is None and models is not None else E
    head = (models, p(table), None if env is None else ctypes.byref(env))
    if sat:
        cost = _cost() if cost == 'default' else cost
        head += (None if cost is None else ctypes.byref(cost),)
    return getattr(_lib.lib(), SAT_MULTI if sat else MULTI)(*head, E, P, T, p(x0), p(mean), p(std), p(noise), p(rows), p(obj),
                                                            p(con), None, None, None, None, 1, p(status), None)


@pytest.mark.parametrize('sat', [False, True])
def test_argument_errors_without_a_gpu(sat):
    """Every pointer is one that would fault if read (16), and this machine has no device: the answers come from the host."""
    three = lambda: _models(_model(n_train=7), _model(n_train=200), _model(n_train=590))
    env = _env()
    call = lambda models, env=env, **kw: _call(models, env, sat=sat, **kw)
    for kw in (dict(x0=None), dict(rows=None), dict(obj=None), dict(con=None), dict(status=None), dict(table=None),
               dict(mean=None), dict(std=None), dict(E=0), dict(P=0), dict(T=0), dict(T=-3)):      # (noise without mean / std)
        assert call(three(), **kw) == _lib.SX_ERR_ARG, kw
    assert call(None, E=3) == _lib.SX_ERR_ARG and call(three(), env=None) == _lib.SX_ERR_ARG
    if sat:
        assert call(three(), cost=None) == _lib.SX_ERR_ARG
        bad = _cost()
        bad.rank = 0
        assert call(three(), cost=bad) == _lib.SX_ERR_ARG
    # mixed (n_s, n_u) among the models, and models that disagree with env
    assert call(_models(_model(), _model(2, 2), _model())) == _lib.SX_ERR_ARG
    assert call(_models(_model(2, 2), _model(2, 2))) == _lib.SX_ERR_ARG
    # an unpacked or empty model among the n, wherever it stands
    for where in range(3):
        for field in ('x_train', 'a_pack', 'stage_tab'):
            models = three()
            setattr(models[where], field, None)
            assert call(models) == _lib.SX_ERR_ARG, (where, field)
        models = three()
        models[where].n_train = 0
        assert call(models) == _lib.SX_ERR_ARG
    if not sat:
        assert call(three(), env=_env(obj_mode=7)) == _lib.SX_ERR_ARG
    neg = _env()
    neg.m = -1
    assert call(three(), env=neg) == _lib.SX_ERR_ARG
    # SX_ERR_UNSUPPORTED, before any launch: too many rows, a shape without a kernel, a model without a form
    many = _env()
    many.m = _lib.SX_MAX_M + 1
    assert call(three(), env=many) == _lib.SX_ERR_UNSUPPORTED
    assert call(_models(_model(3, 2), _model(3, 2)), env=_env(3, 2)) == _lib.SX_ERR_UNSUPPORTED
    assert call(_models(_model(n_train=7), _model(n_train=1100))) == _lib.SX_ERR_UNSUPPORTED
    assert call(_models(_model(n_train=1100), _model(n_train=7)), noise=None, mean=None, std=None) == _lib.SX_ERR_UNSUPPORTED
    assert call(_models(_model(1, 1, n_train=7), _model(1, 1, n_train=1022)), env=_env(1, 1)) == _lib.SX_ERR_UNSUPPORTED


# ---- the form --------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1), (4, 1), (2, 2)]
TRIPLES = [(7, 200, 590), (7, 100, 200)]


@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_the_form_query_folds_the_plan_over_the_models(n_s, n_u):
    lib = _lib.lib()
    extra = taylor_extra_bytes(n_s, n_u, cautious=True)
    for sizes in TRIPLES:
        for T in (1, 2, 8):
            models = _models(*[_model(n_s, n_u, N) for N in sizes])
            own = [rule_with_extra(n_s, n_u, m.n_pad, T, extra) for m in models]
            assert all(f >= 0 for f in own)
            want = SX_FORM_BYOUT if SX_FORM_BYOUT in own else SX_FORM_STREAM       # plan_stream_multi's verdict
            assert int(lib.sx_cem_cautious_rollout_multi_form(models, len(sizes), T)) == want, (sizes, T)
            assert [int(lib.sx_cem_cautious_rollout_form(ctypes.byref(m), T)) for m in models] == own
            assert want == (SX_FORM_BYOUT if 590 in sizes else SX_FORM_STREAM)
            for e, m in enumerate(models):       # n = 1 is the single-model query
                assert int(lib.sx_cem_cautious_rollout_multi_form(_models(m), 1, T)) == own[e]
    form = lambda models, n=None, T=8: int(lib.sx_cem_cautious_rollout_multi_form(models, len(models) if n is None else n, T))
    past = _models(_model(n_s, n_u, 7), _model(n_s, n_u, 1100))              # a model past the LDS plan (n_pad > 1024)
    assert form(past) < 0 and form(past, n=1) == SX_FORM_STREAM
    assert form(None, n=2) < 0 and form(past, n=0) < 0 and form(_models(_model(n_s, n_u, 7)), T=0) < 0
    assert form(_models(_model(n_s, n_u, 7), _model(2, 2 if n_u == 1 else 1, 7))) < 0     # mixed shapes
    bad = _models(_model(n_s, n_u, 7), _model(n_s, n_u, 7))
    bad[1].a_pack = None
    assert form(bad) < 0
    assert form(_models(_model(3, 2), _model(3, 2))) < 0                       # a shape without a kernel


def test_every_compiled_shape_has_its_multi_model_kernels():
    """The shift-0 shapes of SX_ROLLOUT_SHAPES, read from the source; the instantiations by their symbols in the library:
    cem_cautious_rollout_kernel<NS, NU, BYOUT, SAT, MM = true>, and the launcher of either form."""
    src = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'sx_stream_launch.hpp')).read()
    body = re.search(r'#define SX_ROLLOUT_SHAPES\(X, \.\.\.\)((?:.*\\\n)*.*\n)', src).group(1)
    shapes = sorted({(int(a), int(b)) for a, b, sh in re.findall(r'X\((\d+), (\d+), (\d+), __VA_ARGS__\)', body) if sh == '0'})
    assert len(shapes) == 6 and (2, 1) in shapes and (1, 1) in shapes
    data = open(_lib.LIB_PATH, 'rb').read()
    for n_s, n_u in shapes:
        for sat in (0, 1):
            for byout in (0, 1):
                kernel = f'cem_cautious_rollout_kernelILi{n_s}ELi{n_u}ELb{byout}ELb{sat}ELb1EJEE'.encode()
                # one output has no output-by-output kernel
                assert (kernel in data) == (not (byout and n_s == 1)), (n_s, n_u, byout, sat)
            const = b'16CautiousSatConst' if sat else b'13CautiousConst'
            launcher = f'_ZN2sx20launch_perf_gp_multiILi{n_s}ELi{n_u}EEEiPKNS_7GpConstIXT_EXplT_T0_EEERKNS_'.encode() + const
            assert launcher in data, (n_s, n_u, sat)
    build = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'build.sh')).read()
    assert 'sx_cautious_multi.hip' in build and 'sx_cautious_sat_multi.hip' in build
    host = open(os.path.join(ROOT, 'safe_exploration_amd', 'csrc', 'sx_cautious_host.hpp')).read()
    assert 'SX_ERR_UNSUPPORTED' not in host                                      # the stub is gone


# ---- the wrapper and the class --------------------------------------------------------------------------------------------
def test_wrapper_raises_fused_multi_unsupported():
    z = lambda *s: torch.zeros(s, dtype=torch.float64)
    ssms, env = [_Ssm(), _Ssm(n_train=100)], _env()
    fake = mock.Mock()
    fake.sx_cem_cautious_rollout_multi.return_value = _lib.SX_ERR_UNSUPPORTED
    fake.sx_cem_cautious_rollout_sat_multi.return_value = _lib.SX_OK
    table = mock.Mock(spec=cem_mpc.GpModelTable)
    table.family = 'rbf'
    table.get.return_value = ('models', z(4))
    with mock.patch.object(_lib, 'require_gpu', lambda *a: None), mock.patch.object(_lib, 'lib', lambda: fake), \
            mock.patch.object(_lib, 'stream_ptr', lambda dev: None):
        call = lambda **kw: cem_mpc.cem_cautious_rollout_multi(ssms, env, z(2, 2), 3, table=table, **kw)
        with pytest.raises(cem_mpc.FusedMultiUnsupported, match='no single launch of the cautious rollout'):
            call(rows=z(2, 4, 3, 1))
        with pytest.raises(ValueError, match='one word per problem'):
            call(rows=z(2, 4, 3, 1), status=torch.zeros(1, dtype=torch.int32))
        with pytest.raises(ValueError, match='one model per problem'):
            cem_mpc.cem_cautious_rollout_multi(ssms, env, z(3, 2), 3, table=table, rows=z(3, 4, 3, 1))
        with pytest.raises(NotImplementedError, match='exact RBF'):
            cem_mpc.cem_cautious_rollout_multi([_Ssm(), _Ssm('feature')], env, z(2, 2), 3, table=table, rows=z(2, 4, 3, 1))
        cost = SaturatingCost([0.0, 0.0], np.eye(2))
        out = call(noise=z(2, 4, 3, 1), mean=z(2, 3, 1), std=z(2, 3, 1), cost=cost, want_cov=True)
        args = fake.sx_cem_cautious_rollout_sat_multi.call_args[0]
        assert len(args) == 21 and args[0] == 'models' and args[4:7] == (2, 4, 3) and args[18] == 1
        assert tuple(out['status'].shape) == (2,) and tuple(out['cov'].shape) == (2, 4, 3, 2, 2)


def _solvers(n=3, **kw):
    base = dict(time_horizon=5, num_rollouts=64, num_elites=8, num_iterations=3, propagate=True, init_std=0.2)
    out = []
    for e in range(n):
        s = dict(base, **{k: v for k, v in kw.items() if not isinstance(v, dict)})
        s.update({k: v[e] for k, v in kw.items() if isinstance(v, dict) and e in v})
        env = s.pop('env', None) or _env()
        out.append(CautiousCemMpc(_Ssm(n_train=20 + e), env, s.pop('time_horizon'), s.pop('num_rollouts'),
                                  s.pop('num_elites'), s.pop('num_iterations'), device='cpu', seed=e, **s))
    return out


def test_check_solvers_refuses_each_disagreement_by_name():
    MultiModelCautiousCemMpc.check_solvers(_solvers())
    for name, other in (('time_horizon', 4), ('num_rollouts', 128), ('num_elites', 4), ('num_iterations', 2),
                        ('propagate', False), ('init_std', 0.5)):
        with pytest.raises(ValueError, match=name):
            MultiModelCautiousCemMpc.check_solvers(_solvers(**{name: {1: other}}))
    with pytest.raises(ValueError, match=r'environment constants \(env'):
        MultiModelCautiousCemMpc.check_solvers(_solvers(env={2: _env(obj_mode=ABS)}))
    beta = _env()
    beta.beta = 3.0
    with pytest.raises(ValueError, match='env'):
        MultiModelCautiousCemMpc.check_solvers(_solvers(env={1: beta}))
    solvers = _solvers()
    solvers[1].set_cost(SaturatingCost([0.0, 0.0], np.eye(2)))
    with pytest.raises(ValueError, match='cost'):
        MultiModelCautiousCemMpc.check_solvers(solvers)
    for s in solvers:
        s.set_cost(SaturatingCost([0.0, 0.0], np.eye(2)))
    MultiModelCautiousCemMpc.check_solvers(solvers)                              # equal costs agree
    with pytest.raises(ValueError, match='cost'):
        solvers[2].set_cost(SaturatingCost([0.5, 0.0], np.eye(2)))
        MultiModelCautiousCemMpc.check_solvers(solvers)
    # the constructors
    with pytest.raises(ValueError, match='MultiModelCautiousCemMpc'):
        CautiousCemMpc([_Ssm(), _Ssm()], _env(), 5, 64, 8, 3, device='cpu')
    multi = MultiModelCautiousCemMpc.from_solvers(_solvers())
    assert len(multi.solvers) == 3 and multi.last_status == [0, 0, 0] and multi.per_model_solves == 0
    built = MultiModelCautiousCemMpc([_Ssm(), _Ssm(n_train=100)], _env(), 5, 64, 8, 3, device='cpu', seed=7, propagate=False)
    assert [s._gen.initial_seed() for s in built.solvers] == [7, 8] and not built.solvers[1]._propagate
    with pytest.raises(ValueError, match='num_rollouts'):
        MultiModelCautiousCemMpc.from_solvers(_solvers(num_rollouts={2: 32}))
    with pytest.raises(NotImplementedError, match='process group'):
        MultiModelCautiousCemMpc([_Ssm()], _env(), 5, 64, 8, 3, device='cpu', process_group=object())


def test_fused_applies_reads_the_form_and_the_hooks():
    mk = lambda sizes: MultiModelCautiousCemMpc([_packed(n) for n in sizes], _env(), 5, 64, 8, 3, device='cpu')
    assert mk((7, 200, 590)).form() == SX_FORM_BYOUT and mk((7, 200)).form() == SX_FORM_STREAM
    assert mk((7, 200)).fused_applies() and not mk((7, 1100)).fused_applies()
    hooked = mk((7, 200))
    hooked.solvers[1].set_env(_env(), objective_hook=lambda ps: ps[:, 0])
    assert not hooked.fused_applies()
    hooked.set_cost(SaturatingCost([0.0, 0.0], np.eye(2)))                       # a kernel cost: the hook is not evaluated
    assert hooked.fused_applies()
    # a solve that cannot be fused raises before it draws anything
    state = [s._gen.get_state() for s in hooked.solvers]
    with pytest.raises(cem_mpc.FusedMultiUnsupported):
        mk((7, 1100)).solve(torch.zeros((2, 2), dtype=torch.float64))
    assert all(torch.equal(a, s._gen.get_state()) for a, s in zip(state, hooked.solvers))


def _packed(n_train):
    ssm = _Ssm(n_train=n_train)
    ssm.device_model = _model(2, 1, n_train)
    return ssm


def test_a_multi_solve_is_one_rollout_and_one_ranking_per_iteration(monkeypatch):
    seen = []
    E, P, T, iters = 3, 64, 5, 3

    def rollout(ssms, env, x0, T_, *, mean, std, noise, propagate, status, table, **kw):
        seen.append(('rollout', len(ssms), T_, tuple(mean.shape), noise.clone(), propagate, tuple(status.shape), kw))
        z = torch.zeros((E, P), dtype=torch.float64)
        return dict(rows=mean.unsqueeze(1) + std.unsqueeze(1) * noise, obj_cost=z, con_cost=z, status=status)

    def rank(con, obj, rows, k, **kw):
        seen.append(('rank', k, kw))
        return dict(mean=torch.zeros((E, T)), std=torch.ones((E, T)), best=rows[:, 0].reshape(E, -1),
                    best_ok=torch.ones(E, dtype=torch.int32), elite_rows=None)

    monkeypatch.setattr(cem_mpc, 'cem_cautious_rollout_multi', rollout)
    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)
    monkeypatch.setattr(cem_mpc, 'cem_cautious_rollout', lambda *a, **kw: pytest.fail('a single-model rollout'))
    mpc = MultiModelCautiousCemMpc([_packed(n) for n in (7, 100, 200)], _env(), T, P, 8, iters, device='cpu', init_std=0.2,
                                   propagate=False, seed=11)
    init = torch.full((E, T, 1), 0.5, dtype=torch.float64)
    best, ok, status = mpc.solve(torch.zeros((E, 2), dtype=torch.float64), init_mean=init)
    assert [s[0] for s in seen] == ['rollout', 'rank'] * iters and tuple(best.shape) == (E, T, 1)
    assert tuple(status.shape) == (E,) and status.dtype == torch.int32
    assert seen[0][1:4] == (E, T, (E, T, 1)) and seen[0][5:] == (False, (E,), {})
    assert seen[1][1:] == (8, dict(want_refit=True))
    # problem e saw what solver e draws: sample_noise(1) of a solver with seed 11 + e
    for e in range(E):
        twin = CautiousCemMpc(_packed(7), _env(), T, P, 8, iters, device='cpu', seed=11 + e)
        draws = twin.sample_noise(1)
        for it in range(iters):
            assert torch.equal(seen[2 * it][4][e], draws[it, 0]), (e, it)
    with pytest.raises(ValueError, match='noise'):
        mpc.solve(torch.zeros((E, 2), dtype=torch.float64), noise=torch.zeros((iters, E, P, T + 1, 1), dtype=torch.float64))


# ---- the runner and the ladders ----------------------------------------------------------------------------------------------
def test_do_rollout_batch_refuses_a_mixed_list():
    cautious, spec = _cautious([])
    other = mock.Mock()                                                          # any solver that is not a CautiousCemMPC
    envs = [mock.Mock(), mock.Mock()]
    with pytest.raises(ValueError, match='mix'):
        episode_runner.do_rollout_batch(envs, 3, [cautious, other])
    with pytest.raises(ValueError, match='mix'):
        episode_runner.do_rollout_batch(envs, 3, [other, cautious])
    assert not envs[0].reset.called                                              # refused before an environment is touched
    with pytest.raises(ValueError, match='CautiousCemMPC'):
        cautious_mpc.get_actions_multi([cautious, other], np.zeros((2, 2)))


def test_do_rollout_batch_sends_cautious_solvers_to_their_own_multi():
    from safe_exploration_amd import problems
    row = np.arange(1.0, 5.0).reshape(4, 1) / 10
    pairs = [_cautious([row, None, row * 2]), _cautious([None, row * 3, None])]
    solvers = [p[0] for p in pairs]
    envs = [problems.StubEnv(p[1], np.array([0.01 * (e + 1), 0.0]), never_done=True) for e, p in enumerate(pairs)]
    with mock.patch.object(episode_runner, 'get_actions_multi', side_effect=AssertionError('the SafeMPC path')):
        res = episode_runner.do_rollout_batch(envs, 3, solvers)
    F, Pv, S = MpcResult.FOUND_SOLUTION, MpcResult.PREVIOUS_SOLUTION, MpcResult.SAFE_CONTROLLER
    assert res[0].mpc_results == [F, Pv, F] and res[1].mpc_results == [S, F, Pv]
    assert [len(s._mpc.inits) for s in solvers] == [3, 3]


def test_get_actions_multi_keeps_separate_ladders():
    row = np.arange(1.0, 5.0).reshape(4, 1)
    scripts = [[row, None, None, None, None, 3 * row], [None, -row, -2 * row, None, None, None]]
    pairs = [_cautious(script, safe_policy=(lambda x: np.array([7.0])) if e else None) for e, script in enumerate(scripts)]
    solvers, spec = [p[0] for p in pairs], pairs[0][1]
    states = np.array([[0.1, -0.2], [0.0, 0.3]])
    F, Pv, S = MpcResult.FOUND_SOLUTION, MpcResult.PREVIOUS_SOLUTION, MpcResult.SAFE_CONTROLLER
    want = [([F, S], [1.0, 7.0], [0, Conf.T]), ([Pv, F], [2.0, -1.0], [1, 0]), ([Pv, F], [3.0, -2.0], [2, 0]),
            ([Pv, Pv], [4.0, -4.0], [3, 1]), ([S, Pv], [float((spec.k_fb @ states[0])[0]), -6.0], [4, 2]),
            ([F, Pv], [3.0, -8.0], [0, 3])]
    for step, (results, first, fails) in enumerate(want):
        acts, res = cautious_mpc.get_actions_multi(solvers, states)
        assert res == results and [s.n_fail for s in solvers] == fails, step
        np.testing.assert_array_equal(acts[:, 0], first)
    # every solver was asked once per step, for its own state alone, from its own warm start
    inits = [[i.numpy() for i in s._mpc.inits] for s in solvers]
    assert all(len(i) == len(want) and all(x.shape == (1, 4, 1) for x in i) for i in inits)
    assert not inits[0][0].any() and np.array_equal(inits[0][1][0, :, 0], [2.0, 3.0, 4.0, 4.0]) and not inits[0][2].any()
    assert not inits[1][1].any() and np.array_equal(inits[1][2][0, :, 0], [-2.0, -3.0, -4.0, -4.0])
    assert np.array_equal(inits[1][3][0, :, 0], [-4.0, -6.0, -8.0, -8.0]) and not inits[1][4].any()
    assert np.array_equal(solvers[0].k_ff_old, 3 * row) and np.array_equal(solvers[1].k_ff_old, -2 * row)
    with pytest.raises(ValueError, match='shape'):
        cautious_mpc.get_actions_multi(solvers, states[:1])


def test_get_actions_multi_caches_one_multi_object_on_the_first_solver():
    """Over real CautiousCemMpc optimisers the multi object is built once and handed the stacked warm starts."""
    solvers = [_cautious(None)[0] for _ in range(2)]
    for e, s in enumerate(solvers):
        s._ssm = _packed(20 + e)
    calls = []

    def fake(self, flat, init_mean=None, where='get_actions_multi'):
        calls.append((self, tuple(flat.shape), init_mean.clone()))
        return torch.ones((2, 4, 1), dtype=torch.float64) * torch.tensor([1.0, 2.0]).view(2, 1, 1), torch.tensor([True, False])

    with mock.patch.object(MultiModelCautiousCemMpc, 'get_actions_multi', fake):
        for _ in range(2):
            acts, res = cautious_mpc.get_actions_multi(solvers, np.zeros((2, 2)))
    assert calls[0][0] is calls[1][0] is solvers[0]._multi[1] and calls[0][1] == (2, 6)
    assert calls[0][0].solvers == [s._mpc for s in solvers]
    assert res == [MpcResult.FOUND_SOLUTION, MpcResult.SAFE_CONTROLLER] and solvers[0].n_fail == 0
    assert not calls[0][2].any() and bool((calls[1][2][0] == 1.0).all()) and not calls[1][2][1].any()


def test_update_models_multi_subtracts_each_prior():
    pairs = [_cautious([]) for _ in range(2)]
    solvers = [p[0] for p in pairs]
    rng = np.random.default_rng(0)
    xs, ys = [rng.normal(size=(5, 3)) for _ in solvers], [rng.normal(size=(5, 2)) for _ in solvers]
    with mock.patch.object(cautious_mpc.gp_ssm_cem, 'update_models_multi') as upd:
        cautious_mpc.update_models_multi(solvers, xs, ys, opt_hyp=True, replace_old=False)
    ssms, xt, yt, opt_hyp, replace_old = upd.call_args[0]
    assert ssms == [s._ssm for s in solvers] and opt_hyp is True and replace_old is False
    for s, x, y, a, b in zip(solvers, xs, ys, xt, yt):
        np.testing.assert_array_equal(a.numpy(), x)
        np.testing.assert_array_equal(b.numpy(), y - s.eval_prior(x[:, :2], x[:, 2:]))
    with pytest.raises(ValueError, match='solvers'):
        cautious_mpc.update_models_multi(solvers, xs[:1], ys)
