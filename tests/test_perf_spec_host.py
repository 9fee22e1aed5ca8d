"""`PerfSpec`: the one value that says whether a solve has a performance trajectory and which one, its one validation under
both spellings of the settings, and the one accessor `perf_spec_of`.  Host only: nothing is launched."""
from unittest import mock

import pytest

from safe_exploration_amd import safempc_cem
from safe_exploration_amd.cem_mpc import CONF_NAMES, KEYWORD_NAMES, PERF_OFF, FusedCemMpc, PerfSpec, perf_spec_of
from safe_exploration_amd.safempc_cem import CemSafeMPC
from test_perf_multi_host import _env, _safempc, _Ssm, conf

H = 5       # the safety horizon of every case here (Conf.mpc_time_horizon)

# (the spec, the fields whose names the message must carry); every one is a ValueError in both constructors
RULES = [
    (PerfSpec(-1), ('n_perf',)),                                                         # n_perf >= 0
    (PerfSpec(6, 0), ('r', 'n_perf', 'horizon')),                                        # 1 <= r
    (PerfSpec(8, H + 1), ('r', 'n_perf', 'horizon')),                                    # r <= H
    (PerfSpec(3, 3), ('r', 'n_perf')),                                                   # n_perf > r
    (PerfSpec(0, variance=True), ('variance', 'n_perf')),                                # variance needs n_perf > 0
    (PerfSpec(6, type='unscented'), ('type',)),                                          # type in PERF_TYPES
    (PerfSpec(0, type='taylor'), ('type', 'n_perf')),                                    # 'taylor' needs n_perf > 0
    (PerfSpec(0, terminal_safety=True), ('terminal_safety',)),                           # terminal_safety needs n_perf > 0 ...
    (PerfSpec(0, type='taylor', terminal_safety=True), ('n_perf',)),
    (PerfSpec(H + 2, terminal_safety=True), ('terminal_safety', 'type')),                # ... and 'taylor'
    (PerfSpec(H + 2, variance=True, terminal_safety=True), ('terminal_safety', 'type')),
    (PerfSpec(H + 1, type='taylor', terminal_safety=True), ('terminal_safety', 'n_perf', 'horizon')),   # n_perf >= H + 2
]


@pytest.mark.parametrize('names', [KEYWORD_NAMES, CONF_NAMES], ids=['keywords', 'conf'])
@pytest.mark.parametrize('spec, fields', RULES)
def test_every_rule_raises_and_names_the_setting_as_the_caller_spells_it(names, spec, fields):
    with pytest.raises(ValueError) as err:
        spec.checked(H, names=names)
    message = str(err.value)
    for field in fields:
        assert getattr(names, field) in message, (field, message)
    if names is KEYWORD_NAMES:
        assert 'cem_' not in message and 'mpc_time_horizon' not in message, message
    else:       # every mention of a setting carries the configuration's prefix
        stripped = message
        for name in CONF_NAMES[:6]:
            stripped = stripped.replace(name, '')
        assert not any(name in stripped for name in KEYWORD_NAMES[:6]), message


def test_the_names_are_the_constructors_own():
    assert KEYWORD_NAMES[:6] == ('n_perf', 'perf_r', 'perf_variance', 'perf_type', 'perf_terminal_safety', 'time_horizon')
    assert CONF_NAMES[:6] == ('cem_n_perf', 'cem_perf_r', 'cem_perf_variance', 'cem_perf_type', 'cem_perf_terminal_safety',
                              'mpc_time_horizon')
    assert KEYWORD_NAMES._fields[:5] == PerfSpec._fields
    # ... and the default of `names` is the keywords'
    with pytest.raises(ValueError, match=r'1 <= perf_r <= time_horizon and n_perf > perf_r, got n_perf=6, perf_r=0'):
        PerfSpec(6, 0).checked(H)


def test_each_caller_keeps_its_order_of_the_rules():
    """Two rules broken at once: the constructor's keywords name the range first, the configuration's settings last."""
    both = PerfSpec(6, 0, terminal_safety=True)
    with pytest.raises(ValueError, match='1 <= perf_r <= time_horizon'):
        both.checked(H)
    with pytest.raises(ValueError, match=r"cem_perf_terminal_safety needs the propagated covariance \(cem_perf_type='taylor'\)"):
        both.checked(H, names=CONF_NAMES)
    # the same through the two constructors
    with pytest.raises(ValueError, match='1 <= perf_r <= time_horizon'):
        FusedCemMpc(_Ssm(), _env(), H, 64, 8, 3, device='cpu', n_perf=6, perf_r=0, perf_terminal_safety=True)
    with pytest.raises(ValueError, match='cem_perf_terminal_safety needs'):
        _safempc(conf(cem_n_perf=6, cem_perf_r=0, cem_perf_terminal_safety=True))
    with pytest.raises(ValueError, match='1 <= cem_perf_r <= mpc_time_horizon'):
        _safempc(conf(cem_n_perf=6, cem_perf_r=0))


def test_a_valid_spec_comes_back_with_plain_fields():
    for names in (KEYWORD_NAMES, CONF_NAMES):
        assert PERF_OFF.checked(H, names=names) == PerfSpec(0, 1, False, 'mean_equivalent', False) == PerfSpec()
        assert PerfSpec(0, r=99).checked(H, names=names).on is False               # r is not read without a trajectory
        assert PerfSpec(6, H).checked(H, names=names) == PerfSpec(6, H)
        assert PerfSpec(H + 2, 1, False, 'taylor', True).checked(H, names=names).terminal_safety is True
    spec = PerfSpec(6.0, True, 1, 'taylor', 0).checked(H)
    assert spec == PerfSpec(6, 1, True, 'taylor', False)
    assert [type(v) for v in spec] == [int, int, bool, str, bool]
    with pytest.raises(AttributeError):
        spec.n_perf = 7                                                            # immutable


def test_kind_tail_and_row_steps():
    assert (PERF_OFF.on, PERF_OFF.kind, PERF_OFF.tail, PERF_OFF.row_steps(H)) == (False, None, 0, H)
    # off whatever else is set (unchecked specs of stand-ins included)
    odd = PerfSpec(0, 3, True, 'taylor', True)
    assert (odd.on, odd.kind, odd.tail, odd.row_steps(H)) == (False, None, 0, H)
    for spec, kind in ((PerfSpec(6, 2), 'mean'), (PerfSpec(6, 2, variance=True), 'variance'),
                       (PerfSpec(6, 2, type='taylor'), 'taylor'), (PerfSpec(6, 2, True, 'taylor'), 'taylor'),
                       (PerfSpec(7, 2, type='taylor', terminal_safety=True), 'taylor')):
        assert spec.on and spec.kind == kind
        assert spec.tail == spec.n_perf - 2 and spec.row_steps(H) == H + spec.n_perf - 2 and spec.row_steps(9) == 9 + spec.tail


def test_keywords_are_the_constructors_and_leave_defaults_out():
    assert PERF_OFF.keywords() == dict(n_perf=0, perf_r=1)
    assert PerfSpec(6, 2, variance=True).keywords() == dict(n_perf=6, perf_r=2, perf_variance=True)
    assert PerfSpec(7, 1, False, 'taylor', True).keywords() == dict(n_perf=7, perf_r=1, perf_type='taylor',
                                                                   perf_terminal_safety=True)
    for spec in (PERF_OFF, PerfSpec(6, 2, True), PerfSpec(7, 1, False, 'taylor', True), PerfSpec(6, type='taylor')):
        assert FusedCemMpc(_Ssm(), _env(), H, 64, 8, 3, device='cpu', **spec.keywords())._perf == spec


def test_perf_spec_of_an_object_without_a_spec_is_the_off_spec():
    assert perf_spec_of(object()) is PERF_OFF
    assert perf_spec_of(mock.Mock()) is PERF_OFF                     # an injected optimiser: any attribute, no spec
    assert perf_spec_of(CemSafeMPC.__new__(CemSafeMPC)) is PERF_OFF
    assert perf_spec_of(FusedCemMpc.__new__(FusedCemMpc)) is PERF_OFF
    holder = type('Fake', (), dict(_n_perf=6, _cem_n_perf=6))()      # the loose attributes of old say nothing
    assert perf_spec_of(holder) is PERF_OFF
    spec = PerfSpec(6, 2, type='taylor')
    holder._perf = spec
    assert perf_spec_of(holder) is spec
    mpc = FusedCemMpc(_Ssm(), _env(), H, 64, 8, 3, device='cpu', n_perf=6, perf_r=2, perf_type='taylor')
    assert perf_spec_of(mpc) == spec and perf_spec_of(mpc) is mpc._perf
    assert perf_spec_of(_safempc(conf(cem_n_perf=6, cem_perf_r=2, cem_perf_type='taylor'))) == spec


CASES = [dict(), dict(n_perf=0), dict(n_perf=6), dict(n_perf=6, perf_r=2, perf_variance=True),
         dict(n_perf=6, perf_type='taylor'), dict(n_perf=7, perf_r=3, perf_type='taylor', perf_terminal_safety=True),
         dict(n_perf=7, perf_variance=True, perf_type='taylor', perf_terminal_safety=True)]


@pytest.mark.parametrize('kw', CASES)
def test_the_solver_keeps_the_spec_its_front_end_hands_down(monkeypatch, kw):
    """FusedCemMpc(**kw)._perf is the spec a CemSafeMPC built from the equivalent conf keeps, and the optimiser that front
    end builds keeps it too."""
    direct = FusedCemMpc(_Ssm(), _env(), H, 64, 8, 3, device='cpu', **kw)
    front = _safempc(conf(**{'cem_' + k: v for k, v in kw.items()}))
    assert front._perf == direct._perf == PerfSpec(**{f: kw[k] for f, k in zip(PerfSpec._fields, KEYWORD_NAMES) if k in kw})
    assert front.performance_trajectory_length == direct._perf.n_perf
    handed = {}

    class Spy(FusedCemMpc):
        def __init__(self, ssm, env, *a, **given):
            handed.update(given)
            FusedCemMpc.__init__(self, _Ssm(), env, *a, **dict(given, device='cpu'))

    monkeypatch.setattr(safempc_cem, 'FusedCemMpc', Spy)
    monkeypatch.setattr(CemSafeMPC, '_build_env', lambda self: (_env(), False))
    built = front._solver()
    assert built._perf == direct._perf and perf_spec_of(built) == perf_spec_of(front)
    assert {k: v for k, v in handed.items() if k in KEYWORD_NAMES} == direct._perf.keywords()
