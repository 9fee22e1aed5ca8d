"""CPU: the streaming LDS rule behind every exact-GP form query -- all outputs in LDS if they fit beside the tile's actions,
else output by output for n_s > 1, else no form; n_pad <= 1024 (csrc/sx_stream_launch.hpp).  The safety entries
(sx_cem_rollout_starts_form, sx_cem_rollout_sat_form, sx_cem_rollout_multi_form) and the performance entries
(sx_cem_perf_rollout_var[_multi]_form) answer alike; the Taylor and cautious queries answer the same rule with their step
constants behind the actions; and every multi-model query folds its models' single answers the same way.  No device access:
the models carry fake non-null buffers, which no query dereferences."""
import ctypes
import os

import pytest

from safe_exploration_amd import _lib
from test_static_explore_host import form_rule

pytestmark = pytest.mark.skipif(bool(os.environ.get('SX_ROLLOUT')), reason='SX_ROLLOUT forces a form')

SX_FORM_STREAM, SX_FORM_BYOUT = 0, 3   # include/sx_amd.h
SHAPES = [(1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2), (3, 2)]
COMPILED = SHAPES[:-1]                 # (3, 2) has a junk-dimension kernel only: no query shift 0 in SX_ROLLOUT_SHAPES
STEPS = (2, 3, 15, 40, 400)
SIZES = list(range(1, 1200, 13)) + [2000]


def _model(n_s, n_u, n_train):
    m = _lib.SxGpModel()
    m.n_s, m.n_u, m.n_train = n_s, n_u, n_train
    m.n_pad = (n_train + 1 + n_s + n_u + 15) // 16 * 16   # sx_gp.hpp: gp_n_pad
    m.x_train = m.a_pack = m.stage_tab = 0x1000             # never dereferenced
    return m


def _models(n_s, n_u, sizes):
    return (_lib.SxGpModel * len(sizes))(*[_model(n_s, n_u, n) for n in sizes])


def taylor_extra_bytes(n_s, n_u, cautious=False):
    """The step constants the Taylor kernels keep in LDS behind the tile's actions; the cautious kernel adds beta."""
    M = _lib.SX_MAX_M
    return (2 * n_s * n_s + 2 * n_s * n_u + 2 * n_u + 3 * n_s + M * n_s + M) * 8 + (8 if cautious else 0)


def rule_with_extra(n_s, n_u, n_pad, steps, extra_bytes):
    """form_rule with `extra_bytes` more LDS: the rule counts 16 * steps * n_u doubles of actions, so the bytes enter as
    extra_bytes / (128 n_u) further steps -- a dyadic fraction for n_u = 1, 2, exact in floating point."""
    assert n_u in (1, 2) and extra_bytes % 8 == 0
    if (n_s, n_u) not in COMPILED:
        return -1
    return form_rule(n_s, n_u, n_pad, steps + extra_bytes / (128 * n_u))


@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_the_five_plain_form_queries_agree(n_s, n_u):
    lib = _lib.lib()
    seen = set()
    for steps in STEPS:
        for N in SIZES:
            one = _models(n_s, n_u, [N])
            m = ctypes.byref(one[0])
            answers = [int(lib.sx_cem_rollout_starts_form(m, steps)), int(lib.sx_cem_rollout_sat_form(m, steps)),
                       int(lib.sx_cem_rollout_multi_form(one, 1, steps)), int(lib.sx_cem_perf_rollout_var_form(m, steps)),
                       int(lib.sx_cem_perf_rollout_var_multi_form(one, 1, steps))]
            assert len(set(answers)) == 1, (N, steps, answers)
            assert answers[0] == rule_with_extra(n_s, n_u, one[0].n_pad, steps, 0), (N, steps)
            seen.add(answers[0])
    want = {-1} if (n_s, n_u) not in COMPILED else {SX_FORM_STREAM, -1} if n_s == 1 else {SX_FORM_STREAM, SX_FORM_BYOUT, -1}
    assert seen == want


@pytest.mark.parametrize('n_s,n_u', SHAPES)
def test_taylor_and_cautious_queries_follow_the_rule_with_their_extra_bytes(n_s, n_u):
    lib = _lib.lib()
    seen = set()
    for steps in STEPS:
        for N in SIZES:
            one = _models(n_s, n_u, [N])
            m = ctypes.byref(one[0])
            taylor = rule_with_extra(n_s, n_u, one[0].n_pad, steps, taylor_extra_bytes(n_s, n_u))
            cautious = rule_with_extra(n_s, n_u, one[0].n_pad, steps, taylor_extra_bytes(n_s, n_u, cautious=True))
            assert int(lib.sx_cem_perf_rollout_taylor_form(m, steps)) == taylor, (N, steps)
            assert int(lib.sx_cem_perf_rollout_taylor_multi_form(one, 1, steps)) == taylor, (N, steps)
            assert int(lib.sx_cem_cautious_rollout_form(m, steps)) == cautious, (N, steps)
            seen |= {taylor, cautious}
    want = {-1} if (n_s, n_u) not in COMPILED else {SX_FORM_STREAM, -1} if n_s == 1 else {SX_FORM_STREAM, SX_FORM_BYOUT, -1}
    assert seen == want


def test_the_extra_bytes_move_an_answer():
    """At least one grid point answers differently with the step constants in LDS: the test above is not the plain rule's."""
    moved = [(s, N) for s in COMPILED for N in range(1, 1200) for n_pad in [_model(*s, N).n_pad]
             if form_rule(*s, n_pad, 15) != rule_with_extra(*s, n_pad, 15, taylor_extra_bytes(*s))]
    assert moved


MULTI_QUERIES = [('sx_cem_rollout_multi_form', 'sx_cem_rollout_starts_form'),
                 ('sx_cem_perf_rollout_var_multi_form', 'sx_cem_perf_rollout_var_form'),
                 ('sx_cem_perf_rollout_taylor_multi_form', 'sx_cem_perf_rollout_taylor_form')]


@pytest.mark.parametrize('multi,single', MULTI_QUERIES, ids=[q[0] for q in MULTI_QUERIES])
def test_multi_queries_fold_the_single_answers(multi, single):
    lib = _lib.lib()
    folds = set()
    for (n_s, n_u), sizes in (((2, 1), (60, 200, 560, 700, 1000, 1100, 2000)), ((4, 1), (60, 128, 260, 400, 590, 700)),
                              ((2, 2), (60, 300, 500, 900, 1100)), ((3, 1), (77, 300, 500, 1200)), ((1, 1), (40, 900, 1100))):
        for steps in (3, 15, 40):
            for N in sizes:
                for others in ((), (60,), (60, 200), (sizes[-2], 60)):
                    ms = _models(n_s, n_u, others + (N,))
                    singles = [int(getattr(lib, single)(ctypes.byref(ms[i]), steps)) for i in range(len(ms))]
                    want = -1 if -1 in singles else SX_FORM_BYOUT if SX_FORM_BYOUT in singles else SX_FORM_STREAM
                    assert int(getattr(lib, multi)(ms, len(ms), steps)) == want, (n_s, n_u, steps, others, N, singles)
                    if len(set(singles)) > 1:
                        folds.add((want, tuple(sorted(set(singles)))))
    # mixed sets of every kind were among them: BYOUT beside STREAM, and a model without a form beside either
    assert (SX_FORM_BYOUT, (SX_FORM_STREAM, SX_FORM_BYOUT)) in folds
    assert (-1, (-1, SX_FORM_STREAM)) in folds and any(f[0] == -1 and SX_FORM_BYOUT in f[1] for f in folds)
