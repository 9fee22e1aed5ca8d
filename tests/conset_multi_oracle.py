"""The inputs of the multi-model solve with a SafeMPC constraint set (test infrastructure; used by
test_conset_multi_host.py and test_gpu_conset_multi.py), beside tests/conset_oracle.py, whose rule, `cem_solve` and
settings (P, K, ITERS, H, INIT_STD) they keep: E = 3 pendulum problems that share the environment and ONE set
(`conset_oracle.pendulum_set`), each with a training set, a start state and noise draws of its own.  Problem 0 is
`conset_oracle.solve()` itself.  Computed once and left unchanged."""
import numpy as np

import conset_oracle as co
from oracle import cem as ocem
from safe_exploration_amd import _lib, problems

# (training-set size, training-set seed, start state, seed of the noise draws) per problem; problem 0: conset_oracle.solve()
PROBLEMS = ((200, 0, co.PENDULUM_X0, co.SEED),
            (100, 1, np.array([-0.03, 0.04]), co.SEED + 1),
            (37, 2, np.array([0.05, 0.01]), co.SEED + 2))
E = len(PROBLEMS)

_DONE = {}


def spec_of(e):
    n_train, seed = PROBLEMS[e][:2]
    return problems.pendulum(n_train=n_train, seed=seed, obj_mode=_lib.SX_OBJ_AFFINE_ABS)


def solves():
    """Per problem what `conset_oracle.solve` returns: (spec, set, H, x0, init_std, noise [iters x P x H x n_u], best row
    with the set, its trace, best row and trace of the same solve without the set)."""
    if 'solves' not in _DONE:
        out = [co.solve()]
        con = out[0][1]
        for e in range(1, E):
            spec, x0 = spec_of(e), PROBLEMS[e][2]
            noise = np.random.default_rng(PROBLEMS[e][3]).normal(size=(co.ITERS, co.P, co.H, spec.n_u))
            prob, gp = problems.oracle_problem(spec, ocem), co.gp_of(spec)
            best, trace = co.cem_solve(prob, con, gp, x0, noise, co.K, co.INIT_STD)
            plain_best, plain_trace = co.cem_solve(prob, None, gp, x0, noise, co.K, co.INIT_STD)
            out.append((spec, con, co.H, x0, co.INIT_STD, noise, best, trace, plain_best, plain_trace))
        _DONE['solves'] = out
    return _DONE['solves']
