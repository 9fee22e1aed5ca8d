"""Solve time of E exploration scenarios with a performance trajectory: E solves one after another against one
multi-model solve, on this build.

    python tools/perf_multi_timing.py [--shape expl|cfg2] [--scenarios 6] [--solves 100] [--warmup 10] [--sequential-only]
                                      [--taylor] [--label L] [--out F]

Shapes: `expl`, the reference's dynamic-exploration shape (20 particles, H = 2, n_perf = 5, 3 elites, 8 iterations, the
variance objective on the performance trajectory), and `cfg2`, config 2 (4096 particles, H = 15, 409 elites, 8 iterations)
with n_perf = 15; the scenarios' training sets have N = 200 - 10 e points.  Rows (one JSON line each: median and p95 in ms
of synchronous calls on the host clock, `--solves` times after `--warmup` untimed ones; printed and, with `--out`, appended
to that jsonl file):
  sequential       E FusedCemMpc(n_perf=..., perf_variance=True).solve calls one after another, then one synchronisation
  sequential_off   the same E solves without a performance trajectory (the setting off)
  multi            one MultiModelPerfCemMpc.solve
  launch_perf_multi, launch_perf_var_multi   sx_cem_perf_rollout_multi / sx_cem_perf_rollout_var_multi alone: 200 launches
                   back to back between two synchronisations, per launch, in us
`--taylor` measures the Taylor form (perf_type='taylor') in place of all of the above, with rows that mean the same on
this build and on a checkout of the commit before the multi-model Taylor launch (copy this file there):
  taylor_sequential          E FusedCemMpc(n_perf=..., perf_type='taylor').solve calls one after another
  taylor_get_actions_multi   MultiModelPerfCemMpc.from_solvers(...).get_actions_multi over those solvers: one multi-model
                             solve where the build has one, else one solve per model (`per_model_solves` says which); the
                             call ends with its own device -> host hand-off
  launch_perf_taylor_multi, launch_perf_var_multi[_ns4]   (builds with the launch only) the two launches alone at shape
                             (2, 1), and over cart-pole models of the same sizes at (4, 1), as above
`--sequential-only` stops after sequential_off and uses nothing the parent commit lacks: run the same file from a checkout of
the parent for the same-box comparison, alternating with this build (`--label` names the build in the rows).  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import _lib, cem_mpc, problems  # noqa: E402
from safe_exploration_amd.cem_mpc import FusedCemMpc  # noqa: E402

DEV = 'cuda:0'
SHAPES = {'expl': dict(P=20, H=2, n_perf=5, k=3, iters=8), 'cfg2': dict(P=4096, H=15, n_perf=15, k=409, iters=8)}


def timed(fn, warmup, n):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.percentile(ms, 95))


def time_launches(fn, n=200, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def taylor_rows(args, row, ssms, env, x0, c, kw):
    """The rows of `--taylor` (see the module's docstring)."""
    E, P, H, n_perf, k, iters = len(ssms), c['P'], c['H'], c['n_perf'], c['k'], c['iters']
    perf = dict(n_perf=n_perf, perf_r=1, perf_type='taylor')
    solvers = [FusedCemMpc(ssm, env, H, P, k, iters, seed=e, **kw, **perf) for e, ssm in enumerate(ssms)]
    med, p95 = timed(lambda: [s.solve(x0[e:e + 1]) for e, s in enumerate(solvers)], args.warmup, args.solves)
    row(row='taylor_sequential', median_ms=med, p95_ms=p95)
    multi = cem_mpc.MultiModelPerfCemMpc.from_solvers(solvers)
    n_s = x0.size(1)
    states = torch.cat([x0, torch.zeros((E, n_s * n_s), dtype=torch.float64, device=DEV)], dim=1)
    med, p95 = timed(lambda: multi.get_actions_multi(states), args.warmup, args.solves)
    row(row='taylor_get_actions_multi', median_ms=med, p95_ms=p95, fused=bool(multi.fused_applies()),
        per_model_solves=multi.per_model_solves)
    if not hasattr(cem_mpc, 'cem_perf_rollout_taylor_multi'):
        return
    # the launches alone: Taylor beside variance, at (2, 1) and over cart-pole models of the same sizes at (4, 1)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64, device=DEV)
    status = torch.zeros(E, dtype=torch.int32, device=DEV)
    built4 = [problems.build(problems.cartpole(n_train=int(s.device_model.n_train), seed=2 + e), device=DEV)
              for e, s in enumerate(ssms)]
    env4 = _lib.SxEnv.from_buffer_copy(built4[0][1])
    env4.obj_mode = _lib.SX_OBJ_NEG_VARIANCE
    for suffix, models, e_, x in (('', ssms, env, x0), ('_ns4', [b[0] for b in built4], env4, full(0, E, 4))):
        bufs = dict(safe_actions=0.1 * rnd(E, P, H, 1), obj_cost=full(0, E, P), con_cost=full(0, E, P), status=status,
                    tail_mean=full(0, E, n_perf - 1, 1), tail_std=full(0.1, E, n_perf - 1, 1),
                    tail_noise=rnd(E, P, n_perf - 1, 1), table=cem_mpc.GpModelTable())
        row(row='launch_perf_taylor_multi' + suffix, us=time_launches(
            lambda: cem_mpc.cem_perf_rollout_taylor_multi(models, e_, x, H, n_perf, 1, **bufs)))
        row(row='launch_perf_var_multi' + suffix, us=time_launches(
            lambda: cem_mpc.cem_perf_rollout_multi(models, e_, x, H, n_perf, 1, variance=True, **bufs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--shape', default='expl', choices=sorted(SHAPES))
    ap.add_argument('--scenarios', type=int, default=6)
    ap.add_argument('--solves', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--sequential-only', action='store_true')
    ap.add_argument('--taylor', action='store_true')
    ap.add_argument('--label', default='this')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('perf_multi_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None
    c, E = SHAPES[args.shape], args.scenarios
    P, H, n_perf, k, iters = c['P'], c['H'], c['n_perf'], c['k'], c['iters']

    def row(**kw):
        line = json.dumps(dict(workload=args.shape, build=args.label, E=E, P=P, H=H, n_perf=n_perf, iters=iters,
                               solves=args.solves, **kw))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    specs = [problems.pendulum(n_train=200 - 10 * e, seed=e) for e in range(E)]     # the variance objective
    built = [problems.build(s, device=DEV) for s in specs]
    ssms, env = [b[0] for b in built], built[0][1]
    x0 = torch.tensor(problems.start_states(2, E, seed=5, std=0.03), dtype=torch.float64, device=DEV)
    kw = dict(device=DEV, init_std=0.2)
    if args.taylor:
        return taylor_rows(args, row, ssms, env, x0, c, kw)
    perf = dict(n_perf=n_perf, perf_r=1, perf_variance=True)
    for name, extra in (('sequential', perf), ('sequential_off', {})):
        solvers = [FusedCemMpc(ssm, env, H, P, k, iters, seed=e, **kw, **extra) for e, ssm in enumerate(ssms)]
        med, p95 = timed(lambda: [s.solve(x0[e:e + 1]) for e, s in enumerate(solvers)], args.warmup, args.solves)
        row(row=name, median_ms=med, p95_ms=p95)
    if args.sequential_only:
        return
    multi = cem_mpc.MultiModelPerfCemMpc(ssms, env, H, P, k, iters, **kw, **perf)
    assert multi.fused_applies()
    med, p95 = timed(lambda: multi.solve(x0), args.warmup, args.solves)
    row(row='multi', median_ms=med, p95_ms=p95)
    # the launches alone
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64, device=DEV)
    status = torch.zeros(E, dtype=torch.int32, device=DEV)
    safety = cem_mpc.cem_rollout_multi(ssms, env, x0, H, mean=full(0, E, H, 1), std=full(0.2, E, H, 1), noise=rnd(E, P, H, 1),
                                       status=status)
    tail = dict(tail_mean=full(0, E, n_perf - 1, 1), tail_std=full(0.2, E, n_perf - 1, 1), tail_noise=rnd(E, P, n_perf - 1, 1))
    env_abs = _lib.SxEnv.from_buffer_copy(env)
    env_abs.obj_mode = _lib.SX_OBJ_AFFINE_ABS
    for name, variance, e_, table in (('launch_perf_multi', False, env_abs, cem_mpc.PerfModelTable()),
                                      ('launch_perf_var_multi', True, env, cem_mpc.GpModelTable())):
        row(row=name, us=time_launches(lambda: cem_mpc.cem_perf_rollout_multi(
            ssms, e_, x0, H, n_perf, 1, variance=variance, safe_actions=safety['actions'], obj_cost=safety['obj_cost'],
            con_cost=safety['con_cost'], status=status, table=table, **tail)))


if __name__ == '__main__':
    main()
