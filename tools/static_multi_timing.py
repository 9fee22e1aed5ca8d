"""Launch and solve time of static exploration over several scenarios: ONE multi-model launch / solve for all of them against
one per scenario, in one process ("the multi-model form").

    python tools/static_multi_timing.py [--scenarios 6] [--shapes 20x20x3,1x4096x400] [--iters 8] [--horizon 3]
                                        [--repeats 7] [--launches 200] [--solves 30] [--warmup 10]
                                        [--out profiles/static_multi_timing.jsonl]

`--scenarios` GPs with data and hyper-parameters of their own over the pendulum (N = 200 - 10 s) and over a cart-pole model of
the same sizes; per shape RxPxk: R restarts of P rows with k elites (the reference's CEM shape with n_restarts_optimizer = 20,
and 4096 rows with one restart, where one problem fills the chip).  Rows (one JSON line each; printed and, with `--out`,
appended to that file):
  launch_multi        ONE sx_cem_rollout_starts_multi launch over the S R problems: `--launches` launches back to back between
                      two synchronisations, per launch in us; the median, the smallest and the largest of `--repeats` such
                      measurements
  launch_sequential   one sx_cem_rollout_starts launch (E = R) per scenario, S in a row, measured in alternation with it;
                      `speedup` = sequential / multi (below 1: the single launch is slower)
  solve_multi         MultiModelStaticCemMpc.find over the scenarios' StaticCemMpc: the median of `--solves` synchronous finds in
                      ms; the median, the smallest and the largest of `--repeats` such measurements
  solve_sequential    every scenario's StaticCemMpc.find in turn, measured in alternation with it; `speedup`
Needs the GPU.
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
from safe_exploration_amd.cem_mpc import GpModelTable, MultiModelStaticCemMpc, StaticCemMpc  # noqa: E402

DEV = 'cuda:0'


def time_launches(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def time_solves(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--scenarios', type=int, default=6)
    ap.add_argument('--shapes', default='20x20x3,1x4096x400', help='RxPxk per measured shape')
    ap.add_argument('--iters', type=int, default=8)
    ap.add_argument('--horizon', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--solves', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('static_multi_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None

    def row(**kw):
        line = json.dumps(dict(workload='static multi', **kw))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    S, H = args.scenarios, args.horizon
    sizes = [200 - 10 * s for s in range(S)]
    families = (('pendulum', [problems.pendulum(n_train=n, seed=s) for s, n in enumerate(sizes)]),
                ('cartpole', [problems.cartpole(n_train=n, seed=2 + s) for s, n in enumerate(sizes)]))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    for family, specs in families:
        for s, spec in enumerate(specs):       # hyper-parameters of their own
            spec.lengthscale, spec.outputscale = spec.lengthscale * (0.8 + 0.1 * s), spec.outputscale * (1.0 + 0.1 * s)
        built = [problems.build(spec, device=DEV) for spec in specs]
        ssms, env = [b[0] for b in built], _lib.SxEnv.from_buffer_copy(built[0][1])
        env.obj_mode = _lib.SX_OBJ_NEG_VARIANCE
        n_s, n_u = specs[0].n_s, specs[0].n_u
        L = n_s + H * n_u
        for shape in args.shapes.split(','):
            R, P, k = (int(v) for v in shape.split('x'))
            E = S * R
            info = dict(model=family, S=S, R=R, N=sizes, P=P, H=H)
            mean = torch.zeros((E, L), dtype=torch.float64, device=DEV)
            std = torch.cat([torch.full((E, n_s), 0.05, dtype=torch.float64, device=DEV),
                             torch.full((E, H * n_u), 0.3, dtype=torch.float64, device=DEV)], dim=1).contiguous()
            noise = torch.randn((E, P, L), dtype=torch.float64, device=DEV, generator=gen)
            repeated = [ssm for ssm in ssms for _ in range(R)]
            table = GpModelTable()
            st_e, st_1 = torch.zeros(E, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            per = [tuple(t[s * R:(s + 1) * R].contiguous() for t in (mean, std, noise)) for s in range(S)]

            def multi():
                cem_mpc.cem_rollout_starts_multi(repeated, env, H, mean=mean, std=std, noise=noise, status=st_e, table=table)

            def sequential():
                for s in range(S):
                    m, sd, z = per[s]
                    cem_mpc.cem_rollout_starts(ssms[s], env, H, mean=m, std=sd, noise=z, status=st_1)

            kinds = (('multi', multi), ('sequential', sequential))
            us = {name: [] for name, _ in kinds}
            for _ in range(args.repeats):
                for name, fn in kinds:                  # in alternation: a drift of the clocks meets both alike
                    us[name].append(time_launches(fn, args.launches, args.warmup))
            med = {name: float(np.median(v)) for name, v in us.items()}
            stats = lambda name: dict(us=med[name], us_min=min(us[name]), us_max=max(us[name]), repeats=args.repeats,
                                      launches=args.launches)
            row(row='launch_multi', **info, **stats('multi'))
            row(row='launch_sequential', **info, **stats('sequential'), speedup=med['sequential'] / med['multi'])
            solvers = [StaticCemMpc(ssm, env, H, P, k, args.iters, start_mean=np.zeros(n_s), start_std=np.full(n_s, 0.05),
                                    n_restarts=R, seed=100 * s, init_std=0.3, device=DEV) for s, ssm in enumerate(ssms)]
            mpc = MultiModelStaticCemMpc.from_solvers(solvers)
            assert mpc.fused_applies()
            kinds = (('multi', mpc.find), ('sequential', lambda: [s.find() for s in solvers]))
            ms = {name: [] for name, _ in kinds}
            for _ in range(args.repeats):
                for name, fn in kinds:
                    ms[name].append(time_solves(fn, args.solves, args.warmup))
            med = {name: float(np.median(v)) for name, v in ms.items()}
            stats = lambda name: dict(median_ms=med[name], ms_min=min(ms[name]), ms_max=max(ms[name]), repeats=args.repeats,
                                      solves=args.solves, iters=args.iters, elites=k)
            row(row='solve_multi', **info, **stats('multi'), per_model_solves=mpc.per_model_solves,
                stepwise_fallbacks=mpc.stepwise_fallbacks)
            row(row='solve_sequential', **info, **stats('sequential'), speedup=med['sequential'] / med['multi'])


if __name__ == '__main__':
    main()
