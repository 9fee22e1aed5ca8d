"""Launch and solve time of Cautious MPC against the Taylor performance rollout of equal length, in one process: config 2's
model (pendulum, N = 200, 4096 particles).

    python tools/cautious_timing.py [--steps 10,20] [--solve-steps 10] [--repeats 7] [--launches 200] [--solves 100]
                                    [--warmup 20] [--out profiles/cautious_timing.jsonl]

Rows (one JSON line each; printed and, with `--out`, appended to that jsonl file):
  launch_taylor_T     sx_cem_perf_rollout_taylor at n_perf = T + 1, r = 1, H = 1: the same GP work per step as a cautious
                      launch of T steps plus one step; `--launches` launches back to back between two synchronisations, per
                      launch in us; the median, the smallest and the largest of `--repeats` such measurements
  launch_cautious_T   sx_cem_cautious_rollout at T steps, propagate 1, measured the same way in alternation with the Taylor
                      launch; `ratio` = median / the Taylor median, `ratio_per_step` the same per GP step (T against T + 1),
                      `taylor_spread` = (largest - smallest) / median of the Taylor launch: the run-to-run spread a ratio is
                      read against
  launch_cautious_me_T  the same with propagate 0
  solve_cautious_T    a CautiousCemMpc solve (config 2's particles, elites and iterations) at T = --solve-steps: median and
                      p95 in ms of `--solves` synchronous solves after `--warmup` untimed ones
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

from safe_exploration_amd import cem_mpc, problems  # noqa: E402
from safe_exploration_amd.cem_mpc import CautiousCemMpc  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', default='10,20')
    ap.add_argument('--solve-steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--solves', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cautious_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None
    wl = problems.baseline_workload(2)
    ssm, env = problems.build(wl.spec, device=DEV)
    P = wl.particles
    x0 = torch.tensor(wl.x0[:1, :wl.spec.n_s], dtype=torch.float64, device=DEV)

    def row(**kw):
        line = json.dumps(dict(workload='cfg2 model', N=int(wl.spec.X.shape[0]), P=P, **kw))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for steps in [int(s) for s in args.steps.split(',')]:
        full = lambda v: torch.full((1, steps, 1), v, dtype=torch.float64, device=DEV)
        mean, std = full(0.0), full(wl.init_std)
        noise = torch.randn((1, P, steps, 1), dtype=torch.float64, device=DEV, generator=gen)
        safe = (std[:, :1, None] * noise[:, :, :1]).contiguous()
        obj, con = torch.zeros((1, P), dtype=torch.float64, device=DEV), torch.zeros((1, P), dtype=torch.float64, device=DEV)
        taylor = lambda: cem_mpc.cem_perf_rollout_taylor(ssm, env, x0, 1, steps + 1, 1, safe_actions=safe, obj_cost=obj,
                                                         con_cost=con, status=status, tail_mean=mean, tail_std=std,
                                                         tail_noise=noise)
        cautious = lambda propagate: (lambda: cem_mpc.cem_cautious_rollout(ssm, env, x0, steps, mean=mean, std=std, noise=noise,
                                                                           propagate=propagate, status=status))
        kinds = (('taylor', taylor), ('cautious', cautious(True)), ('cautious_me', cautious(False)))
        us = {name: [] for name, _ in kinds}
        for _ in range(args.repeats):
            for name, fn in kinds:                      # in alternation: a drift of the clocks meets all three alike
                us[name].append(time_launches(fn, args.launches, args.warmup))
        med = {name: float(np.median(v)) for name, v in us.items()}
        spread = (max(us['taylor']) - min(us['taylor'])) / med['taylor']
        row(row=f'launch_taylor_{steps}', n_perf=steps + 1, r=1, us=med['taylor'], us_min=min(us['taylor']),
            us_max=max(us['taylor']), repeats=args.repeats, launches=args.launches)
        for name in ('cautious', 'cautious_me'):
            row(row=f'launch_{name}_{steps}', T=steps, us=med[name], us_min=min(us[name]), us_max=max(us[name]),
                ratio=med[name] / med['taylor'], ratio_per_step=med[name] / steps / (med['taylor'] / (steps + 1)),
                taylor_spread=spread, repeats=args.repeats, launches=args.launches)
    mpc = CautiousCemMpc(ssm, env, args.solve_steps, P, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)
    for _ in range(args.warmup):
        mpc.solve(x0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.solves):
        t0 = time.perf_counter()
        mpc.solve(x0)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    row(row=f'solve_cautious_{args.solve_steps}', T=args.solve_steps, iters=wl.iterations, elites=wl.elites,
        median_ms=float(np.median(ms)), p95_ms=float(np.percentile(ms, 95)), solves=args.solves)


if __name__ == '__main__':
    main()
