"""Solve time with and without the performance trajectory, on this build: config 2 (pendulum, N = 200, 4096 particles,
H = 15, 8 CEM iterations, 409 elites).

    python tools/perf_traj_timing.py [--n-perf 15,30,45] [--solves 200] [--warmup 20] [--off-only] [--variance] [--taylor]
                                     [--label L] [--out F]

Rows (one JSON line each: median and p95 in ms of synchronous solves -- FusedCemMpc.solve + device synchronise on the host
clock -- `--solves` times after `--warmup` untimed ones; printed and, with `--out`, appended to that jsonl file):
  off_cfg2        config 2 as bench.py runs it (the variance objective), the setting absent
  off             the same with the pendulum's |theta_target - theta| objective, which the performance trajectory needs
  off_H30         safety horizon 30, no performance trajectory: what a 30-step look-ahead costs without the setting
  n_perf=K        H = 15 with a performance trajectory of K steps (r = 1), for every K of --n-perf; `extra_ms` is the
                  difference to `off`
  launch_safety, launch_perf_K   one launch alone (sx_cem_rollout at H = 15; sx_cem_perf_rollout at n_perf = K): 200
                  launches back to back between two synchronisations, per launch, in us
`--variance` adds, for every K: `n_perf=K var_affine` (perf_variance=True with the same objective: the cost of the variance
kernel alone), `n_perf=K var` (perf_variance=True over config 2's own variance objective; `extra_ms` against off_cfg2) and
`launch_perf_var_K` (sx_cem_perf_rollout_var alone).
`--taylor` adds, for every K: `n_perf=K taylor` (perf_type='taylor' over config 2's variance objective; `extra_ms` against
off_cfg2), `launch_perf_taylor_K` (sx_cem_perf_rollout_taylor alone) and, on a cart-pole model of the same N (shape (4, 1),
where the owner lanes' tail is 8 x the FMAs), `launch_perf_var_ns4_K` / `launch_perf_taylor_ns4_K`.
`--off-only` stops after off_H30 and uses nothing the parent commit lacks: run the same file from a checkout of the parent for
the same-session comparison (`--label` names the build in the rows).  Needs the GPU.
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


def time_solves(mpc, x0, warmup, solves):
    for _ in range(warmup):
        mpc.solve(x0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(solves):
        t0 = time.perf_counter()
        mpc.solve(x0)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--n-perf', default='15,30,45')
    ap.add_argument('--solves', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--off-only', action='store_true')
    ap.add_argument('--variance', action='store_true')
    ap.add_argument('--taylor', action='store_true')
    ap.add_argument('--label', default='this')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('perf_traj_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None
    wl = problems.baseline_workload(2)
    x0 = torch.tensor(wl.x0[:1, :wl.spec.n_s], dtype=torch.float64, device=DEV)

    def row(**kw):
        line = json.dumps(dict(workload='cfg2', build=args.label, P=wl.particles, iters=wl.iterations, solves=args.solves,
                               **kw))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    def solver(ssm, env, H, **kw):
        return FusedCemMpc(ssm, env, H, wl.particles, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std, **kw)

    ssm, env_var = problems.build(wl.spec, device=DEV)
    off_cfg2, p95 = time_solves(solver(ssm, env_var, wl.horizon), x0, args.warmup, args.solves)
    row(row='off_cfg2', H=wl.horizon, n_perf=0, median_ms=off_cfg2, p95_ms=p95)
    spec = problems.pendulum(wl.spec.X.shape[0], seed=0, obj_mode=_lib.SX_OBJ_AFFINE_ABS)
    ssm, env = problems.build(spec, device=DEV)
    off, p95 = time_solves(solver(ssm, env, wl.horizon), x0, args.warmup, args.solves)
    row(row='off', H=wl.horizon, n_perf=0, median_ms=off, p95_ms=p95)
    med, p95 = time_solves(solver(ssm, env, 30), x0, args.warmup, args.solves)
    row(row='off_H30', H=30, n_perf=0, median_ms=med, p95_ms=p95)
    if args.off_only:
        return
    H, P = wl.horizon, wl.particles
    ks = [int(k) for k in args.n_perf.split(',')]
    for k in ks:
        med, p95 = time_solves(solver(ssm, env, H, n_perf=k, perf_r=1), x0, args.warmup, args.solves)
        row(row=f'n_perf={k}', H=H, n_perf=k, r=1, median_ms=med, p95_ms=p95, extra_ms=med - off,
            extra_per_iteration_us=(med - off) * 1e3 / wl.iterations)
        if args.variance:
            for name, e, base in (('var_affine', env, off), ('var', env_var, off_cfg2)):
                med, p95 = time_solves(solver(ssm, e, H, n_perf=k, perf_r=1, perf_variance=True), x0, args.warmup, args.solves)
                row(row=f'n_perf={k} {name}', H=H, n_perf=k, r=1, median_ms=med, p95_ms=p95, extra_ms=med - base,
                    extra_per_iteration_us=(med - base) * 1e3 / wl.iterations)
        if args.taylor:
            med, p95 = time_solves(solver(ssm, env_var, H, n_perf=k, perf_r=1, perf_type='taylor'), x0, args.warmup,
                                   args.solves)
            row(row=f'n_perf={k} taylor', H=H, n_perf=k, r=1, median_ms=med, p95_ms=p95, extra_ms=med - off_cfg2,
                extra_per_iteration_us=(med - off_cfg2) * 1e3 / wl.iterations)
    # the launches alone
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    mean, std, noise = torch.zeros((1, H, 1), dtype=torch.float64, device=DEV), torch.full((1, H, 1), wl.init_std,
                                                                                           dtype=torch.float64, device=DEV), rnd(1, P, H, 1)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    safety = cem_mpc.cem_rollout(ssm, env, x0, H, mean=mean, std=std, noise=noise, status=status)
    row(row='launch_safety', H=H, us=time_launches(
        lambda: cem_mpc.cem_rollout(ssm, env, x0, H, mean=mean, std=std, noise=noise, status=status)))
    for k in ks:
        t_mean, t_std = torch.zeros((1, k - 1, 1), dtype=torch.float64, device=DEV), torch.full((1, k - 1, 1), wl.init_std,
                                                                                                dtype=torch.float64, device=DEV)
        t_noise = rnd(1, P, k - 1, 1)
        row(row=f'launch_perf_{k}', H=H, n_perf=k, r=1, us=time_launches(
            lambda: cem_mpc.cem_perf_rollout(ssm, env, x0, H, k, 1, safe_actions=safety['actions'],
                                             obj_cost=safety['obj_cost'], con_cost=safety['con_cost'], status=status,
                                             tail_mean=t_mean, tail_std=t_std, tail_noise=t_noise)))
        if args.variance:
            row(row=f'launch_perf_var_{k}', H=H, n_perf=k, r=1, us=time_launches(
                lambda: cem_mpc.cem_perf_rollout_var(ssm, env_var, x0, H, k, 1, safe_actions=safety['actions'],
                                                     obj_cost=safety['obj_cost'], con_cost=safety['con_cost'], status=status,
                                                     tail_mean=t_mean, tail_std=t_std, tail_noise=t_noise)))
        if args.taylor:
            row(row=f'launch_perf_taylor_{k}', H=H, n_perf=k, r=1, us=time_launches(
                lambda: cem_mpc.cem_perf_rollout_taylor(ssm, env_var, x0, H, k, 1, safe_actions=safety['actions'],
                                                        obj_cost=safety['obj_cost'], con_cost=safety['con_cost'],
                                                        status=status, tail_mean=t_mean, tail_std=t_std, tail_noise=t_noise)))
    if args.taylor:
        # shape (4, 1): the same N and particles over a cart-pole model, the two launches alone
        spec4 = problems.cartpole(n_train=wl.spec.X.shape[0])
        ssm4, env4 = problems.build(spec4, device=DEV)
        env4 = _lib.SxEnv.from_buffer_copy(env4)
        env4.obj_mode = _lib.SX_OBJ_NEG_VARIANCE
        x4 = torch.zeros((1, 4), dtype=torch.float64, device=DEV)
        safe4 = dict(actions=0.1 * rnd(1, P, H, 1), obj_cost=torch.zeros((1, P), dtype=torch.float64, device=DEV),
                     con_cost=torch.zeros((1, P), dtype=torch.float64, device=DEV))
        for k in ks:
            t_mean = torch.zeros((1, k - 1, 1), dtype=torch.float64, device=DEV)
            t_std, t_noise = torch.full_like(t_mean, 0.1), rnd(1, P, k - 1, 1)
            for name, fn in (('var', cem_mpc.cem_perf_rollout_var), ('taylor', cem_mpc.cem_perf_rollout_taylor)):
                row(row=f'launch_perf_{name}_ns4_{k}', H=H, n_perf=k, r=1, us=time_launches(
                    lambda: fn(ssm4, env4, x4, H, k, 1, safe_actions=safe4['actions'], obj_cost=safe4['obj_cost'],
                               con_cost=safe4['con_cost'], status=status, tail_mean=t_mean, tail_std=t_std,
                               tail_noise=t_noise)))


if __name__ == '__main__':
    main()
