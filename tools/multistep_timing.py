"""What a feedback gain per particle and step costs in the streaming rollout, and what the one launch of
`multistep_reachability` saves against the step-by-step path, on this build.

    python tools/multistep_timing.py [--repeats 7] [--launches 200] [--rollouts 1000] [--steps 5] [--stepwise-runs 3]
                                     [--out profiles/multistep_timing.jsonl]

Models: config 2's pendulum (problems.baseline_workload(2): N = 200, n_s = 2) and a cart-pole (problems.cartpole with
N = 200, n_s = 4: a training set the streaming kernel serves).  Rows (one JSON line each; printed and, with `--out`,
appended to that file):
  launch_gains     one sx_cem_rollout_gains launch against one sx_cem_rollout_starts launch (`parent_us`) on the same rows
                   (config 2's particle count; its horizon, 15, at the pendulum and 4 at the cart-pole, where every particle
                   stays finite: the row carries the launches' `status`), measured in alternation: `--repeats` rounds, each `--launches`
                   launches back to back between two synchronisations after 20 untimed ones, per launch in us.  `us` /
                   `parent_us` are the medians of the rounds, `min_us` / `max_us` the extremes of ours, `ratio` the cost of
                   the per-lane gain and its factor, `parent_spread` = (largest - smallest) / median of the parent's rounds:
                   what the ratio is read against.
  multistep_fused  `multistep_reachability` for `--rollouts` rollouts of `--steps` steps, one launch: median / min / max in ms
                   of `--repeats` x 10 synchronous calls (call + status read on the host clock) after 10 untimed ones.
  multistep_steps  the same call with the fused entry switched off (`fused_gains_form` answering -1): one
                   `onestep_reachability` per rollout and step, the only way to compute this before the entry existed.
                   Median / min / max in ms of `--stepwise-runs` calls after one untimed call; `speedup` = its median over
                   the fused median.
Needs the GPU.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import _lib, cem_mpc, problems  # noqa: E402
from safe_exploration_amd import gp_reachability_pytorch as grp  # noqa: E402

DEV = 'cuda:0'


def time_launches(fn, n, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def time_calls(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rollouts', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--stepwise-runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('multistep_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None

    def row(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    wl = problems.baseline_workload(2)
    # (under its LQR gain the cart-pole's ellipsoids outgrow double precision within ~8 steps of random actions, and lanes
    # that carry NaNs leave the eigenvalue sweeps early: 4 steps keep every particle finite, status 0 in both launches)
    models = (('cfg2_pendulum', wl.spec, wl.particles, wl.horizon), ('cartpole_n200', problems.cartpole(n_train=200), wl.particles, 4))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    for name, spec, P, H in models:
        ssm, env = problems.build(spec, device=DEV)
        n_s, n_u = spec.n_s, spec.n_u
        form = int(_lib.lib().sx_cem_rollout_gains_form(ctypes.byref(ssm.device_model), H))
        # ---- one launch against the parent variant's, same rows; every gain the environment's own, so that both do the same work
        rows = torch.cat((0.05 * rnd(1, P, n_s), 0.2 * rnd(1, P, H * n_u)), dim=2).contiguous()
        gains = torch.tensor(spec.k_fb, dtype=torch.float64, device=DEV).expand(1, P, H - 1, n_u, n_s).contiguous()
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ours = lambda: cem_mpc.cem_rollout_gains(ssm, env, H, rows=rows, gains=gains, status=status)
        parent = lambda: cem_mpc.cem_rollout_starts(ssm, env, H, rows=rows, status=status)
        a, b = [], []
        for _ in range(args.repeats):
            a.append(time_launches(parent, args.launches))
            b.append(time_launches(ours, args.launches))
        med_a, med_b = float(np.median(a)), float(np.median(b))
        row(row='launch_gains', model=name, N=int(spec.X.shape[0]), n_s=n_s, n_u=n_u, P=P, H=H, form=form, us=med_b, min_us=min(b),
            max_us=max(b), parent_us=med_a, ratio=med_b / med_a, parent_spread=(max(a) - min(a)) / med_a, repeats=args.repeats,
            launches=args.launches, status=int(status.item()))
        # ---- multistep_reachability: the one launch against the step-by-step path
        R, n = args.rollouts, args.steps
        t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)
        p_0, k_fb, k_ff = 0.05 * rnd(R, n_s), 0.1 * rnd(R, n - 1, n_u, n_s), 0.1 * rnd(R, n, n_u)
        call = lambda: grp.multistep_reachability(p_0, ssm, k_fb, k_ff, t(spec.l_mu), t(spec.l_sigma), c_safety=spec.beta,
                                                  verbose=0, a=t(spec.a), b=t(spec.b))
        fused = time_calls(call, 10 * args.repeats, 10)
        row(row='multistep_fused', model=name, N=int(spec.X.shape[0]), n_s=n_s, n_u=n_u, R=R, n=n, median_ms=float(np.median(fused)),
            min_ms=min(fused), max_ms=max(fused), runs=len(fused))
        real_form = grp.fused_gains_form
        grp.fused_gains_form = lambda ssm, n: -1
        try:
            steps = time_calls(call, args.stepwise_runs, 1)
        finally:
            grp.fused_gains_form = real_form
        row(row='multistep_steps', model=name, N=int(spec.X.shape[0]), n_s=n_s, n_u=n_u, R=R, n=n, median_ms=float(np.median(steps)),
            min_ms=min(steps), max_ms=max(steps), runs=len(steps), speedup=float(np.median(steps)) / float(np.median(fused)))


if __name__ == '__main__':
    main()
