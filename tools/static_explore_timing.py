"""Solve time of static exploration (StaticCemMpc: the start state is optimised with the actions) against a plain solve on
the streaming kernel, on this build: config 2 (pendulum, N = 200, 4096 particles, H = 15, 8 CEM iterations, 409 elites).

    python tools/static_explore_timing.py [--restarts 1,6] [--solves 200] [--warmup 20] [--plain-only] [--label L] [--out F]
                                          [--repeats 5]

Rows (one JSON line each: median and p95 in ms of synchronous solves -- solve + device synchronise on the host clock --
`--solves` times after `--warmup` untimed ones; printed and, with `--out`, appended to that jsonl file):
  plain_stream     FusedCemMpc.solve with the rollout forced onto the streaming kernel (this tool sets SX_ROLLOUT=stream
                   before the library loads): the kernel a static solve runs, without the start entries.  The elite refit
                   then runs in the rollout's prologue.
  plain_stream_E   the same for E problems at once (every E > 1 of --restarts), the comparison for that many restarts
  static_E         StaticCemMpc.solve with n_restarts = E, for every E of --restarts; `extra_ms` is the difference to the
                   plain solve of the same E: n_s more row entries in the ranking, the refit in the ranking launch, the
                   start's draw and polytope test in the rollout
  launch_plain, launch_starts   one launch alone (sx_cem_rollout on the streaming kernel; sx_cem_rollout_starts): 200
                   launches back to back between two synchronisations, per launch, in us
  static_cons_E    StaticCemMpc(con_set=...).solve with a full set (the feedback bounds and two obstacle rows, as
                   tools/conset_timing.py builds them), measured in alternation with the same solver without the set,
                   `--repeats` rounds of `--solves` / `--repeats` solves each: the median of the rounds' medians, `parent_ms`
                   likewise for the solver without the set, `ratio` = median / parent's, `parent_spread` = (largest - smallest)
                   / median of the parent's rounds: what a ratio is read against
  launch_starts_cons   sx_cem_rollout_starts_cons with that set on launch_starts' buffers, in the same alternation with
                   sx_cem_rollout_starts (`parent_us`): median, smallest and largest of `--repeats` measurements
A static solve is the streaming kernel plus the longer rows, so it is compared with plain_stream, not with the resident form
a plain config-2 solve takes by default.  `--plain-only` stops after the plain rows and uses nothing the parent commit
lacks: run the same file from a checkout of the parent for the same-session comparison (`--label` names the build in the
rows).  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

os.environ['SX_ROLLOUT'] = 'stream'      # read once, when the library plans its first rollout

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import cem_mpc, problems  # noqa: E402
from safe_exploration_amd.cem_mpc import FusedCemMpc  # noqa: E402

DEV = 'cuda:0'


def time_solves(solve, warmup, solves):
    for _ in range(warmup):
        solve()
    torch.cuda.synchronize()
    ms = []
    for _ in range(solves):
        t0 = time.perf_counter()
        solve()
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
    ap.add_argument('--restarts', default='1,6')
    ap.add_argument('--solves', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--label', default='this')
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('static_explore_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None
    wl = problems.baseline_workload(2)
    n_s = wl.spec.n_s
    H, P = wl.horizon, wl.particles

    def row(**kw):
        line = json.dumps(dict(workload='cfg2', build=args.label, P=P, H=H, iters=wl.iterations, solves=args.solves, **kw))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    ssm, env = problems.build(wl.spec, device=DEV)
    restarts = [int(e) for e in args.restarts.split(',')]
    plain = {}
    for E in sorted(set([1] + restarts)):
        x0 = torch.tensor(np.repeat(wl.x0[:1, :n_s], E, axis=0), dtype=torch.float64, device=DEV)
        mpc = FusedCemMpc(ssm, env, H, P, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)
        plain[E], p95 = time_solves(lambda: mpc.solve(x0), args.warmup, args.solves)
        row(row='plain_stream' if E == 1 else f'plain_stream_{E}', E=E, median_ms=plain[E], p95_ms=p95)
    if args.plain_only:
        return
    for E in restarts:
        mpc = cem_mpc.StaticCemMpc(ssm, env, H, P, wl.elites, wl.iterations, start_mean=wl.x0[0, :n_s],
                                   start_std=np.full(n_s, 0.05), n_restarts=E, init_std=wl.init_std, device=DEV)
        med, p95 = time_solves(mpc.solve, args.warmup, args.solves)
        row(row=f'static_{E}', E=E, median_ms=med, p95_ms=p95, extra_ms=med - plain[E],
            extra_per_iteration_us=(med - plain[E]) * 1e3 / wl.iterations)
    # the constraint set: the feedback bounds, and the first two rows of the safe polytope pulled in as the obstacle
    from safe_exploration_amd.gp_reachability_pytorch import make_con_set
    con_set = make_con_set(n_s, h_mat_obs=wl.spec.h_mat[:2], h_obs=0.9 * wl.spec.h_vec[:2, 0], ctrl_ellipsoid=True)

    def alternate(parent, ours, measure):
        a, b = [], []
        for _ in range(args.repeats):
            a.append(measure(parent))
            b.append(measure(ours))
        med = float(np.median(a))
        return dict(parent=med, ours=float(np.median(b)), lo=float(min(b)), hi=float(max(b)), ratio=float(np.median(b)) / med,
                    parent_spread=(max(a) - min(a)) / med)

    per_round = max(1, args.solves // args.repeats)
    for E in restarts:
        kw = dict(start_mean=wl.x0[0, :n_s], start_std=np.full(n_s, 0.05), n_restarts=E, init_std=wl.init_std, device=DEV)
        without = cem_mpc.StaticCemMpc(ssm, env, H, P, wl.elites, wl.iterations, **kw)
        with_set = cem_mpc.StaticCemMpc(ssm, env, H, P, wl.elites, wl.iterations, con_set=con_set, **kw)
        m = alternate(without.solve, with_set.solve, lambda solve: time_solves(solve, args.warmup, per_round)[0])
        row(row=f'static_cons_{E}', E=E, median_ms=m['ours'], min_ms=m['lo'], max_ms=m['hi'], parent_ms=m['parent'],
            ratio=m['ratio'], parent_spread=m['parent_spread'], repeats=args.repeats)
    # the launches alone
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    L = n_s + H * wl.spec.n_u
    x0 = torch.tensor(wl.x0[:1, :n_s], dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    mean, std = torch.zeros((1, H, 1), dtype=torch.float64, device=DEV), torch.full((1, H, 1), float(wl.init_std),
                                                                                   dtype=torch.float64, device=DEV)
    noise = rnd(1, P, H, 1)
    row(row='launch_plain', E=1, us=time_launches(
        lambda: cem_mpc.cem_rollout(ssm, env, x0, H, mean=mean, std=std, noise=noise, status=status)))
    r_mean = torch.cat([x0, mean.view(1, -1)], dim=1)
    r_std = torch.cat([torch.full((1, n_s), 0.05, dtype=torch.float64, device=DEV), std.view(1, -1)], dim=1)
    r_noise = rnd(1, P, L)
    row(row='launch_starts', E=1, us=time_launches(
        lambda: cem_mpc.cem_rollout_starts(ssm, env, H, mean=r_mean, std=r_std, noise=r_noise, status=status)))
    m = alternate(lambda: cem_mpc.cem_rollout_starts(ssm, env, H, mean=r_mean, std=r_std, noise=r_noise, status=status),
                  lambda: cem_mpc.cem_rollout_starts(ssm, env, H, mean=r_mean, std=r_std, noise=r_noise, status=status,
                                                     con_set=con_set), time_launches)
    row(row='launch_starts_cons', E=1, us=m['ours'], min_us=m['lo'], max_us=m['hi'], parent_us=m['parent'], ratio=m['ratio'],
        parent_spread=m['parent_spread'], repeats=args.repeats)


if __name__ == '__main__':
    main()
