"""What the saturating cost costs as a kernel objective, in one process: config 2's model (pendulum, N = 200, 4096
particles), T = 10 cautious steps and n_perf = 30 performance steps; the launches also over a cart-pole model (n_s = 4,
N = 200, the reference's cost constants: rank 2 of 5), whose instantiations spill.

    python tools/sat_cost_timing.py [--models cfg2,cartpole] [--repeats 7] [--launches 200] [--solves 60] [--warmup 20]
                                    [--out profiles/sat_cost_timing.jsonl]

Rows (one JSON line each; printed and, with `--out`, appended to that jsonl file):
  launch_<entry>          the parent entry in SX_OBJ_AFFINE_ABS mode (sx_cem_cautious_rollout at T = 10,
                          sx_cem_perf_rollout_taylor and sx_cem_perf_rollout_taylor_multi (two GPs) at n_perf = 30, r = 1):
                          `--launches` launches back to back between two synchronisations, per launch in us; the median, the
                          smallest and the largest of `--repeats` such measurements
  launch_<entry>_sat      the _sat entry on the same buffers, measured in alternation with its parent; `ratio` = median / the
                          parent's median, `parent_spread` = (largest - smallest) / median of the parent: the run-to-run
                          spread a ratio is read against.  The cart-pole rows carry `workload: "cartpole"`.
  solve_<solver>_kernel   a solve (config 2's particles, elites and iterations) with the cost set on the solver (set_cost):
                          median and p95 in ms of `--solves` synchronous solves after `--warmup` untimed ones
  solve_<solver>_torch    the same solve with the parent entry recording means and covariances and
                          SaturatingCost.__call__ pricing them in torch every iteration -- the only way to this objective
                          without the kernel form; measured in alternation with the kernel form; `ratio` = kernel median /
                          torch median.  Config 2's model only.
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
from safe_exploration_amd.cem_mpc import CautiousCemMpc, FusedCemMpc  # noqa: E402
from safe_exploration_amd.costs import SaturatingCost  # noqa: E402

DEV = 'cuda:0'
T_CAUTIOUS, N_PERF = 10, 30


def time_launches(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def time_solve(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--models', default='cfg2,cartpole')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--solves', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sat_cost_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None
    wl = problems.baseline_workload(2)
    ssm, env = problems.build(wl.spec, device=DEV)
    env = _lib.SxEnv.from_buffer_copy(env)
    env.obj_mode = _lib.SX_OBJ_AFFINE_ABS
    other, _ = problems.build(problems.pendulum(n_train=200, seed=1), device=DEV)
    P, H = wl.particles, wl.horizon
    # the pendulum's state is (d_theta, theta): the angle is state 1, upright is cos = 1
    cost = SaturatingCost([0.0, 0.0, 1.0], np.diag([0.1, 1.0, 1.0]), trig_idx=1)
    x0 = torch.tensor(wl.x0[:1, :wl.spec.n_s], dtype=torch.float64, device=DEV)

    def row(**kw):
        line = json.dumps({**dict(workload='cfg2 model', N=int(wl.spec.X.shape[0]), P=P), **kw})
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    randn = lambda *shape: torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    full = lambda v, *shape: torch.full(shape, v, dtype=torch.float64, device=DEV)

    # ---- (a) per launch: each _sat entry against its parent ----
    def cautious(ssm, env, x0, std0, **kw):
        mean, std, noise = full(0.0, 1, T_CAUTIOUS, 1), full(std0, 1, T_CAUTIOUS, 1), randn(1, P, T_CAUTIOUS, 1)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        return lambda: cem_mpc.cem_cautious_rollout(ssm, env, x0, T_CAUTIOUS, mean=mean, std=std, noise=noise, status=status,
                                                    **kw)

    def taylor(ssm, other, env, x0, std0, E, **kw):
        tail = N_PERF - 1
        mean, std, noise = full(0.0, E, tail, 1), full(std0, E, tail, 1), randn(E, P, tail, 1)
        safe = (std0 * randn(E, P, H, 1)).contiguous()
        obj, con = full(0.0, E, P), full(0.0, E, P)
        status = torch.zeros(E, dtype=torch.int32, device=DEV)
        xs = x0.expand(E, -1).contiguous()
        common = dict(safe_actions=safe, obj_cost=obj, con_cost=con, status=status, tail_mean=mean, tail_std=std,
                      tail_noise=noise, **kw)
        if E == 1:
            return lambda: cem_mpc.cem_perf_rollout_taylor(ssm, env, xs, H, N_PERF, 1, **common)
        table = cem_mpc.GpModelTable()
        return lambda: cem_mpc.cem_perf_rollout_taylor_multi([ssm, other], env, xs, H, N_PERF, 1, table=table, **common)

    def pairs(ssm, other, env, x0, std0, cost, **tag):
        one, two = (ssm, other, env, x0, std0, 1), (ssm, other, env, x0, std0, 2)
        return (('sx_cem_cautious_rollout', dict(T=T_CAUTIOUS, **tag), cautious(ssm, env, x0, std0),
                 cautious(ssm, env, x0, std0, cost=cost)),
                ('sx_cem_perf_rollout_taylor', dict(n_perf=N_PERF, H=H, r=1, **tag), taylor(*one), taylor(*one, cost=cost)),
                ('sx_cem_perf_rollout_taylor_multi', dict(n_perf=N_PERF, H=H, r=1, E=2, **tag), taylor(*two),
                 taylor(*two, cost=cost)))

    models = args.models.split(',')
    todo = list(pairs(ssm, other, env, x0, wl.init_std, cost)) if 'cfg2' in models else []
    if 'cartpole' in models:
        # the same launches over a cart-pole model with the reference's constants (defaultconfig_episode.py:115-120).  The
        # rows are feed-forward actions on an unstable prior (a step multiplies the pole's angle by about 1.9): actions of
        # 0.01 keep the angle of step 30 where the library's sine takes its ordinary argument reduction
        cp_ssm, cp_env = problems.build(problems.cartpole(n_train=200), device=DEV)
        cp_env = _lib.SxEnv.from_buffer_copy(cp_env)
        cp_env.obj_mode = _lib.SX_OBJ_AFFINE_ABS
        cp_other, _ = problems.build(problems.cartpole(n_train=200, seed=3), device=DEV)
        cp_cost = SaturatingCost([2.5, 0.0, 0.0, 0.0, 0.5], np.diag([20.0, 0.0, 0.0, 0.0, 5.0]) / 100.0, trig_idx=2)
        cp_x0 = torch.zeros((1, 4), dtype=torch.float64, device=DEV)
        todo += list(pairs(cp_ssm, cp_other, cp_env, cp_x0, 0.01, cp_cost, workload='cartpole'))
    for entry, shape, parent, sat in todo:
        us = {'parent': [], 'sat': []}
        for _ in range(args.repeats):               # in alternation: a drift of the clocks meets both alike
            us['parent'].append(time_launches(parent, args.launches, args.warmup))
            us['sat'].append(time_launches(sat, args.launches, args.warmup))
        med = {k: float(np.median(v)) for k, v in us.items()}
        spread = (max(us['parent']) - min(us['parent'])) / med['parent']
        row(row=f'launch_{entry}', us=med['parent'], us_min=min(us['parent']), us_max=max(us['parent']),
            repeats=args.repeats, launches=args.launches, **shape)
        row(row=f'launch_{entry}_sat', us=med['sat'], us_min=min(us['sat']), us_max=max(us['sat']),
            ratio=med['sat'] / med['parent'], parent_spread=spread, repeats=args.repeats, launches=args.launches, **shape)

    # ---- (b) a whole solve: the kernel form against torch on the recorded trajectory ----
    real_cautious, real_taylor = cem_mpc.cem_cautious_rollout, cem_mpc.cem_perf_rollout_taylor

    def torch_cautious(*a, **kw):
        r = real_cautious(*a, **dict(kw, want_traj=True, want_cov=True))
        r['obj_cost'] = cost(r['traj'], r['cov']).sum(dim=-1).contiguous()
        return r

    def torch_taylor(*a, **kw):
        r = real_taylor(*a, **dict(kw, want_traj=True, want_cov=True))
        r['obj_cost'] = cost(r['perf_traj'], r['perf_cov']).sum(dim=-1).contiguous()
        return r

    if 'cfg2' not in models:
        return
    solvers = (('cautious', dict(T=T_CAUTIOUS), 'cem_cautious_rollout', torch_cautious, real_cautious,
                lambda: CautiousCemMpc(ssm, env, T_CAUTIOUS, P, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)),
               ('taylor', dict(n_perf=N_PERF, H=H, r=1), 'cem_perf_rollout_taylor', torch_taylor, real_taylor,
                lambda: FusedCemMpc(ssm, env, H, P, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std,
                                    n_perf=N_PERF, perf_r=1, perf_type='taylor')))
    for name, shape, wrapper, in_torch, real, make in solvers:
        kernel, plain = make(), make()
        kernel.set_cost(cost)

        def solve_torch():
            setattr(cem_mpc, wrapper, in_torch)
            try:
                plain.solve(x0)
            finally:
                setattr(cem_mpc, wrapper, real)

        solve_kernel = lambda: kernel.solve(x0)
        for _ in range(args.warmup):
            solve_kernel()
            solve_torch()
        torch.cuda.synchronize()
        ms = {'kernel': [], 'torch': []}
        for _ in range(args.solves):
            ms['kernel'].append(time_solve(solve_kernel))
            ms['torch'].append(time_solve(solve_torch))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in ('kernel', 'torch'):
            row(row=f'solve_{name}_{k}', iters=wl.iterations, elites=wl.elites, median_ms=med[k],
                p95_ms=float(np.percentile(ms[k], 95)), solves=args.solves,
                **(dict(ratio=med['kernel'] / med['torch']) if k == 'torch' else {}), **shape)


if __name__ == '__main__':
    main()
