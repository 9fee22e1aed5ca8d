"""What the saturating cost on the safety trajectory costs, in one process: config 2's model (pendulum, N = 200, its horizon)
and a cart-pole model (problems.cartpole(200), H = 4, the reference's cost constants: rank 2 of 5), 4096 particles.

    python tools/safety_sat_timing.py [--models cfg2,cartpole] [--repeats 7] [--launches 200] [--solves 60] [--warmup 20]
                                      [--out profiles/safety_sat_timing.jsonl]
    SX_ROLLOUT=stream python tools/safety_sat_timing.py --no-solves ...       # the parents forced to the streaming form

The _sat entries have the streaming kernel only, so a parent that takes a resident form by default is measured twice: in a
process of its own under SX_ROLLOUT=stream (what the section alone costs) and in its default form (what a cost_on_safety
solve pays in all).  Every row carries `override` (SX_ROLLOUT of the process) and `parent_form` (sx_cem_rollout_form /
sx_cem_rollout_multi_form in that process: 0 streaming, 1 four-wave, 2 eight-wave, 3 output by output).

Rows (one JSON line each; printed and, with `--out`, appended to that jsonl file):
  launch_<entry>          the parent entry (sx_cem_rollout, sx_cem_rollout_elites, sx_cem_rollout_multi and
                          sx_cem_rollout_elites_multi over two GPs) in SX_OBJ_AFFINE_ABS mode: `--launches` launches back to
                          back between two synchronisations, per launch in us; the median, the smallest and the largest of
                          `--repeats` such measurements
  launch_<entry>_sat      the _sat entry on the same buffers, measured in alternation with its parent; `ratio` = median / the
                          parent's median, `parent_spread` = (largest - smallest) / median of the parent: the run-to-run
                          spread a ratio is read against
  solve_safety_kernel     a solve (config 2's particles, elites and iterations) of FusedCemMpc(cost_on_safety=True) with the
                          cost set: median and p95 in ms of `--solves` synchronous solves after `--warmup` untimed ones
  solve_safety_torch      the same solve with the parent entry recording `traj` and SaturatingCost.__call__ pricing it in
                          torch every iteration -- the only way to this objective without the kernel form; measured in
                          alternation with the kernel form; `ratio` = kernel median / torch median.  Both models.
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
from safe_exploration_amd.cem_mpc import FusedCemMpc  # noqa: E402
from safe_exploration_amd.costs import SaturatingCost  # noqa: E402

DEV = 'cuda:0'
H_CARTPOLE = 4


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
    ap.add_argument('--no-solves', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('safety_sat_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None
    override = os.environ.get('SX_ROLLOUT') or 'none'
    wl = problems.baseline_workload(2)
    P = wl.particles
    lib = _lib.lib()

    def row(**kw):
        line = json.dumps({**dict(P=P, override=override), **kw})
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    randn = lambda *shape: torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    full = lambda v, *shape: torch.full(shape, v, dtype=torch.float64, device=DEV)

    def affine(env):
        env = _lib.SxEnv.from_buffer_copy(env)
        env.obj_mode = _lib.SX_OBJ_AFFINE_ABS
        return env

    workloads = {}
    if 'cfg2' in args.models.split(','):
        ssm, env = problems.build(wl.spec, device=DEV)
        other, _ = problems.build(problems.pendulum(n_train=200, seed=1), device=DEV)
        # the pendulum's state is (d_theta, theta): the angle is state 1, upright is cos = 1
        workloads['cfg2 model'] = (ssm, other, affine(env), wl.horizon, wl.init_std,
                                   torch.tensor(wl.x0[:1, :wl.spec.n_s], dtype=torch.float64, device=DEV),
                                   SaturatingCost([0.0, 0.0, 1.0], np.diag([0.1, 1.0, 1.0]), trig_idx=1))
    if 'cartpole' in args.models.split(','):
        # the reference's constants (defaultconfig_episode.py:115-120); feed-forward actions of 0.01 on the unstable prior
        ssm, env = problems.build(problems.cartpole(n_train=200), device=DEV)
        other, _ = problems.build(problems.cartpole(n_train=200, seed=3), device=DEV)
        workloads['cartpole'] = (ssm, other, affine(env), H_CARTPOLE, 0.01, torch.zeros((1, 4), dtype=torch.float64, device=DEV),
                                 SaturatingCost([2.5, 0.0, 0.0, 0.0, 0.5], np.diag([20.0, 0.0, 0.0, 0.0, 5.0]) / 100.0,
                                                trig_idx=2))

    # ---- (a) per launch: each _sat entry against its parent ----
    def rollout(models, env, x0, H, std0, elites, **kw):
        E = len(models)
        n_u = models[0].num_actions
        mean, std, noise = full(0.0, E, H, n_u), full(std0, E, H, n_u), randn(E, P, H, n_u)
        rows = torch.cat([full(0.0, E, wl.elites, 2), std0 * randn(E, wl.elites, H * n_u)], dim=2).contiguous()
        status = torch.zeros(E, dtype=torch.int32, device=DEV)
        xs = x0.expand(E, -1).contiguous()
        dist = dict(elite_rows=rows) if elites else dict(mean=mean, std=std)
        if E == 1:
            return lambda: cem_mpc.cem_rollout(models[0], env, xs, H, noise=noise, status=status, **dist, **kw)
        table = cem_mpc.GpModelTable()
        return lambda: cem_mpc.cem_rollout_multi(models, env, xs, H, noise=noise, status=status, table=table, **dist, **kw)

    for name, (ssm, other, env, H, std0, x0, cost) in workloads.items():
        N = int(ssm.device_model.n_train)
        forms = {1: int(lib.sx_cem_rollout_form(ctypes.byref(ssm.device_model), H)),
                 2: int(lib.sx_cem_rollout_multi_form(cem_mpc.model_array([ssm, other], 'rbf'), 2, H))}
        for models in ([ssm], [ssm, other]):
            for elites in (False, True):
                E = len(models)
                entry = 'sx_cem_rollout' + ('_elites' if elites else '') + ('_multi' if E > 1 else '')
                parent, sat = rollout(models, env, x0, H, std0, elites), rollout(models, env, x0, H, std0, elites, cost=cost)
                us = {'parent': [], 'sat': []}
                for _ in range(args.repeats):               # in alternation: a drift of the clocks meets both alike
                    us['parent'].append(time_launches(parent, args.launches, args.warmup))
                    us['sat'].append(time_launches(sat, args.launches, args.warmup))
                med = {k: float(np.median(v)) for k, v in us.items()}
                spread = (max(us['parent']) - min(us['parent'])) / med['parent']
                shape = dict(workload=name, N=N, H=H, E=E, parent_form=forms[E], repeats=args.repeats, launches=args.launches)
                row(row=f'launch_{entry}', us=med['parent'], us_min=min(us['parent']), us_max=max(us['parent']), **shape)
                row(row=f'launch_{entry}_sat', us=med['sat'], us_min=min(us['sat']), us_max=max(us['sat']),
                    ratio=med['sat'] / med['parent'], parent_spread=spread, **shape)

    # ---- (b) a whole solve: the kernel form against torch on the recorded trajectory ----
    if args.no_solves:
        return
    real = cem_mpc.cem_rollout
    for name, (ssm, other, env, H, std0, x0, cost) in workloads.items():
        n_s = ssm.num_states

        def in_torch(*a, **kw):
            r = real(*a, **dict(kw, want_traj=True))
            traj = r['traj']
            r['obj_cost'] = cost(traj[..., :n_s], traj[..., n_s:].reshape(traj.shape[:-1] + (n_s, n_s))).sum(dim=-1).contiguous()
            return r

        make = lambda **kw: FusedCemMpc(ssm, env, H, P, wl.elites, wl.iterations, device=DEV, init_std=std0, **kw)
        kernel, plain = make(cost_on_safety=True), make()
        kernel.set_cost(cost)

        def solve_torch():
            cem_mpc.cem_rollout = in_torch
            try:
                plain.solve(x0)
            finally:
                cem_mpc.cem_rollout = real

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
        form = int(lib.sx_cem_rollout_form(ctypes.byref(ssm.device_model), H))
        for k in ('kernel', 'torch'):
            row(row=f'solve_safety_{k}', workload=name, N=int(ssm.device_model.n_train), H=H, iters=wl.iterations,
                elites=wl.elites, parent_form=form, median_ms=med[k], p95_ms=float(np.percentile(ms[k], 95)),
                solves=args.solves, **(dict(ratio=med['kernel'] / med['torch']) if k == 'torch' else {}))


if __name__ == '__main__':
    main()
