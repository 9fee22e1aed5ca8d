"""What the SafeMPC constraint set in the rollout costs, in one process: config 2's pendulum (N = 200) and a cart-pole model
(problems.cartpole(200)), 4096 rows, H = 15 and 20.

    python tools/conset_timing.py [--workloads cfg2,cartpole] [--horizons 15,20] [--repeats 7] [--launches 200] [--solves 60]
                                  [--warmup 20] [--out profiles/conset_timing.jsonl] [--label TEXT]
    SX_ROLLOUT=stream python tools/conset_timing.py --no-solves ...       # the parent forced to the streaming form
    python tools/conset_timing.py --models 6 --horizons 15 --repeats 5 --launches 100 ...      # the multi-model form

The _cons entries have the streaming kernel only, so a parent that takes a resident form by default is measured twice: in a
process of its own under SX_ROLLOUT=stream (what the section alone costs) and in its default form (what a solve with a set
pays in all).  Every row carries `override` (SX_ROLLOUT of the process) and `parent_form` (sx_cem_rollout_form in that
process: 0 streaming, 1 four-wave, 2 eight-wave, 3 output by output).

Rows (one JSON line each; printed and, with `--out`, appended to that jsonl file):
  launch_<entry>             the parent entry (sx_cem_rollout, sx_cem_rollout_elites) in SX_OBJ_AFFINE_ABS mode: `--launches`
                             launches back to back between two synchronisations, per launch in us; the median, the smallest
                             and the largest of `--repeats` such measurements
  launch_<entry>_cons        the _cons entry with the full set (the feedback bounds and two obstacle rows) and cost = NULL on
                             the same buffers, measured in alternation with its parent; `ratio` = median / the parent's median,
                             `parent_spread` = (largest - smallest) / median of the parent: what a ratio is read against
  launch_<entry>_sat         sx_cem_rollout[_elites]_sat with the model's saturating cost, in the same alternation
  launch_<entry>_cons_sat    the _cons entry with the full set and that cost; `ratio` against the parent, `ratio_sat` against
                             the _sat entry (the expectation: the _sat entry's own ratio over its parent)
  solve_plain, solve_cons    a solve (config 2's elites and iterations) of FusedCemMpc without and with con_set: median and p95
                             in ms of `--solves` synchronous solves after `--warmup` untimed ones, in alternation; `ratio` =
                             with / without.  Run on the parent commit, solve_plain is the same solve there.
With `--models E` (an integer) the rows are those of the multi-model form instead: E models of the workload with a training
set each (seeds 0 .. E-1 beside the workload's own), one launch for all of them, P rows per problem.
  launch_<entry>_multi            sx_cem_rollout[_elites]_multi, as launch_<entry> above
  launch_<entry>_cons_multi       sx_cem_rollout[_elites]_cons_multi with the full set and cost = NULL; `ratio`, `parent_spread`
  launch_<entry>_sat_multi        the _sat_multi entry with the model's saturating cost
  launch_<entry>_cons_sat_multi   the _cons_multi entry with the full set and that cost; `ratio`, `ratio_sat`
  solve_multi_plain               MultiModelCemMpc.get_actions_multi over the E models (the same solve on the parent commit)
  solve_multi_cons                MultiModelConsCemMpc.get_actions_multi with the full set; `ratio` over solve_multi_plain
  solve_each_cons                 the same E problems as E FusedCemMpc(con_set=...).get_actions_batch calls in turn: what a user
                                  did before the multi-model form; `ratio` over solve_multi_cons
Every solve row carries `through`: 'get_actions_multi' (the checked hand-off included; solve_each_cons: get_actions_batch), or
'solve' where the workload's solves end with a numerical status word that the hand-off raises for.
(`--models` with a list of names is `--workloads`, as before.)
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


def multi_rows(args, E, workloads, horizons, wl, row, full_set, has_multi_cons, randn, full):
    """The rows of `--models E`: the launches of the multi-model entries, then the solves."""
    from safe_exploration_amd.cem_mpc import GpModelTable, MultiModelCemMpc
    lib, P = _lib.lib(), wl.particles
    for name, (ssm0, env, spec0, std0, x0_one, cost) in workloads.items():
        N, n_s, n_u = int(ssm0.device_model.n_train), spec0.n_s, spec0.n_u
        # E training sets of the workload's size: the workload's own model, and its problem at other seeds
        others = [problems.pendulum(n_train=N, seed=e) if name.startswith('cfg2') else problems.cartpole(n_train=N, seed=2 + e)
                  for e in range(1, E)]
        ssms = [ssm0] + [problems.build(s, device=DEV)[0] for s in others]
        x0 = x0_one.expand(E, n_s).contiguous()
        models = cem_mpc.model_array(ssms, 'rbf')
        table = GpModelTable('rbf')

        def rollout(H, elites, **kw):
            mean, std, noise = full(0.0, E, H, n_u), full(std0, E, H, n_u), randn(E, P, H, n_u)
            rows = torch.cat([full(0.0, E, wl.elites, 2), std0 * randn(E, wl.elites, H * n_u)], dim=2).contiguous()
            status = torch.zeros(E, dtype=torch.int32, device=DEV)
            dist = dict(elite_rows=rows) if elites else dict(mean=mean, std=std)
            return lambda: cem_mpc.cem_rollout_multi(ssms, env, x0, H, noise=noise, status=status, table=table, **dist, **kw)

        for H in horizons:
            form = int(lib.sx_cem_rollout_multi_form(models, E, H))
            for elites in (False, True):
                entry = 'sx_cem_rollout' + ('_elites' if elites else '')
                fns = {'parent': rollout(H, elites), 'sat': rollout(H, elites, cost=cost)}
                if has_multi_cons:
                    cons = full_set(spec0)
                    fns['cons'] = rollout(H, elites, con_set=cons)
                    fns['cons_sat'] = rollout(H, elites, con_set=cons, cost=cost)
                us = {k: [] for k in fns}
                for _ in range(args.repeats):               # in alternation: a drift of the clocks meets all alike
                    for k, fn in fns.items():
                        us[k].append(time_launches(fn, args.launches, args.warmup))
                med = {k: float(np.median(v)) for k, v in us.items()}
                spread = (max(us['parent']) - min(us['parent'])) / med['parent']
                shape = dict(workload=name, models=E, N=N, H=H, form=form, repeats=args.repeats, launches=args.launches)
                for k in fns:
                    extra = {} if k == 'parent' else dict(ratio=med[k] / med['parent'], parent_spread=spread)
                    if k == 'cons_sat':
                        extra['ratio_sat'] = med[k] / med['sat']
                    row(row=f'launch_{entry}' + ('' if k == 'parent' else '_' + k) + '_multi', us=med[k], us_min=min(us[k]),
                        us_max=max(us[k]), **shape, **extra)
        if args.no_solves:
            continue
        states = torch.cat([x0, torch.zeros((E, n_s * n_s), dtype=torch.float64, device=DEV)], dim=1)
        for H in horizons:
            make = lambda e, **kw: FusedCemMpc(ssms[e], env, H, P, wl.elites, wl.iterations, device=DEV, init_std=std0, seed=e,
                                               **kw)
            plain = MultiModelCemMpc.from_solvers([make(e) for e in range(E)])
            # through get_actions_multi / get_actions_batch (the checked hand-off included) where the workload's solves end
            # with a clean status; where the hand-off raises for a numerical status (the cart-pole model: DESIGN.md section 2b,
            # configs 3 and 4), through solve(), which synchronises nothing and checks nothing
            try:
                plain.get_actions_multi(states)
                through = 'get_actions_multi'
            except ValueError:
                through = 'solve'
            checked = through == 'get_actions_multi'
            runs = {'multi_plain': (lambda: plain.get_actions_multi(states)) if checked else (lambda: plain.solve(x0))}
            if has_multi_cons:
                cons = full_set(spec0)
                each = [make(e, con_set=cons) for e in range(E)]
                together = cem_mpc.MultiModelConsCemMpc.from_solvers([make(e, con_set=cons) for e in range(E)])
                runs['multi_cons'] = (lambda: together.get_actions_multi(states)) if checked else (lambda: together.solve(x0))
                runs['each_cons'] = ((lambda: [s.get_actions_batch(states[e:e + 1]) for e, s in enumerate(each)]) if checked
                                     else (lambda: [s.solve(x0[e:e + 1]) for e, s in enumerate(each)]))
            for _ in range(args.warmup):
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in runs}
            for _ in range(args.solves):
                for k, fn in runs.items():
                    ms[k].append(time_solve(fn))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            spread = (max(ms['multi_plain']) - min(ms['multi_plain'])) / med['multi_plain']
            for k in runs:
                extra = dict(ratio=med[k] / med['multi_plain' if k == 'multi_cons' else 'multi_cons']) if k != 'multi_plain' else {}
                row(row=f'solve_{k}', workload=name, models=E, N=N, H=H, iters=wl.iterations, elites=wl.elites,
                    form=int(lib.sx_cem_rollout_multi_form(models, E, H)), median_ms=med[k], min_ms=min(ms[k]),
                    p95_ms=float(np.percentile(ms[k], 95)), plain_spread=spread, solves=args.solves, through=through, **extra)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--workloads', default='cfg2,cartpole')
    ap.add_argument('--models', default=None, help='an integer E: the rows of the multi-model form over E models per launch '
                                                   '(a list of names: --workloads)')
    ap.add_argument('--horizons', default='15,20')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--solves', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--no-solves', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--label', default=None, help='a `label` field for every row (which commit, say)')
    args = ap.parse_args()
    n_models = int(args.models) if args.models and args.models.isdigit() else 0
    if args.models and not n_models:
        args.workloads = args.models
    if not torch.cuda.is_available():
        raise SystemExit('conset_timing.py needs the GPU')
    out = open(args.out, 'a') if args.out else None
    override = os.environ.get('SX_ROLLOUT') or 'none'
    wl = problems.baseline_workload(2)
    P = wl.particles
    lib = _lib.lib()
    has_cons = hasattr(cem_mpc, 'conset_eval')      # (false on the parent commit: the parent rows and solve_plain only)
    has_multi_cons = hasattr(cem_mpc, 'MultiModelConsCemMpc')
    if has_cons:
        from safe_exploration_amd.gp_reachability_pytorch import make_con_set

    def row(**kw):
        line = json.dumps({**dict(P=P, override=override), **({'label': args.label} if args.label else {}), **kw})
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

    def full_set(spec):
        # the feedback bounds, and the first two rows of the safe polytope pulled in as the obstacle
        return make_con_set(spec.n_s, h_mat_obs=spec.h_mat[:2], h_obs=0.9 * spec.h_vec[:2, 0], ctrl_ellipsoid=True)

    workloads = {}
    if 'cfg2' in args.workloads.split(','):
        ssm, env = problems.build(wl.spec, device=DEV)
        workloads['cfg2 model'] = (ssm, affine(env), wl.spec, wl.init_std,
                                   torch.tensor(wl.x0[:1, :wl.spec.n_s], dtype=torch.float64, device=DEV),
                                   SaturatingCost([0.0, 0.0, 1.0], np.diag([0.1, 1.0, 1.0]), trig_idx=1))
    if 'cartpole' in args.workloads.split(','):
        spec = problems.cartpole(n_train=200)
        ssm, env = problems.build(spec, device=DEV)
        workloads['cartpole'] = (ssm, affine(env), spec, 0.01, torch.zeros((1, 4), dtype=torch.float64, device=DEV),
                                 SaturatingCost([2.5, 0.0, 0.0, 0.0, 0.5], np.diag([20.0, 0.0, 0.0, 0.0, 5.0]) / 100.0,
                                                trig_idx=2))
    horizons = [int(h) for h in args.horizons.split(',')]
    if n_models:
        return multi_rows(args, n_models, workloads, horizons, wl, row, full_set if has_cons else None, has_multi_cons, randn,
                          full)

    # ---- (a) per launch: the _cons entry against its parent and against _sat ----
    def rollout(ssm, env, x0, H, std0, elites, **kw):
        n_u = ssm.num_actions
        mean, std, noise = full(0.0, 1, H, n_u), full(std0, 1, H, n_u), randn(1, P, H, n_u)
        rows = torch.cat([full(0.0, 1, wl.elites, 2), std0 * randn(1, wl.elites, H * n_u)], dim=2).contiguous()
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        dist = dict(elite_rows=rows) if elites else dict(mean=mean, std=std)
        return lambda: cem_mpc.cem_rollout(ssm, env, x0, H, noise=noise, status=status, **dist, **kw)

    for name, (ssm, env, spec, std0, x0, cost) in workloads.items():
        N = int(ssm.device_model.n_train)
        for H in horizons:
            form = int(lib.sx_cem_rollout_form(ctypes.byref(ssm.device_model), H))
            for elites in (False, True):
                entry = 'sx_cem_rollout' + ('_elites' if elites else '')
                fns = {'parent': rollout(ssm, env, x0, H, std0, elites), 'sat': rollout(ssm, env, x0, H, std0, elites, cost=cost)}
                if has_cons:
                    cons = full_set(spec)
                    fns['cons'] = rollout(ssm, env, x0, H, std0, elites, con_set=cons)
                    fns['cons_sat'] = rollout(ssm, env, x0, H, std0, elites, con_set=cons, cost=cost)
                us = {k: [] for k in fns}
                for _ in range(args.repeats):               # in alternation: a drift of the clocks meets all alike
                    for k, fn in fns.items():
                        us[k].append(time_launches(fn, args.launches, args.warmup))
                med = {k: float(np.median(v)) for k, v in us.items()}
                spread = (max(us['parent']) - min(us['parent'])) / med['parent']
                shape = dict(workload=name, N=N, H=H, parent_form=form, repeats=args.repeats, launches=args.launches)
                for k in fns:
                    extra = {} if k == 'parent' else dict(ratio=med[k] / med['parent'], parent_spread=spread)
                    if k == 'cons_sat':
                        extra['ratio_sat'] = med[k] / med['sat']
                    row(row=f'launch_{entry}' + ('' if k == 'parent' else '_' + k), us=med[k], us_min=min(us[k]),
                        us_max=max(us[k]), **shape, **extra)

    # ---- (b) a whole solve without and with the set ----
    if args.no_solves:
        return
    for name, (ssm, env, spec, std0, x0, cost) in workloads.items():
        for H in horizons:
            make = lambda **kw: FusedCemMpc(ssm, env, H, P, wl.elites, wl.iterations, device=DEV, init_std=std0, **kw)
            solvers = {'plain': make()}
            if has_cons:
                solvers['cons'] = make(con_set=full_set(spec))
            for _ in range(args.warmup):
                for s in solvers.values():
                    s.solve(x0)
            torch.cuda.synchronize()
            ms = {k: [] for k in solvers}
            for _ in range(args.solves):
                for k, s in solvers.items():
                    ms[k].append(time_solve(lambda: s.solve(x0)))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            form = int(lib.sx_cem_rollout_form(ctypes.byref(ssm.device_model), H))
            for k in solvers:
                row(row=f'solve_{k}', workload=name, N=int(ssm.device_model.n_train), H=H, iters=wl.iterations, elites=wl.elites,
                    parent_form=form, median_ms=med[k], p95_ms=float(np.percentile(ms[k], 95)), solves=args.solves,
                    **(dict(ratio=med['cons'] / med['plain']) if k == 'cons' else {}))


if __name__ == '__main__':
    main()
