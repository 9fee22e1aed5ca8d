"""Time update_models_multi of E windowed models with full windows with conf.cem_gp_incremental_lockstep (one sx_gp_drop_multi
and one sx_gp_append_multi for all) against without it (model by model, sx_gp_drop + sx_gp_append: the path the parent
commit runs, so the baseline).

    python tools/drop_multi_timing.py [--out profiles/gp_drop_multi_timing.jsonl] [--runs 25]

For (n_s, n_u) in (2,1), (4,1), windows of m in 200, 590, 2000 rows, r = k in 1, 16 and E in 2, 6: E models
(conf.cem_gp_window = m) are fitted on m rows each (untimed), then the update that gives k rows to every one of them, so that
each slides by r = k rows, is timed, host wall time around update_models_multi and a device synchronisation, with the
setting on and off; the median of --runs repetitions after 3 warm-up ones.  The method is tools/append_multi_timing.py's,
and both arms run in one process on one box.  Every (shape, m, k) runs in a child process of its own under a time limit, one
at a time; the first that fails ends the run.  One JSON line per (shape, m, k, E).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/drop_multi_timing.py --one 2 1 2000 1 --models 6

runs one configuration with one E in the traced process itself: the kernels of the lockstep arm are the <.., true>
instantiations, those of the other arm the <.., false> ones, so the trace's per-kernel statistics separate the arms."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [(n_s, n_u, m, k) for n_s, n_u in ((2, 1), (4, 1)) for m in (200, 590, 2000) for k in (1, 16)]
MODELS = (2, 6)
CHILD_LIMIT_S = 200


def one(n_s, n_u, m, k, runs, models=MODELS):
    import numpy as np
    import torch

    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM, update_models_multi

    class Conf:
        device, exact_gp_kernel, exact_gp_training_iterations, cem_gp_incremental = 'cuda:0', 'rbf', 0, True
        cem_gp_window = m

        def __init__(self, lockstep):
            self.cem_gp_incremental_lockstep = lockstep

    D = n_s + n_u
    data = []
    for e in range(max(models)):
        rng = np.random.default_rng([n_s, n_u, m, k, e])
        X = rng.uniform(-1.0, 1.0, size=(m + k, D))
        Y = np.stack([np.sin(X @ rng.normal(size=D)) for _ in range(n_s)], 1) + 0.01 * rng.normal(size=(m + k, n_s))
        data.append((torch.tensor(X, device='cuda:0'), torch.tensor(Y, device='cuda:0')))
    for E in models:
        out = dict(n_s=n_s, n_u=n_u, m=m, r=k, k=k, E=E, runs=runs)
        for name, lockstep in (('lockstep_ms', True), ('one_by_one_ms', False)):
            ssms = [GpCemSSM(Conf(lockstep), n_s, n_u) for _ in range(E)]
            for ssm in ssms:
                ssm.set_hyperparameters(0.8, 1.0, 0.01)
            times = []
            for rep in range(runs + 3):
                for ssm, (X, Y) in zip(ssms, data):
                    ssm.update_model(X[:m], Y[:m], replace_old=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                update_models_multi(ssms, [X[m:] for X, _ in data[:E]], [Y[m:] for _, Y in data[:E]])
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                assert all(ssm._appended == k and ssm.x_train.size(0) == m for ssm in ssms)   # (every model slid)
            out[name] = statistics.median(times[3:])
        out['speedup'] = out['one_by_one_ms'] / out['lockstep_ms']
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gp_drop_multi_timing.jsonl'))
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--one', type=int, nargs=4, metavar=('N_S', 'N_U', 'M', 'K'), help='one configuration, in this process')
    ap.add_argument('--models', type=int, nargs='+', default=list(MODELS), help='with --one: the E to run (for a kernel trace)')
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs: at least 20')
    if args.one:
        one(*args.one, args.runs, tuple(args.models))
        return 0
    lines = []
    for cfg in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), '--runs', str(args.runs), '--one'] + [str(v) for v in cfg]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f'{cfg}: no result within {CHILD_LIMIT_S} s; stopping', file=sys.stderr)
            return 1
        if done.returncode != 0:
            print(f'{cfg}: exit status {done.returncode}; stopping\n{done.stderr[-2000:]}', file=sys.stderr)
            return 1
        found = [l for l in done.stdout.splitlines() if l.startswith('{')]
        if len(found) != len(MODELS):
            print(f'{cfg}: {len(found)} result lines; stopping', file=sys.stderr)
            return 1
        for line in found:
            print(line, flush=True)
            lines.append(line)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
