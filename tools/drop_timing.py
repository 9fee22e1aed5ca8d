"""Time GpCemSSM.update_model of a windowed model (conf.cem_gp_window: sx_gp_drop + sx_gp_append) against the full sx_gp_fit
of the last m rows.

    python tools/drop_timing.py [--out profiles/gp_drop_timing.jsonl] [--runs 25]
    python tools/drop_timing.py --one N_S N_U M K          (one configuration of any size, one JSON line)

For (n_s, n_u) in (2,1), (4,1), m in 200, 590, 2000 and r = k in 1, 50: a model with window m is fitted on m rows (untimed), then
the update that adds k rows and so drops the r = k oldest is timed, host wall time around the call and a device synchronisation;
the median of --runs repetitions after 3 warm-up ones.  `full_ms` is the same update of a model without the settings, given
the last m rows with replace_old: the code path the parent commit runs at the bound.  `drop_ms` is sx_gp_drop alone (its
seven launches, synchronised).  Every configuration runs in a child process of its own under a time limit, one at a time;
the first that fails ends the run.  One JSON line each."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [(n_s, n_u, m, k) for n_s, n_u in ((2, 1), (4, 1)) for m in (200, 590, 2000) for k in (1, 50)]
CHILD_LIMIT_S = 150


def one(n_s, n_u, m, k, runs):
    import numpy as np
    import torch

    from safe_exploration_amd.ssm_cem import gp_ssm_cem
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM

    # the model slides up to MAX_SLIDE_ROWS rows, a cap set from this table: lifted here, so that the rows beyond it are timed
    gp_ssm_cem.MAX_SLIDE_ROWS = gp_ssm_cem.MAX_DROP_ROWS

    class Conf:
        device, exact_gp_kernel, exact_gp_training_iterations = 'cuda:0', 'rbf', 0

        def __init__(self, window):
            if window is not None:
                self.cem_gp_incremental, self.cem_gp_window = True, window

    rng = np.random.default_rng([n_s, n_u, m, k])
    D = n_s + n_u
    X = rng.uniform(-1.0, 1.0, size=(m + k, D))
    Y = np.stack([np.sin(X @ rng.normal(size=D)) for _ in range(n_s)], 1) + 0.01 * rng.normal(size=(m + k, n_s))
    X, Y = torch.tensor(X, device='cuda:0'), torch.tensor(Y, device='cuda:0')
    out = dict(n_s=n_s, n_u=n_u, m=m, r=k, k=k, runs=runs)
    for name, window in (('slide_ms', m), ('full_ms', None)):
        ssm = GpCemSSM(Conf(window), n_s, n_u)
        ssm.set_hyperparameters(0.8, 1.0, 0.01)
        times = []
        for rep in range(runs + 3):
            ssm.update_model(X[:m], Y[:m], replace_old=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if window is None:
                ssm.update_model(X[k:], Y[k:], replace_old=True)
            else:
                ssm.update_model(X[m:], Y[m:])
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            assert ssm._appended == (k if window else 0) and ssm.x_train.size(0) == m
        out[name] = statistics.median(times[3:])
    windowed = GpCemSSM(Conf(m), n_s, n_u)
    windowed.set_hyperparameters(0.8, 1.0, 0.01)
    windowed.update_model(X[:m], Y[:m], replace_old=True)
    y_kept = Y[k:m].contiguous()
    times = []
    for rep in range(runs + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        windowed._drop(y_kept, k)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    out['drop_ms'] = statistics.median(times[3:])
    out['speedup'] = out['full_ms'] / out['slide_ms']
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gp_drop_timing.jsonl'))
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--one', type=int, nargs=4, metavar=('N_S', 'N_U', 'M', 'K'), help='(internal) one configuration')
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs: at least 20')
    if args.one:
        one(*args.one, args.runs)
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
        line = [l for l in done.stdout.splitlines() if l.startswith('{')][-1]
        print(line, flush=True)
        lines.append(line)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
