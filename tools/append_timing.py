"""Time GpCemSSM.update_model with conf.cem_gp_incremental (sx_gp_append) against without it (the full sx_gp_fit).

    python tools/append_timing.py [--out profiles/gp_append_timing.jsonl] [--runs 25]

For (n_s, n_u) in (2,1), (4,1), N in 200, 590, 2000 and k in 1, 50: a model is fitted on N rows (untimed), then the update
that adds k rows is timed, host wall time around the call and a device synchronisation, with the setting on and off; the
median of --runs repetitions after 3 warm-up ones.  With the setting off the code path is the one the parent commit runs
for every update.  `pack_ms` is sx_gp_pack alone at N + k rows, which both updates end in.  Every configuration runs in a
child process of its own under a time limit, one at a time; the first that fails ends the run.  One JSON line each."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [(n_s, n_u, n, k) for n_s, n_u in ((2, 1), (4, 1)) for n in (200, 590, 2000) for k in (1, 50)]
CHILD_LIMIT_S = 150


def one(n_s, n_u, n, k, runs):
    import ctypes

    import numpy as np
    import torch

    from safe_exploration_amd import _lib
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM

    class Conf:
        device, exact_gp_kernel, exact_gp_training_iterations = 'cuda:0', 'rbf', 0

        def __init__(self, incremental):
            self.cem_gp_incremental = incremental

    rng = np.random.default_rng([n_s, n_u, n, k])
    D = n_s + n_u
    X = rng.uniform(-1.0, 1.0, size=(n + k, D))
    Y = np.stack([np.sin(X @ rng.normal(size=D)) for _ in range(n_s)], 1) + 0.01 * rng.normal(size=(n + k, n_s))
    X, Y = torch.tensor(X, device='cuda:0'), torch.tensor(Y, device='cuda:0')
    out = dict(n_s=n_s, n_u=n_u, N=n, k=k, runs=runs)
    for name, incremental in (('append_ms', True), ('full_ms', False)):
        ssm = GpCemSSM(Conf(incremental), n_s, n_u)
        ssm.set_hyperparameters(0.8, 1.0, 0.01)
        times = []
        for rep in range(runs + 3):
            ssm.update_model(X[:n], Y[:n], replace_old=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ssm.update_model(X[n:], Y[n:])
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            assert ssm._appended == (k if incremental else 0)
        out[name] = statistics.median(times[3:])
    m = _lib.SxGpModel.from_buffer_copy(ssm.device_model)
    times = []
    for rep in range(runs + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ssm._pack(m, ssm._fit_ws[1], ssm._alpha)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    out['pack_ms'] = statistics.median(times[3:])
    out['speedup'] = out['full_ms'] / out['append_ms']
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gp_append_timing.jsonl'))
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--one', type=int, nargs=4, metavar=('N_S', 'N_U', 'N', 'K'), help='(internal) one configuration')
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
    at = {(r['n_s'], r['N'], r['k']): r for r in map(json.loads, lines)}
    slow = [key for key, r in at.items() if key[1] == 2000 and key[2] == 1 and not r['append_ms'] < r['full_ms']]
    if slow:
        print(f'the appended update is not faster than the full one at N = 2000, k = 1: {slow}', file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
