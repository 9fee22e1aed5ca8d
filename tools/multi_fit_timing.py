"""Wall time of hyper-parameter training for E pendulum GPs (one MI355X): gp_ssm_cem.update_models_multi (lockstep, one
fit + MLL-gradient launch sequence per Adam step for all E) against update_model one model after another.

    python tools/multi_fit_timing.py [--iters 1000] [--out profiles/multi_fit_timing.jsonl]

One JSON line per (E, N): the medians of --reps timed runs (after one warm-up run) of each way, the ratio, and the
settings (iters, reps).  profiles/multi_fit_timing.jsonl: `--iters 1000 --reps 3`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM, update_models_multi  # noqa: E402

DEV = 'cuda:0'


def models(E, iters):
    class Conf:
        exact_gp_kernel, device, exact_gp_training_iterations = 'rbf', DEV, iters
    return [GpCemSSM(Conf(), 2, 1) for _ in range(E)]


def data(E, n):
    rng = np.random.default_rng(n)
    xs, ys = [], []
    for _ in range(E):
        X = rng.uniform(-1, 1, size=(n, 3))
        Y = np.stack([np.sin(X @ rng.normal(size=3)), np.cos(X @ rng.normal(size=3))], 1) + 0.01 * rng.normal(size=(n, 2))
        xs.append(torch.tensor(X, device=DEV))
        ys.append(torch.tensor(Y, device=DEV))
    return xs, ys


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ns', default='60,200,410')
    ap.add_argument('--es', default='1,6')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for E in [int(v) for v in a.es.split(',')]:
        for n in [int(v) for v in a.ns.split(',')]:
            xs, ys = data(E, n)

            def one_by_one():
                for m, x, y in zip(models(E, a.iters), xs, ys):
                    m.update_model(x, y, opt_hyp=True)

            def lockstep():
                update_models_multi(models(E, a.iters), xs, ys, opt_hyp=True)

            res = {}
            for name, fn in (('sequential_s', one_by_one), ('batched_s', lockstep)):
                fn()   # warm-up (allocations, code-object load)
                res[name] = float(np.median([timed(fn) for _ in range(a.reps)]))
            line = dict(E=E, N=n, iters=a.iters, reps=a.reps, warmup=1, **res,
                        speedup=res['sequential_s'] / res['batched_s'], batched_ms_per_step=1e3 * res['batched_s'] / a.iters)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
