"""Wall time of the max-variance subset selection and of a solve on a bounded model (one MI355X).

    python tools/subset_timing.py [--out profiles/subset_select_timing.jsonl]

One JSON line per measurement (medians of --reps timed runs after one warm-up run):

  select   (2, 1) pool of n points, m kept: `kernel_s` GpCemSSM.select_subset (sx_gp_select: one launch per step),
           `torch_s` the same pivoted factorisation driven step by step from torch on the device (per step: a gather, a
           kernel column, a matrix-vector product, an argmax and its host read), `host_s` the same in numpy on the
           host (once; skipped above --host-max n x m^2); `same_idx`: do all three choose the same rows?
  solve    a config-2 solve (H, particles, elites, iterations of BASELINE config 2) on a pool of --pool points: fitted
           whole (`n_train` = the pool) and with cem_gp_subset_size = --subset; `update_s` is the update_model that
           precedes it (selection, fit and pack), `solve_ms` the median synchronous solve.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import problems  # noqa: E402
from safe_exploration_amd.cem_mpc import FusedCemMpc  # noqa: E402
from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM  # noqa: E402

DEV = 'cuda:0'


def conf(**kw):
    base = dict(exact_gp_kernel='rbf', device=DEV, exact_gp_training_iterations=0)
    base.update(kw)
    return type('Conf', (), base)()


def pool(n, seed=0):
    """X uniform in [-1, 1]^3, per-output hyper-parameters, noise = 1e-2 outputscale"""
    rng = np.random.default_rng([n, seed])
    X = rng.uniform(-1.0, 1.0, size=(n, 3))
    ls = rng.uniform(0.4, 1.5, size=(2, 3))
    s = rng.uniform(0.5, 2.0, size=2)
    return X, ls, s, 1e-2 * s


def timed(fn, sync=True):
    if sync:
        torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return time.perf_counter() - t, out


def select_torch(X, ls, s, noise, m):
    """the pivoted factorisation with torch operations on the device, one greedy step at a time"""
    n = X.size(0)
    r = (s + noise)[:, None].expand(-1, n).clone()
    C = torch.zeros((s.numel(), m, n), dtype=torch.float64, device=X.device)
    mask = torch.zeros(n, dtype=torch.bool, device=X.device)
    chosen = []
    for j in range(m):
        p = int(torch.argmax(torch.where(mask, -np.inf, r.sum(0))))
        chosen.append(p)
        mask[p] = True
        q = (((X - X[p]) / ls[:, None, :]) ** 2).sum(-1)                     # [n_s x n]
        k = s[:, None] * torch.exp(-0.5 * q)
        k[:, p] += noise
        c = (k - torch.einsum('dl,dln->dn', C[:, :j, p], C[:, :j])) / torch.sqrt(r[:, p])[:, None]
        C[:, j] = c
        r -= c * c
    return chosen


def select_host(X, ls, s, noise, m):
    n = X.shape[0]
    r = np.repeat((s + noise)[:, None], n, 1)
    C = np.zeros((len(s), m, n))
    mask = np.zeros(n, bool)
    chosen = []
    for j in range(m):
        p = int(np.argmax(np.where(mask, -np.inf, r.sum(0))))
        chosen.append(p)
        mask[p] = True
        for d in range(len(s)):
            k = s[d] * np.exp(-0.5 * (((X - X[p]) / ls[d]) ** 2).sum(1))
            k[p] += noise[d]
            c = (k - C[d, :j, p] @ C[d, :j]) / np.sqrt(r[d, p])
            C[d, j] = c
            r[d] -= c * c
    return chosen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ns', default='1000,4000,16000')
    ap.add_argument('--ms', default='200,1000')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-max', type=float, default=2e10, help='largest n x m^2 the host form is timed at')
    ap.add_argument('--pool', type=int, default=800)
    ap.add_argument('--subset', type=int, default=200)
    ap.add_argument('--solves', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('subset_timing.py needs the GPU')
    lines = []

    def row(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    for n in [int(v) for v in a.ns.split(',')]:
        X, ls, s, noise = pool(n)
        ssm = GpCemSSM(conf(), 2, 1)
        ssm.set_hyperparameters(ls, s, noise)
        dev = [torch.tensor(v, device=DEV) for v in (X, ls, s, noise)]
        for m in [int(v) for v in a.ms.split(',')]:
            if m > n:
                continue
            kernel = lambda: ssm.select_subset(dev[0], m)[0].cpu().tolist()
            in_torch = lambda: select_torch(*dev, m)
            res, idx = {}, {}
            for name, fn in (('kernel_s', kernel), ('torch_s', in_torch)):
                fn()   # warm-up (allocations, code-object load)
                runs = [timed(fn) for _ in range(a.reps)]
                res[name], idx[name] = float(np.median([t for t, _ in runs])), runs[-1][1]
            same = idx['kernel_s'] == idx['torch_s']
            if n * m * m <= a.host_max:
                res['host_s'], host_idx = timed(lambda: select_host(X, ls, s, noise, m), sync=False)
                same = same and host_idx == idx['kernel_s']
            row(what='select', n_s=2, n_u=1, n=n, m=m, reps=a.reps, warmup=1, **res, same_idx=same,
                kernel_us_per_step=1e6 * res['kernel_s'] / m, torch_over_kernel=res['torch_s'] / res['kernel_s'])

    wl = problems.baseline_workload(2, n_train=a.pool)
    spec = wl.spec
    _, env = problems.build(problems.pendulum(n_train=8), device=DEV)
    x0 = torch.tensor(wl.x0, device=DEV)
    xt, yt = torch.tensor(spec.X, device=DEV), torch.tensor(spec.Y, device=DEV)
    for subset in (None, a.subset):
        ssm = GpCemSSM(conf(cem_gp_subset_size=subset), spec.n_s, spec.n_u)
        ssm.set_hyperparameters(spec.lengthscale, spec.outputscale, spec.noise)
        update = lambda: ssm.update_model(xt, yt, replace_old=True)
        update()
        update_s = float(np.median([timed(update)[0] for _ in range(a.reps)]))
        mpc = FusedCemMpc(ssm, env, wl.horizon, wl.particles, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)
        for _ in range(3):
            mpc.solve(x0)
        times = [timed(lambda: mpc.solve(x0))[0] for _ in range(a.solves)]
        row(what='solve', cfg=2, pool=a.pool, cem_gp_subset_size=subset, n_train=int(ssm.device_model.n_train),
            update_s=update_s, solve_ms=1e3 * float(np.median(times)), solve_ms_p95=1e3 * float(np.percentile(times, 95)),
            solves=a.solves, warmup=3)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
