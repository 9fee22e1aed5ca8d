"""Solve time against the number of junk states (the reference's "exact gp rbf" curve, notebooks/results.ipynb cell 15),
on this build: config 2 (pendulum, N = 200, 4096 particles, H = 15, 8 CEM iterations, 409 elites), JunkDimensionsSSM
over the exact RBF GP with J_s = 0 .. 5 junk states and J_a junk actions (default 0).

    python tools/junk_sweep.py [--js 0,1,2,3,4,5] [--ja 0] [--solves 200] [--warmup 20] [--no-stepwise]

For every J_s: one synchronous solve (FusedCemMpc.solve + device synchronise) timed on the host clock, `--solves` times
after `--warmup` untimed ones, on the fused path (kernel_family 'rbf_junk': one sx_cem_rollout_junk launch per iteration)
and on the forced step-by-step path (solve(..., stepwise=True): H x (sx_gp_predict + sx_onestep_reach + costs) per
iteration).  A first row times the plain GpCemSSM of the same problem (no wrapper).  One JSON line per row: median and
p95 in ms.  SX_ROLLOUT=stream makes the J_s = 0 / plain rows use the streaming kernel (the form J_s > 0 always uses).
Needs the GPU.
"""
import argparse
import functools
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
from safe_exploration_amd.ssm_cem.ssm_cem import JunkDimensionsSSM  # noqa: E402

DEV = 'cuda:0'


class Conf:
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'rbf'
    device = DEV


def junk_model(spec, js, ja):
    """The wrapper with the spec's data; the junk columns and outputs get fixed hyper-parameters (length-scale 1,
    outputscale 0.01, noise 1e-5) -- they do not change the real outputs."""
    ssm = JunkDimensionsSSM(functools.partial(GpCemSSM, Conf()), state_dimen=spec.n_s, action_dimen=spec.n_u,
                            junk_states=js, junk_actions=ja)
    d_pad = spec.n_s + js + spec.n_u + ja
    ls = np.ones((spec.n_s + js, d_pad))
    ls[:spec.n_s, :spec.n_s + spec.n_u] = spec.lengthscale
    s_out = np.concatenate((spec.outputscale, np.full(js, 0.01)))
    nz = np.concatenate((spec.noise, np.full(js, 1e-5)))
    if ssm.folded_columns is None:
        ssm._ssm.set_hyperparameters(ls, s_out, nz)
    else:
        ssm._ssm.set_hyperparameters(ls[:spec.n_s][:, list(ssm.folded_columns)], s_out[:spec.n_s], nz[:spec.n_s])
    ssm.update_model(torch.tensor(spec.X, device=DEV), torch.tensor(spec.Y, device=DEV), replace_old=True)
    return ssm


def time_solves(mpc, x0, stepwise, warmup, solves):
    for _ in range(warmup):
        mpc.solve(x0, stepwise=stepwise)
    torch.cuda.synchronize()
    ms = []
    for _ in range(solves):
        t0 = time.perf_counter()
        mpc.solve(x0, stepwise=stepwise)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.percentile(ms, 95))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--js', default='0,1,2,3,4,5')
    ap.add_argument('--ja', type=int, default=0)
    ap.add_argument('--solves', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--no-stepwise', action='store_true', help='time the fused path only')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('junk_sweep.py needs the GPU')
    wl = problems.baseline_workload(2)
    spec = wl.spec
    x0 = torch.tensor(wl.x0[:1, :spec.n_s], dtype=torch.float64, device=DEV)
    form = os.environ.get('SX_ROLLOUT', 'default')

    def row(**kw):
        print(json.dumps(dict(workload='cfg2', H=wl.horizon, P=wl.particles, iters=wl.iterations, rollout_env=form,
                              solves=args.solves, **kw)), flush=True)

    ssm, env = problems.build(spec, device=DEV)
    mpc = FusedCemMpc(ssm, env, wl.horizon, wl.particles, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)
    med, p95 = time_solves(mpc, x0, False, args.warmup, args.solves)
    row(model='GpCemSSM', js=0, ja=0, kernel_family=ssm.kernel_family, path='fused', median_ms=med, p95_ms=p95)
    for js in (int(j) for j in args.js.split(',')):
        ssm = junk_model(spec, js, args.ja)
        mpc = FusedCemMpc(ssm, env, wl.horizon, wl.particles, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)
        common = dict(model='JunkDimensionsSSM', js=js, ja=args.ja, kernel_family=ssm.kernel_family,
                      query_shift=ssm.query_shift)
        if ssm.kernel_family == 'rbf_junk':
            med, p95 = time_solves(mpc, x0, False, args.warmup, args.solves)
            row(path='fused', median_ms=med, p95_ms=p95, stepwise_fallbacks=mpc.stepwise_fallbacks, **common)
        if not args.no_stepwise:
            med, p95 = time_solves(mpc, x0, True, max(1, args.warmup // 4), args.solves)
            row(path='stepwise', median_ms=med, p95_ms=p95, **common)


if __name__ == '__main__':
    main()
