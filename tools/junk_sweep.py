"""Solve time against the number of junk states (the reference's curves per model, notebooks/results.ipynb cell 15), on
this build: config 2 (pendulum, N = 200, 4096 particles, H = 15, 8 CEM iterations, 409 elites), JunkDimensionsSSM over
the inner model `--ssm` with J_s junk states and J_a junk actions (default 0):
  gp          the exact RBF GP, J_s = 0 .. 5 by default (beyond 2 the wrapper folds the padding away)
  linear, nn  the feature-space GP ('nn': layers 8, 16), J_s = 0 .. 2 (the padded model's limit n_s + J_s <= 4)
  mc_dropout  the MC-dropout ensemble of bench.py --ssm mc_dropout (64 x 64, 30 members; 100 training steps), J_s = 0 .. 2

    python tools/junk_sweep.py [--ssm gp] [--js 0,1,2] [--ja 0] [--solves 200] [--warmup 20] [--no-stepwise] [--out F]

For every J_s: one synchronous solve (FusedCemMpc.solve + device synchronise) timed on the host clock, `--solves` times
after `--warmup` untimed ones, on the fused path (kernel_family 'rbf_junk' / 'feature_junk' / 'mlp_junk': one
sx_cem_rollout_{,feat_,mlp_}junk launch per iteration) and on the forced step-by-step path (solve(..., stepwise=True):
H x (predict through the wrapper + sx_onestep_reach + costs) per iteration).  A first row times the plain inner model of
the same problem (no wrapper).  One JSON line per row: median and p95 in ms, printed and, with `--out`, written to that
jsonl file.  SX_ROLLOUT=stream makes the exact GP's J_s = 0 / plain rows use the streaming kernel (the form J_s > 0 always
uses).  Needs the GPU.
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


class FeatConf:
    exact_gp_training_iterations = 0
    nn_kernel_layers = [8, 16]
    device = DEV


class DropConf:     # bench.py --ssm mc_dropout's ensemble, a shorter training
    mc_dropout_training_iterations, mc_dropout_num_samples, mc_dropout_predict_std = 100, 30, False
    mc_dropout_reinitialize, mc_dropout_hidden_features, mc_dropout_type = False, [64, 64], 'fixed'
    mc_dropout_fixed_probability, mc_dropout_on_input, mc_dropout_lengthscale, device = 0.02, False, 1e-4, DEV


def inner_constructor(kind):
    if kind in ('linear', 'nn'):
        return functools.partial(GpCemSSM, type('C', (FeatConf,), {'exact_gp_kernel': kind})())
    from safe_exploration_amd.ssm_cem.dropout_ssm_cem import McDropoutSSM
    return functools.partial(McDropoutSSM, DropConf())


def junk_model(spec, js, ja, kind='gp'):
    """The wrapper with the spec's data.  Exact GP: the junk columns and outputs get fixed hyper-parameters (length-scale
    1, outputscale 0.01, noise 1e-5) -- they do not change the real outputs.  Other models: their defaults."""
    if kind != 'gp':
        ssm = JunkDimensionsSSM(inner_constructor(kind), state_dimen=spec.n_s, action_dimen=spec.n_u, junk_states=js,
                                junk_actions=ja)
        ssm.update_model(torch.tensor(spec.X, device=DEV), torch.tensor(spec.Y, device=DEV), replace_old=True)
        return ssm
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
    ap.add_argument('--ssm', choices=('gp', 'linear', 'nn', 'mc_dropout'), default='gp')
    ap.add_argument('--js', default=None, help='junk-state counts (default 0,1,2,3,4,5 for gp, 0,1,2 otherwise)')
    ap.add_argument('--ja', type=int, default=0)
    ap.add_argument('--solves', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--no-stepwise', action='store_true', help='time the fused path only')
    ap.add_argument('--out', default=None, help='also write the rows to this jsonl file')
    args = ap.parse_args()
    js_list = args.js or ('0,1,2,3,4,5' if args.ssm == 'gp' else '0,1,2')
    out = open(args.out, 'w') if args.out else None
    if not torch.cuda.is_available():
        raise SystemExit('junk_sweep.py needs the GPU')
    wl = problems.baseline_workload(2)
    spec = wl.spec
    x0 = torch.tensor(wl.x0[:1, :spec.n_s], dtype=torch.float64, device=DEV)
    form = os.environ.get('SX_ROLLOUT', 'default')

    def row(**kw):
        line = json.dumps(dict(workload='cfg2', ssm=args.ssm, H=wl.horizon, P=wl.particles, iters=wl.iterations,
                               rollout_env=form, solves=args.solves, **kw))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    ssm, env = problems.build(spec, device=DEV)
    if args.ssm != 'gp':
        ssm = inner_constructor(args.ssm)(state_dimen=spec.n_s, action_dimen=spec.n_u)
        ssm.update_model(torch.tensor(spec.X, device=DEV), torch.tensor(spec.Y, device=DEV), replace_old=True)
    mpc = FusedCemMpc(ssm, env, wl.horizon, wl.particles, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)
    med, p95 = time_solves(mpc, x0, False, args.warmup, args.solves)
    row(model=type(ssm).__name__, js=0, ja=0, kernel_family=ssm.kernel_family, path='fused', median_ms=med, p95_ms=p95)
    for js in (int(j) for j in js_list.split(',')):
        ssm = junk_model(spec, js, args.ja, args.ssm)
        mpc = FusedCemMpc(ssm, env, wl.horizon, wl.particles, wl.elites, wl.iterations, device=DEV, init_std=wl.init_std)
        common = dict(model='JunkDimensionsSSM', js=js, ja=args.ja, kernel_family=ssm.kernel_family,
                      query_shift=ssm.query_shift)
        if ssm.kernel_family != 'stepwise':
            med, p95 = time_solves(mpc, x0, False, args.warmup, args.solves)
            row(path='fused', median_ms=med, p95_ms=p95, stepwise_fallbacks=mpc.stepwise_fallbacks, **common)
        if not args.no_stepwise:
            med, p95 = time_solves(mpc, x0, True, max(1, args.warmup // 4), args.solves)
            row(path='stepwise', median_ms=med, p95_ms=p95, **common)


if __name__ == '__main__':
    main()
