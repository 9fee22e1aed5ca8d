"""Problems with a GP each in one launch (sx_cem_rollout_multi, DESIGN.md sections 3.1 and 3.6), two shapes:

(a) BASELINE config 5's shape -- 8 problems x 4096 particles, H = 15, N = 200 -- with 8 distinct pendulum models: us per
    rollout launch of the multi-model streaming kernel, against the shared-model launch (one model for all 8 problems, the
    form the library picks for it: RH) and the shared-model streaming form (SX_ROLLOUT=stream is not needed: the multi
    launch over 8 copies of one model is that kernel).
(b) The reference's default exploration shape (experiments/sacred_helper.py:84-87, utils_config.py:35-49) -- 6 scenarios,
    20 particles, H = 2, 3 elites, 8 iterations, N from 60 to 400 -- wall time of one synchronous multi-model solve
    (MultiModelCemMpc.get_actions_multi) against six sequential FusedCemMpc.get_actions calls.

--ssm nn | mc_dropout runs both shapes with the feature-space GP ('nn' kernel, sx_cem_rollout_feat_multi) or the MC-dropout
ensemble (the reference's default 64 x 64 network with 30 members, sx_cem_rollout_mlp_multi) instead of the exact RBF GP
(--ssm gp, the default).  Shape (a) then compares the multi launch with the same kernel over one shared model (the multi
launch over 8 copies of one model) and with the plain single-model launch over the 8 problems.

Prints one JSON line.  Environment: REPS (timed repetitions, default 50)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_exploration_amd import _lib, problems  # noqa: E402
from safe_exploration_amd.cem_mpc import FusedCemMpc, GpModelTable, MultiModelCemMpc, cem_rollout, cem_rollout_multi  # noqa: E402

dev = torch.device('cuda:0')
REPS = int(os.environ.get('REPS', 50))


def launch_us(fn, reps=REPS):
    """Median us of one launch from a pair of events around each of `reps` launches (after 3 warm-up launches)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return statistics.median(out)


def wall_ms(fn, reps=REPS):
    """Median ms of `reps` synchronous calls (after 3 warm-up calls)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


class Conf:
    exact_gp_training_iterations = 0
    exact_gp_kernel = 'nn'
    nn_kernel_layers = [16, 16]
    mc_dropout_training_iterations = 20
    mc_dropout_hidden_features = [64, 64]
    mc_dropout_num_samples = 30
    mc_dropout_predict_std = False
    mc_dropout_reinitialize = False
    mc_dropout_type = 'fixed'
    mc_dropout_concrete_initial_probability = 0.1
    mc_dropout_fixed_probability = 0.1
    mc_dropout_on_input = True
    mc_dropout_lengthscale = 1e-4
    device = str(dev)


def build_models(ssm_kind, sizes, seed0):
    """(models, sx_env) for pendulum problems of the given training-set sizes: problem e from seed seed0 + e (its own data,
    and for the networks its own initialisation and masks)."""
    specs = [problems.pendulum(n_train=N, seed=seed0 + e, ard=True) for e, N in enumerate(sizes)]
    env = problems.build(specs[0], dev)[1]
    if ssm_kind == 'gp':
        return [problems.build(s, dev)[0] for s in specs], env
    from safe_exploration_amd.ssm_cem.dropout_ssm_cem import McDropoutSSM
    from safe_exploration_amd.ssm_cem.gp_ssm_cem import GpCemSSM
    models = []
    for e, spec in enumerate(specs):
        conf = type('C', (Conf,), dict(nn_kernel_seed=e, mc_dropout_seed=e))()
        ssm = GpCemSSM(conf, 2, 1) if ssm_kind == 'nn' else McDropoutSSM(conf, 2, 1)
        if ssm_kind == 'nn':
            ssm.set_hyperparameters(kernel_scale=0.5, noise=2e-3)
        ssm.update_model(torch.tensor(spec.X, device=dev), torch.tensor(spec.Y, device=dev), replace_old=True)
        models.append(ssm)
    return models, env


def shape_a(ssm_kind='gp'):
    if ssm_kind != 'gp':
        return shape_a_models(ssm_kind)
    E, P, H = 8, 4096, 15
    built = [problems.build(problems.pendulum(n_train=200, seed=s, ard=True), dev) for s in range(E)]
    ssms, env = [b[0] for b in built], built[0][1]
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x0 = 0.05 * torch.randn((E, 2), dtype=torch.float64, device=dev, generator=g)
    mean = torch.zeros((E, H, 1), dtype=torch.float64, device=dev)
    std = torch.full((E, H, 1), 0.1, dtype=torch.float64, device=dev)
    noise = torch.randn((E, P, H, 1), dtype=torch.float64, device=dev, generator=g)
    status = torch.zeros(E, dtype=torch.int32, device=dev)
    table, shared_table = GpModelTable(), GpModelTable()
    form = _lib.lib().sx_cem_rollout_form(ctypes.byref(ssms[0].device_model), H)
    multi = launch_us(lambda: cem_rollout_multi(ssms, env, x0, H, mean=mean, std=std, noise=noise, status=status,
                                                table=table))
    shared_stream = launch_us(lambda: cem_rollout_multi([ssms[0]] * E, env, x0, H, mean=mean, std=std, noise=noise,
                                                        status=status, table=shared_table))
    shared = launch_us(lambda: cem_rollout(ssms[0], env, x0, H, mean=mean, std=std, noise=noise, status=status[:1]))
    return dict(problems=E, particles=P, horizon=H, n_train=200, shared_form={0: 'STREAM', 1: 'RW', 2: 'RH', 3: 'BYOUT',
                                                                            4: 'BIG'}.get(form, form),
                multi_us=round(multi, 2), shared_us=round(shared, 2), shared_stream_us=round(shared_stream, 2),
                multi_over_shared=round(multi / shared, 4))


def shape_a_models(ssm_kind):
    """shape (a) for the feature GP / the ensemble: the multi launch, the same kernel over one shared model, the plain
    launch (E problems of one model)"""
    E, P, H = 8, 4096, 15
    ssms, env = build_models(ssm_kind, [200] * E, 0)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x0 = 0.05 * torch.randn((E, 2), dtype=torch.float64, device=dev, generator=g)
    mean = torch.zeros((E, H, 1), dtype=torch.float64, device=dev)
    std = torch.full((E, H, 1), 0.1, dtype=torch.float64, device=dev)
    noise = torch.randn((E, P, H, 1), dtype=torch.float64, device=dev, generator=g)
    status = torch.zeros(E, dtype=torch.int32, device=dev)
    family = ssms[0].kernel_family
    table, shared_table = GpModelTable(family), GpModelTable(family)
    multi = launch_us(lambda: cem_rollout_multi(ssms, env, x0, H, mean=mean, std=std, noise=noise, status=status,
                                                table=table))
    shared_multi = launch_us(lambda: cem_rollout_multi([ssms[0]] * E, env, x0, H, mean=mean, std=std, noise=noise,
                                                       status=status, table=shared_table))
    shared = launch_us(lambda: cem_rollout(ssms[0], env, x0, H, mean=mean, std=std, noise=noise, status=status[:1]))
    return dict(ssm=ssm_kind, problems=E, particles=P, horizon=H, n_train=200, multi_us=round(multi, 2),
                shared_multi_us=round(shared_multi, 2), shared_us=round(shared, 2),
                multi_over_shared=round(multi / shared, 4))


def shape_b(ssm_kind='gp'):
    E, P, H, k, iters = 6, 20, 2, 3, 8
    sizes = [60, 120, 180, 250, 320, 400]
    ssms, env = build_models(ssm_kind, sizes, 1)
    solvers = [FusedCemMpc(ssm, env, H, P, k, iters, device=dev, seed=e, init_std=0.3) for e, ssm in enumerate(ssms)]
    multi = MultiModelCemMpc(ssms, env, H, P, k, iters, device=dev, solvers=solvers)
    rng = np.random.default_rng(4)
    flat = torch.zeros((E, 6), dtype=torch.float64, device=dev)
    flat[:, :2] = torch.tensor(rng.normal(0, 0.03, size=(E, 2)), device=dev)
    t_multi = wall_ms(lambda: multi.get_actions_multi(flat))
    t_seq = wall_ms(lambda: [s.get_actions(flat[e:e + 1]) for e, s in enumerate(solvers)])
    assert multi.per_model_solves == 0, 'the multi-model solve fell back to one solve per model'
    return dict(ssm=ssm_kind, scenarios=E, particles=P, horizon=H, elites=k, iterations=iters, n_train=sizes,
                multi_solve_ms=round(t_multi, 3), sequential_ms=round(t_seq, 3), speedup=round(t_seq / t_multi, 3))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--ssm', choices=('gp', 'nn', 'mc_dropout'), default='gp')
    kind = ap.parse_args().ssm
    print(json.dumps(dict(a=shape_a(kind), b=shape_b(kind))))
