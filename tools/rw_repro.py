"""One fused rollout per (n_s, n_u, N) on a synthetic problem, checked against the oracle, each in a child process with its
stderr kept, stopping at the first failure.  SX_ROLLOUT=rh|rw|stream (+ SX_ROLLOUT_STRICT=1) picks the kernel form: this is
how the suite covers the forms that are not the default.   python tools/rw_repro.py [n_s,n_u[,N] ...]
Options (each shape runs every combination; without them: H = 5, every state constrained, the affine objective, the box):
--horizons=1,2,5  --con-modes=0,1 (SX_CON_TERMINAL, SX_CON_ALL_STATES)  --obj-modes=0,1  --rows=m (a general polytope of m
rows whose last row cuts the particles, oracle/cases.py)  --particles=P (53)  --problems=E (1)  --q0 (a start ellipsoid per
problem)  --elites (every combination also samples its actions from elite rows, sx_cem_rollout_elites: the refit against
oracle.cem.refit, the actions against mean + std noise, the launch bit for bit against the plain entry given that refit)
--timeout=S (120 s per child)  --refit-bound (instead of the combinations: one elite-row rollout at the longest horizon the
refit prologue's scratch holds, 2 H n_u = 256 (1 + n_s), on a contracting prior, without trajectories; the costs of whole
tiles -- the first, one of the second pass of the persistent grid, each problem's first and ragged last -- against the
oracle).
TIME=1 also times one rollout of 4096 particles x 15 steps per shape (A/B of the forms on shapes no BASELINE config has)."""
import os
import subprocess
import sys

CHILD = r'''
import ctypes, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from safe_exploration_amd import _lib, problems
from safe_exploration_amd.cem_mpc import cem_rollout
from safe_exploration_amd.utils import dlqr
n_s, n_u, n_train = %(ns)d, %(nu)d, %(n)d
rng = np.random.default_rng(100 * n_s + n_u)
d_in = n_s + n_u
a = np.eye(n_s) + 0.05 * rng.normal(size=(n_s, n_s))
b = 0.3 * rng.normal(size=(n_s, n_u))
k_fb = -dlqr(a, b, np.eye(n_s), 5.0 * np.eye(n_u))[0]
X, Y = problems.synthetic_training_set(n_train, n_s, n_u, seed=n_s * 7 + n_u, scale=0.6)
ls = rng.uniform(0.6, 1.4, size=(n_s, d_in))
s, nz = rng.uniform(0.01, 0.03, size=n_s), rng.uniform(1e-5, 5e-5, size=n_s)
h_mat = np.vstack((np.eye(n_s), -np.eye(n_s)))
h_vec = np.full((2 * n_s, 1), 0.5 if n_s <= 2 else 1.2)
spec = problems.ProblemSpec('synthetic', n_s, n_u, X, Y, ls, s, nz, a, b, k_fb, rng.uniform(0.01, 0.05, size=n_s),
                            rng.uniform(0.01, 0.05, size=n_s), 2.5, h_mat, h_vec, np.full(n_u, -0.4),
                            np.full(n_u, 0.4), obj_mode=_lib.SX_OBJ_AFFINE_ABS, obj_w_abs=rng.uniform(0, 1, size=n_s),
                            obj_target=rng.normal(0, 0.1, size=n_s), obj_w_lin=rng.normal(0, 0.2, size=n_s))
if %(rows)d:
    # a better identified model, so that the ellipsoids stay small enough for a polytope to split the particles
    s *= 0.0001
    spec.outputscale, spec.l_mu, spec.l_sigma = s, 0.01 * spec.l_mu, 0.01 * spec.l_sigma
P, E, bound = %(particles)d, %(problems)d, %(bound)d
if bound:
    # the longest horizon the refit prologue's scratch holds, on a contracting prior with a small model error, so that
    # the ellipsoids stay finite over hundreds of steps
    a = 0.6 * np.eye(n_s) + 0.02 * rng.normal(size=(n_s, n_s))
    k_fb = -dlqr(a, b, np.eye(n_s), 5.0 * np.eye(n_u))[0]
    s *= 0.01
    spec.outputscale, spec.a, spec.k_fb = s, a, k_fb
    spec.l_mu, spec.l_sigma = rng.uniform(0.001, 0.003, size=n_s), rng.uniform(0.001, 0.003, size=n_s)
ssm, env = problems.build(spec, 'cuda:0')
print('built', flush=True)
from oracle import cem as ocem
from oracle.gp import ExactGP
from safe_exploration_amd.gp_reachability_pytorch import make_env
T = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device='cuda:0')
oracle_problem = lambda: problems.oracle_problem(spec, ocem)
if bound:
    Hb = 256 * (1 + n_s) // (2 * n_u)
    combos = [(Hb, 1, 1, True)]
else:
    combos = [(H, c, o, el) for H, c, o in %(combos)r for el in ((False, True) if %(elites)d else (False,))]
gp = ExactGP(X, Y, ls, s, nz)
try:     # (the oracle's small per-step solves run faster on one BLAS thread)
    from threadpoolctl import threadpool_limits
    threadpool_limits(1)
except ImportError:
    pass
cu = torch.cuda.get_device_properties(0).multi_processor_count
tpp = (P + 15) // 16
# whole tiles by global index: the first, one of the second pass of a grid of min(E tpp, cu) workgroups, each problem's
# first and ragged last
tiles = sorted({0, min(cu + 1, E * tpp - 1)} | {e * tpp for e in range(E)} | {e * tpp + tpp - 1 for e in range(E)})
for H, con_mode, obj_mode, elites in combos:
    if elites:
        k = 9
        rows = np.concatenate([np.zeros((E, k, 2)), rng.normal(0.0, 0.25, size=(E, k, H * n_u))], axis=2)
        noise = rng.normal(size=(E, P, H, n_u))
        fits = [ocem.refit(rows[e, :, 2:].reshape(k, H, n_u)) for e in range(E)]
        acts = np.stack([fits[e][0][None] + fits[e][1][None] * noise[e] for e in range(E)])
    else:
        acts = rng.normal(0, 0.25, size=(E, P, H, n_u))
    x0 = rng.normal(0, 0.02, size=(E, n_s))
    q0 = np.stack([np.eye(n_s) * 1e-4 * (e + 1) for e in range(E)]) if %(q0)d else None
    q0e = lambda e: None if q0 is None else q0[e]
    if %(rows)d and not bound:
        # a general polytope chosen from the oracle's trajectories of these particles (which the polytope does not change)
        from oracle import cases
        refs = [ocem.rollout(oracle_problem(), gp, x0[e], acts[e], q0e(e)) for e in range(E)]
        rp, rq = np.concatenate([r.traj_p for r in refs]), np.concatenate([r.traj_q for r in refs])
        # (from at most ~256 particles per problem: active_polytope's search grows faster than linearly with them)
        sub = np.concatenate([np.arange(e * P, (e + 1) * P, max(1, P // 256)) for e in range(E)])
        spec.h_mat, spec.h_vec = cases.active_polytope(np.random.default_rng(H), rp[sub], rq[sub], x0, q0, m=%(rows)d)
        assert cases.min_abs_distance(rp, rq, spec.h_mat, spec.h_vec) > 1e-9
        crossed = cases.crossings(rp, rq, spec.h_mat, spec.h_vec)
        assert crossed.any(1).any() and not crossed.any(1).all(), 'no split of the particles'
        assert all((crossed[:, r] & (crossed.sum(1) == 1)).any() for r in cases.cutting_rows(%(rows)d)), 'a cutting row'
        if H > 1:   # (the two constraint modes differ on some particle)
            costs = []
            for mode in (0, 1):
                spec.con_mode = mode
                costs.append(np.concatenate([ocem.rollout(oracle_problem(), gp, x0[e], acts[e], q0e(e)).con_cost
                                             for e in range(E)]))
            assert (costs[0] != costs[1]).any(), 'the constraint modes agree'
    spec.con_mode, spec.obj_mode = con_mode, obj_mode
    env = make_env(n_s, n_u, a=a, b=b, k_fb=k_fb, l_mu=spec.l_mu, l_sigma=spec.l_sigma, beta=spec.beta, h_mat=spec.h_mat,
                   h_vec=spec.h_vec, u_min=spec.u_min, u_max=spec.u_max, obj_mode=obj_mode, obj_w_abs=spec.obj_w_abs,
                   obj_target=spec.obj_target, obj_w_lin=spec.obj_w_lin, con_mode=con_mode)
    full = not bound
    q0t = None if q0 is None else T(q0)
    if elites:
        r = cem_rollout(ssm, env, T(x0), H, elite_rows=T(rows), noise=T(noise), q0=q0t, want_dist=True, want_traj=full,
                        want_sigma=full)
        for e in range(E):
            np.testing.assert_allclose(r['mean'][e].cpu().numpy(), fits[e][0], rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(r['std'][e].cpu().numpy(), fits[e][1], rtol=1e-12, atol=1e-15)
        # (every tile refits on its own: its actions against mean + std noise from the published refit)
        host = r['mean'].cpu().numpy()[:, None] + r['std'].cpu().numpy()[:, None] * noise
        np.testing.assert_allclose(r['actions'].cpu().numpy(), host, rtol=1e-15, atol=1e-16)
        acts = r['actions'].cpu().numpy()
        r2 = cem_rollout(ssm, env, T(x0), H, mean=r['mean'], std=r['std'], noise=T(noise), q0=q0t, want_traj=full,
                         want_sigma=full)
        for key in ('actions', 'obj_cost', 'con_cost', 'status') + (('traj', 'sigma') if full else ()):
            torch.testing.assert_close(r[key], r2[key], rtol=0, atol=0, msg='elites against the plain entry: ' + key)
    else:
        r = cem_rollout(ssm, env, T(x0), H, actions=T(acts), q0=q0t, want_traj=True, want_sigma=True)
    torch.cuda.synchronize()
    print('rollout ok', float(r['obj_cost'].sum()), int(r['status'].item()), flush=True)
    # against the oracle (the checker): trajectory centres and shapes, variances, costs (at the refit bound: the costs of
    # whole tiles)
    st = 0
    for e in range(E):
        idx = np.arange(P) if full else np.concatenate(
            [np.arange(16 * (t - e * tpp), min(16 * (t - e * tpp) + 16, P)) for t in tiles if t // tpp == e])
        if not idx.size:
            continue
        ref = ocem.rollout(oracle_problem(), gp, x0[e], acts[e][idx], q0e(e))
        st |= ref.status
        if full:
            traj = r['traj'][e].cpu().numpy()
            np.testing.assert_allclose(traj[:, :, :n_s], ref.traj_p, rtol=1e-8, atol=1e-11)
            np.testing.assert_allclose(traj[:, :, n_s:].reshape(P, H, n_s, n_s), ref.traj_q, rtol=1e-7, atol=1e-11)
            np.testing.assert_allclose(r['sigma'][e].cpu().numpy(), ref.sigma, rtol=1e-8, atol=1e-12)
        else:
            assert np.isfinite(ref.traj_q).all() and np.abs(ref.traj_q).max() < 1.0, 'the ellipsoids grow'
        np.testing.assert_allclose(r['obj_cost'][e].cpu().numpy()[idx], ref.obj_cost, rtol=1e-8, atol=1e-11)
        np.testing.assert_array_equal(r['con_cost'][e].cpu().numpy()[idx], ref.con_cost)
    assert int(r['status'].item()) == st
    form = _lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), H)
    if %(rows)d and not bound:
        print('H=%%d con_mode=%%d obj_mode=%%d m=%%d elites=%%d: %%d of %%d particles with a constraint cost'
              %% (H, con_mode, obj_mode, %(rows)d, elites, int((r['con_cost'] > 0).sum()), E * P), flush=True)
    if bound:
        print('H=%%d at the refit bound, N=%%d, n_pad=%%d, %%d tiles on %%d CUs' %% (H, n_train, ssm.device_model.n_pad,
                                                                              E * tpp, cu), flush=True)
    print('matches the oracle; form', int(form), flush=True)
if %(time)d:
    # the same model at config-2 scale (4096 particles, H = 15): one launch, timed over 20 repeats
    import time
    Pt, Ht = 4096, 15
    big = T(rng.normal(0, 0.25, size=(1, Pt, Ht, n_u)))
    for _ in range(3):
        cem_rollout(ssm, env, T(x0[:1]), Ht, actions=big)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20):
        cem_rollout(ssm, env, T(x0[:1]), Ht, actions=big)
    torch.cuda.synchronize()
    print('timed: %%.1f us per rollout of 4096 particles x 15 steps; form %%d' %% ((time.perf_counter() - t0) / 20 * 1e6,
          int(_lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), Ht))), flush=True)
'''


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    opts = dict(a[2:].split('=', 1) if '=' in a else (a[2:], '') for a in sys.argv[1:] if a.startswith('--'))
    ints = lambda key, default: [int(v) for v in opts[key].split(',')] if key in opts else default
    combos = [(H, c, o) for H in ints('horizons', [5]) for c in ints('con-modes', [1]) for o in ints('obj-modes', [1])]
    rows = ints('rows', [0])[0]
    flags = dict(particles=ints('particles', [53])[0], problems=ints('problems', [1])[0], q0=int('q0' in opts),
                 elites=int('elites' in opts), bound=int('refit-bound' in opts))
    shapes = [tuple(int(v) for v in a.split(',')) for a in sys.argv[1:] if not a.startswith('--')] or [(2, 1, 77), (1, 1, 77)]
    for shape in shapes:
        ns, nu = shape[0], shape[1]
        n = shape[2] if len(shape) > 2 else 77
        env = dict(os.environ, SX_DEBUG_SYNC='1', AMD_LOG_LEVEL=os.environ.get('AMD_LOG_LEVEL', '1'))
        p = subprocess.run([sys.executable, '-c', CHILD % dict(root=root, ns=ns, nu=nu, n=n, combos=combos, rows=rows, time=int(os.environ.get('TIME', '0')),
                                                             **flags)], capture_output=True, text=True,
                           env=env, timeout=int(opts.get('timeout', 120)))
        print(f'== n_s={ns} n_u={nu} N={n}: rc={p.returncode}')
        print(p.stdout if rows or len(combos) > 1 or flags['bound'] else p.stdout[-600:])
        print(p.stderr[-2500:])
        if p.returncode != 0:
            sys.exit(1)


if __name__ == '__main__':
    main()
