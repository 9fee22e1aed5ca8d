"""The Kstar phase of the resident rollout kernels (csrc/sx_rollout_rw.hpp: rw_kstar_setup, rw_kstar_phase) reads the centred
training rows from a PERMUTED image -- a lane's two rows of a trip side by side, one 16-byte-aligned piece -- and requests
its LDS operands in an order of its own.  Neither may change a single bit of a result: the same operations meet the same
values in the same order.  So fused rollouts (sx_cem_rollout, trajectories and variances requested) are compared

  * BIT FOR BIT with the arrays the library of the commit before the change produced on the same inputs
    (tests/golden/kstar_layout_parent.npz: inputs and outputs; tests/golden/make_kstar_layout_parent.py wrote it), and
  * with the oracle at rtol = atol = 1e-9 -- the recorded arrays are no reference of their own.

Shapes, the smallest that can break the image: N in {1, 7, 8, 9, 15, 16, 17, 200} -- one row, either side of a pair of 8
rows (the unit of the image and of a trip), either side of a 16-row block, config 2's size --, P in {1, 16, 17} (one lane,
a full tile, a second tile of one particle), H in {1, 2} (the step-0 share of every wave, the later steps' shares).
(n_s, n_u) = (1, 1) and (2, 1) on the 8-wave form (pieces of 6 and 10 doubles), (3, 1) with N = 77 on the 4-wave form
(14 doubles), each form forced through SX_ROLLOUT in a child process of its own (the library reads the switch once).  Two
more cases at (2, 1), N = 17 on the 8-wave form: a NaN start state (the one-entry NaN table) and a start state 50
length-scales outside the data (the clamped exponent).

    python tests/test_gpu_kstar_layout.py FORM IN.npz OUT.npz      the child: every case of FORM, outputs to OUT.npz
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kstar_layout_parent.npz')
SIZES = (1, 7, 8, 9, 15, 16, 17, 200)
PARTICLES = (1, 16, 17)
HORIZONS = (1, 2)
FORM_ID = {'rh': 2, 'rw': 1}                    # sx_cem_rollout_form's answer for the 8-wave and the 4-wave kernel
OUTPUTS = ('traj', 'sigma', 'obj_cost', 'con_cost', 'status')
# (form, n_s, n_u, N, kind): one model each; every group runs P x H
GROUPS = [('rh', ns, nu, n, 'plain') for ns, nu in ((1, 1), (2, 1)) for n in SIZES] + \
         [('rh', 2, 1, 17, 'nan'), ('rh', 2, 1, 17, 'far'), ('rw', 3, 1, 77, 'plain')]


def group_id(g):
    return '%s-%d-%d-N%d-%s' % g


def cases_of(g):
    return [(P, H) for P in PARTICLES for H in HORIZONS]


def case_key(g, P, H):
    return '%s/P%d/H%d' % (group_id(g), P, H)


def make_inputs():
    """The inputs of every case (the script beside the recorded file calls this once; the tests read the file)."""
    sys.path.insert(0, ROOT)
    from safe_exploration_amd import problems
    from safe_exploration_amd.utils import dlqr
    d = {}
    for ns, nu in sorted({(g[1], g[2]) for g in GROUPS}):
        rng = np.random.default_rng(100 * ns + nu)
        a = np.eye(ns) + 0.05 * rng.normal(size=(ns, ns))
        b = 0.3 * rng.normal(size=(ns, nu))
        s = '%d-%d/' % (ns, nu)
        d[s + 'a'], d[s + 'b'] = a, b
        d[s + 'k_fb'] = -dlqr(a, b, np.eye(ns), 5.0 * np.eye(nu))[0]
        d[s + 'ls'] = rng.uniform(0.6, 1.4, size=(ns, ns + nu))
        d[s + 'outputscale'], d[s + 'noise'] = rng.uniform(0.01, 0.03, size=ns), rng.uniform(1e-5, 5e-5, size=ns)
        d[s + 'l_mu'], d[s + 'l_sigma'] = rng.uniform(0.01, 0.05, size=ns), rng.uniform(0.01, 0.05, size=ns)
        d[s + 'obj_w_abs'], d[s + 'obj_target'] = rng.uniform(0, 1, size=ns), rng.normal(0, 0.1, size=ns)
        d[s + 'obj_w_lin'] = rng.normal(0, 0.2, size=ns)
    for g in GROUPS:
        form, ns, nu, n, kind = g
        m = '%d-%d-N%d/' % (ns, nu, n)
        if m + 'X' not in d:
            d[m + 'X'], d[m + 'Y'] = problems.synthetic_training_set(n, ns, nu, seed=ns * 7 + nu + 31 * n, scale=0.6)
        rng = np.random.default_rng(sum(ord(ch) for ch in group_id(g)))
        for P, H in cases_of(g):
            x0 = rng.normal(0, 0.02, size=(1, ns))
            if kind == 'nan':
                x0[0, ns - 1] = np.nan
            elif kind == 'far':
                x0 = x0 + 50.0 * d['%d-%d/ls' % (ns, nu)].max(0)[None, :ns]
            d[case_key(g, P, H) + '/x0'] = x0
            d[case_key(g, P, H) + '/actions'] = rng.normal(0, 0.25, size=(1, P, H, nu))
    return d


def spec_of(d, g):
    from safe_exploration_amd import _lib, problems
    form, ns, nu, n, kind = g
    s, m = '%d-%d/' % (ns, nu), '%d-%d-N%d/' % (ns, nu, n)
    h_mat = np.vstack((np.eye(ns), -np.eye(ns)))
    h_vec = np.full((2 * ns, 1), 0.5 if ns <= 2 else 1.2)
    return problems.ProblemSpec('synthetic', ns, nu, d[m + 'X'], d[m + 'Y'], d[s + 'ls'], d[s + 'outputscale'], d[s + 'noise'],
                                d[s + 'a'], d[s + 'b'], d[s + 'k_fb'], d[s + 'l_mu'], d[s + 'l_sigma'], 2.5, h_mat, h_vec,
                                np.full(nu, -0.4), np.full(nu, 0.4), obj_mode=_lib.SX_OBJ_AFFINE_ABS,
                                obj_w_abs=d[s + 'obj_w_abs'], obj_target=d[s + 'obj_target'], obj_w_lin=d[s + 'obj_w_lin'])


def run_form(form, inputs_path, out_path):
    """The child: every case of `form` through sx_cem_rollout (this process has SX_ROLLOUT=form), outputs to `out_path`."""
    import ctypes

    import torch
    sys.path.insert(0, ROOT)
    from safe_exploration_amd import _lib, problems
    from safe_exploration_amd.cem_mpc import cem_rollout
    d = np.load(inputs_path)
    T = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device='cuda:0')
    out = {}
    for g in GROUPS:
        if g[0] != form:
            continue
        ssm, env = problems.build(spec_of(d, g), 'cuda:0')
        for P, H in cases_of(g):
            key = case_key(g, P, H)
            got = int(_lib.lib().sx_cem_rollout_form(ctypes.byref(ssm.device_model), H))
            assert got == FORM_ID[form], f'{key}: form {got}'
            r = cem_rollout(ssm, env, T(d[key + '/x0']), H, actions=T(d[key + '/actions']), want_traj=True, want_sigma=True)
            torch.cuda.synchronize()
            for name in OUTPUTS:
                out[key + '/' + name] = r[name].cpu().numpy()
    np.savez(out_path, **out)


def run_children(inputs_path, out_dir, extra_env=None):
    """Both forms' children side by side; {form: outputs}."""
    procs = {}
    for form in FORM_ID:
        env = dict(os.environ, SX_ROLLOUT=form, SX_ROLLOUT_STRICT='1', **(extra_env or {}))
        procs[form] = subprocess.Popen([sys.executable, os.path.abspath(__file__), form, inputs_path,
                                        os.path.join(out_dir, form + '.npz')], env=env, stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    outs = {}
    for form, p in procs.items():
        text = p.communicate(timeout=600)[0]
        assert p.returncode == 0, f'{form}: rc={p.returncode}\n{text[-3000:]}'
        outs[form] = dict(np.load(os.path.join(out_dir, form + '.npz')))
    return outs


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope='module')
def device_outputs(tmp_path_factory):
    return run_children(GOLDEN, str(tmp_path_factory.mktemp('kstar_layout')))


@pytest.mark.gpu
@pytest.mark.parametrize('g', GROUPS, ids=group_id)
def test_bit_for_bit_with_the_parent_commit(g, golden, device_outputs):
    for P, H in cases_of(g):
        for name in OUTPUTS:
            key = case_key(g, P, H) + '/' + name
            got, want = device_outputs[g[0]][key], golden[key]
            assert got.shape == want.shape and got.dtype == want.dtype, key
            assert got.tobytes() == want.tobytes(), f'{key}: {int((got.view(np.uint8) != want.view(np.uint8)).sum())} bytes differ'


@pytest.mark.gpu
@pytest.mark.parametrize('g', GROUPS, ids=group_id)
def test_against_the_oracle(g, golden, device_outputs):
    sys.path.insert(0, ROOT)
    from oracle import cem as ocem
    from oracle.gp import ExactGP
    from safe_exploration_amd import problems
    form, ns, nu, n, kind = g
    spec = spec_of(golden, g)
    gp = ExactGP(spec.X, spec.Y, spec.lengthscale, spec.outputscale, spec.noise)
    for P, H in cases_of(g):
        key = case_key(g, P, H)
        r = {name: device_outputs[form][key + '/' + name] for name in OUTPUTS}
        if kind == 'nan':
            # a NaN coordinate poisons every row of Kstar, hence the posterior: every centre, variance and cost is NaN (the
            # first step's shape matrix keeps its structural zeros); the oracle's numpy chain is not defined on such a start
            assert np.isnan(r['traj'][..., :ns]).all() and np.isnan(r['sigma']).all() and np.isnan(r['obj_cost']).all(), key
            continue
        ref = ocem.rollout(problems.oracle_problem(spec, ocem), gp, golden[key + '/x0'][0], golden[key + '/actions'][0])
        tol = dict(rtol=1e-9, atol=1e-9)
        traj = r['traj'][0]
        np.testing.assert_allclose(traj[:, :, :ns], ref.traj_p, err_msg=key, **tol)
        np.testing.assert_allclose(traj[:, :, ns:].reshape(P, H, ns, ns), ref.traj_q, err_msg=key, **tol)
        np.testing.assert_allclose(r['sigma'][0], ref.sigma, err_msg=key, **tol)
        np.testing.assert_allclose(r['obj_cost'][0], ref.obj_cost, err_msg=key, **tol)
        np.testing.assert_array_equal(r['con_cost'][0], ref.con_cost, err_msg=key)
        assert int(r['status'].item()) == ref.status, key


if __name__ == '__main__':
    run_form(sys.argv[1], sys.argv[2], sys.argv[3])
