"""What tests/test_gpu_big_path.py launches on the large-N path (csrc/sx_big.hpp), and the one fixed case it runs under the
A/B settings of trmm_reduce_kernel.  SX_TRMM_ORDER / SX_TRMM_VARIANT / SX_TRMM_PT are read once per process, so a setting
needs a process of its own:   python tests/big_path_case.py OUT.npz   runs the case and writes its raw outputs, with the
tiling sx_gp_big_tiling reports in that process, to OUT.npz.  Not a test module (nothing here is collected)."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import test_gpu_rollout_matrix as rm  # noqa: E402
from safe_exploration_amd import _lib  # noqa: E402

H = 2
SX_FORM_BIG = 4                                                     # include/sx_amd.h
SETTINGS = ('SX_TRMM_ORDER', 'SX_TRMM_VARIANT', 'SX_TRMM_PT')
# the A/B case: (2, 1), N = 1100 (9 row tiles), 1530 particles -- 1536 padded, so that the plain grid of either tile shape
# (18 x 24 or 18 x 12 workgroups) is a multiple of 8 and SX_TRMM_ORDER=1 does not fall back to the plain order
AB_SHAPE, AB_N, AB_P = (2, 1), 1100, 1530


def poison(ssm, nbytes):
    """NaN in every double of the workspace the wrappers hand to the next launch of `nbytes`: a slot that launch reads
    without having written it shows up in its outputs, whatever an earlier launch left there."""
    assert nbytes > 0, 'the model does not take the large-N path'
    ws = ssm.workspace(nbytes)
    ws.fill_(float('nan'))
    assert ssm.workspace(nbytes) is ws


def predict(ssm, z):
    """sx_gp_predict with Jacobians at z (numpy [P x D]) on the large-N path over a NaN-filled workspace."""
    nbytes = int(_lib.lib().sx_gp_predict_workspace_bytes(ctypes.byref(ssm.device_model), len(z)))
    poison(ssm, nbytes)
    zt = rm.T(z)
    return ssm.predict_with_jacobians(zt[:, :ssm.num_states].contiguous(), zt[:, ssm.num_states:].contiguous())


def rollout(ssm, env, x0, acts, q0):
    """sx_cem_rollout of given actions (numpy [E x P x H x n_u]) from the ellipsoids (x0, q0) in the three-launch form over a
    NaN-filled workspace."""
    lib, model = _lib.lib(), ssm.device_model
    E, P = acts.shape[:2]
    assert acts.shape[2] == H and lib.sx_cem_rollout_form(ctypes.byref(model), H) == SX_FORM_BIG
    poison(ssm, int(lib.sx_cem_rollout_workspace_bytes(ctypes.byref(model), E, P, H)))
    from safe_exploration_amd.cem_mpc import cem_rollout
    return cem_rollout(ssm, env, rm.T(x0), H, actions=rm.T(acts), q0=rm.T(q0), want_traj=True, want_sigma=True)


def start_ellipsoids(rng, E, n_s):
    return rng.normal(0, 0.02, size=(E, n_s)), np.stack([np.eye(n_s) * 1e-4 * (e + 1) for e in range(E)])


def ab_case():
    """The A/B case's raw outputs {name: numpy array}: predict with Jacobians and a rollout of H = 2 from an ellipsoid under a
    box some particles leave, and `tiling` = (pt, order, variant, grid) of this process."""
    n_s, n_u = AB_SHAPE
    ssm, _ = rm.cached(rm.build_model, 'rbf', n_s, n_u, AB_N, 2)
    rng = np.random.default_rng(77)
    out = dict(zip(('mean', 'var', 'jac'), predict(ssm, rng.uniform(-0.5, 0.5, size=(AB_P, n_s + n_u)))))
    x0, q0 = start_ellipsoids(rng, 1, n_s)
    acts = rng.normal(0, 0.4, size=(1, AB_P, H, n_u))
    box = rm.Constraints(rm.system(n_s, n_u), np.vstack((np.eye(n_s), -np.eye(n_s))), np.full((2 * n_s, 1), 0.08),
                         np.full(n_u, -0.5), np.full(n_u, 0.5))
    r = rollout(ssm, box.env(_lib.SX_OBJ_AFFINE_ABS, _lib.SX_CON_ALL_STATES), x0, acts, q0)
    out.update({k: r[k] for k in ('obj_cost', 'con_cost', 'traj', 'sigma', 'status')})
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    t = _lib.big_tiling(ssm.device_model, AB_P)
    out['tiling'] = np.array([t['pt'], t['order'], t['variant'], t['grid']], dtype=np.int64)
    return out


if __name__ == '__main__':
    np.savez(sys.argv[1], **ab_case())
