"""Generates tests/golden/multistep_pendulum.npz and multistep_cartpole.npz by RUNNING THE REFERENCE in the build
container.  Not run by the test-suite.

    python tests/golden/make_golden_multistep.py     # needs /root/reference; writes the .npz files next to this script

What runs from the reference, unmodified (imported from /root/reference, never copied):
    safe_exploration/gp_reachability.py   multistep_reachability (:168-221) over its numpy onestep_reachability (:19-165)
with the name-only placeholders of make_golden.py for the modules that are not installed here, and a numpy stand-in SSM
over the closed-form exact GP of ``oracle/gp.py`` (hyper-parameters stored in the fixture), in the single-item shape
conventions of the reference's numpy path.  As with the one-step fixtures, what is pinned is the REACHABILITY arithmetic
under a gain per step; the GP values stay "parity unpinned" (DESIGN.md).

Both fixtures: a linear prior, c_safety = 2, l_mu = l_sigma = 0.05, 12 rollouts of n = 4 steps, gains and feed-forward
terms 0.1 randn, starts 0.1 U(-1, 1).  The reference's compute_remainder_overapproximations asserts that a general
eigen-solver returned no imaginary part (utils.py:137), which rounding alone can trip at n_s = 4: a rollout whose reference
run raises that assertion is dropped, and at least 8 of the 12 must remain.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

R, N_STEPS, KEEP = 12, 4, 8


def main():
    torch.set_default_dtype(torch.double)
    from make_golden import _install_placeholders
    _install_placeholders()
    sys.path.insert(0, REF)
    import safe_exploration.gp_reachability as reach_np
    from safe_exploration.state_space_models import StateSpaceModel

    from oracle.gp import ExactGP

    class NumpySSM(StateSpaceModel):
        """Single-item numpy adapter over the closed-form GP (make_golden.py's)."""

        def __init__(self, gp, n_s, n_u):
            super().__init__(n_s, n_u)
            self.gp = gp

        def predict(self, states, actions, jacobians=False, full_cov=False):
            m, v, j = self.gp.predict(np.concatenate((states, actions), axis=1), jacobians)
            return (m.T, v[0], j[0]) if jacobians else (m.T, v[0])

        def linearize_predict(self, *a, **k):
            raise NotImplementedError

        def get_reverse(self, seed):
            raise NotImplementedError

        def get_linearize_reverse(self, seed):
            raise NotImplementedError

        def update_model(self, *a, **k):
            raise NotImplementedError

    def multistep_case(name, X, Y, n_s, n_u, ls, a, b, seed):
        rng = np.random.default_rng(seed)
        gp = ExactGP(X, Y, ls, 0.5, 1e-2)
        ssm = NumpySSM(gp, n_s, n_u)
        l_mu, l_sigma, c_safety = np.full(n_s, 0.05), np.full(n_s, 0.05), 2.0
        k_fb = 0.1 * rng.normal(size=(R, N_STEPS - 1, n_u, n_s))
        k_ff = 0.1 * rng.normal(size=(R, N_STEPS, n_u))
        p_0 = 0.1 * rng.uniform(-1, 1, size=(R, n_s))
        kept, p_all, q_all = [], [], []
        for i in range(R):
            try:
                pn, qn, pa, qa = reach_np.multistep_reachability(p_0[i][:, None], ssm, k_fb[i], k_ff[i], l_mu, l_sigma,
                                                                 c_safety=c_safety, verbose=0, a=a, b=b)
            except AssertionError as exc:
                print(f'{name}: rollout {i} dropped ({exc!r})')
                continue
            assert np.array_equal(pn.squeeze(), pa[-1]) and np.array_equal(qn, qa[-1])
            kept.append(i)
            p_all.append(pa)
            q_all.append(qa)
        assert len(kept) >= KEEP, f'{name}: the reference ran {len(kept)} of {R} rollouts'
        np.savez(os.path.join(HERE, name + '.npz'), X=X, Y=Y, ls=gp.ls, s=gp.s, noise=gp.noise, a=a, b=b, l_mu=l_mu,
                 l_sigma=l_sigma, c_safety=np.float64(c_safety), p_0=p_0[kept], k_fb=k_fb[kept], k_ff=k_ff[kept],
                 kept=np.array(kept), p_all=np.stack(p_all), q_all=np.stack(q_all))
        print(f'wrote {name}: {len(kept)} rollouts, max |Q| {np.abs(np.stack(q_all)).max():.3g}')

    ref_test = os.path.join(REF, 'safe_exploration', 'test')
    d = np.load(os.path.join(ref_test, 'invpend_data.npz'))
    rng = np.random.default_rng(125)   # (the prior of make_golden.py's pendulum cases)
    a_p, b_p = rng.uniform(0, 1, size=(2, 2)), rng.uniform(0, 1, size=(2, 1))
    multistep_case('multistep_pendulum', d['X'], d['y'], 2, 1, 1.5, a_p, b_p, 31)
    d = np.load(os.path.join(ref_test, 'data_cartpole.npz'))
    multistep_case('multistep_cartpole', d['X'], d['y'], 4, 1, 2.5, d['a'], d['b'], 32)


if __name__ == '__main__':
    main()
