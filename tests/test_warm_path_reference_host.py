"""CPU: the warm path's reference (tests/warm_path_reference.py) against the oracle's ExactGP, against torch autograd and
against central differences of its own long-double MLL; and that it factorises every problem the GPU tests
(tests/test_gpu_warm_path.py) generate, printing cond_2(K), the smallest pivot and LAPACK's residuals (pytest -s, or a
failure's message)."""
import numpy as np
import pytest
import torch

import warm_path_reference as R
from oracle.gp import ExactGP


def test_float64_reference_agrees_with_the_oracle():
    p = R.problem(2, 2, 65)
    ref = R.reference(p)
    gp = ExactGP(p.X, p.Y, p.ls, p.s, p.noise)
    z = R.queries(p, 3, far=False)
    for got, want in ((ref.linv, gp.linv()), (ref.alpha, np.stack(gp.alpha)),
                      (R.variance_jacobian(p, ref.linv, z), gp.variance_jacobian(z)),
                      (R.mean_hessian(p, ref.alpha, z), gp.mean_hessian(z))):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.skipif(not R.HAVE_LD, reason='long double is no wider than double on this platform')
def test_long_double_reference_agrees_with_float64_to_its_conditioning():
    p = R.problem(2, 1, 97)
    f, ld = R.reference(p), R.reference(p, True)
    bound = 97 * R.EPS * max(R.cond2(K) for K in f.K)
    for key in ('linv', 'alpha', 'logdet', 'mll', 'grad'):
        assert getattr(ld, key).dtype == np.longdouble
        assert R.rel_err(getattr(f, key), getattr(ld, key)) <= bound, key
    # and the long-double factors reproduce K far below float64's rounding
    o = ld.out[0]
    assert np.abs(o.L @ o.L.T - o.K).max() < 1e-17 and np.abs(o.W @ o.L - np.eye(o.n)).max() < 1e-16


def _torch_mll_grad(p, d):
    X = torch.tensor(p.X)
    l = torch.tensor(p.ls[d], requires_grad=True)
    s = torch.tensor(p.s[d], requires_grad=True)
    noise = torch.tensor(p.noise[d], requires_grad=True)
    a = X / l
    diff = a[:, None, :] - a[None, :, :]
    K = s * torch.exp(-0.5 * (diff * diff).sum(2)) + noise * torch.eye(len(X), dtype=torch.float64)
    y = torch.tensor(p.Y[:, d])
    L = torch.linalg.cholesky(K)
    mll = -0.5 * y @ torch.cholesky_solve(y[:, None], L)[:, 0] - torch.log(torch.diagonal(L)).sum() \
        - 0.5 * len(X) * np.log(2 * np.pi)
    g = torch.autograd.grad(mll, (l, s, noise))
    return float(mll.detach()), torch.cat([g[0], g[1][None], g[2][None]]).numpy()


@pytest.mark.parametrize('n_s,n_u,n', [(2, 1, 40), (1, 5, 33)])
def test_closed_form_gradient_agrees_with_autograd(n_s, n_u, n):
    p = R.problem(n_s, n_u, n)
    ref = R.reference(p)
    for d in range(n_s):
        mll, grad = _torch_mll_grad(p, d)
        assert abs(ref.mll[d] - mll) <= 1e-8 * abs(mll)
        assert np.abs(ref.grad[d] - grad).max() <= 1e-8 * np.abs(grad).max()


@pytest.mark.skipif(not R.HAVE_LD, reason='long double is no wider than double on this platform')
def test_closed_form_gradient_agrees_with_central_differences_of_the_long_double_mll():
    p = R.problem(2, 1, 40)
    ld = R.reference(p, True)
    h = np.longdouble(1e-6)      # truncation h^2 f''' / 6 ~ 1e-12 relative, rounding 1e-19 / h = 1e-13
    for d in range(p.n_s):
        theta = np.concatenate([p.ls[d], [p.s[d]], [p.noise[d]]]).astype(np.longdouble)
        for c in range(len(theta)):
            vals = []
            for sign in (1, -1):
                t = theta.copy()
                t[c] += sign * h * theta[c]
                ls, s, noise = p.ls.astype(np.longdouble), p.s.astype(np.longdouble), p.noise.astype(np.longdouble)
                ls[d], s[d], noise[d] = t[:-2], t[-2], t[-1]
                vals.append(R.Output(p._replace(ls=ls, s=s, noise=noise), d, np.longdouble).mll)
            fd = (vals[0] - vals[1]) / (2 * h * theta[c])
            assert abs(fd - ld.grad[d, c]) <= 1e-9 * np.abs(ld.grad[d]).max(), (d, c, fd, ld.grad[d, c])


def _id(case):
    return '{}x{}-N{}-ratio{:g}'.format(*case)


@pytest.mark.parametrize('case', R.all_cases(), ids=_id)
def test_reference_factorises_every_generated_problem(case):
    n_s, n_u, n, ratio = case
    p = R.problem(*case)
    ref = R.reference(p)                     # np.linalg.cholesky raises if K is not positive definite
    assert np.isfinite(ref.linv).all() and np.isfinite(ref.alpha).all() and np.isfinite(ref.logdet).all()
    y = p.Y[:, 0]
    cond = R.cond2(ref.K[0])
    r1, r2 = R.residuals(ref.K[0], ref.linv[0], ref.alpha[0], y)
    piv = min(float(np.diag(o.L).min()) for o in ref.out)
    msg = f'cond_2(K) = {cond:.2e}, smallest pivot {piv:.1e}, max|W K W^T - I| = {r1:.1e}, max|K alpha - y|/max|y| = {r2:.1e}'
    print(msg)
    bound = 8 * n * R.EPS * cond             # a sanity bound on LAPACK itself (8: the residual's own roundings at N = 1)
    assert piv > 0 and r1 <= bound and r2 <= bound, msg
    if R.HAVE_LD and n <= R.LD_MAX_N:
        R.reference(p, True)                 # cholesky_ld raises at a non-positive pivot


@pytest.mark.parametrize('n,a,b', R.NOT_PD_CASES)
def test_not_pd_construction_fails_exactly_at_row_b(n, a, b):
    p = R.not_pd_problem(n, a, b)
    for d in range(p.n_s):
        K = R.kmat(p, d)
        assert (np.diag(K) > 0).all()
        np.linalg.cholesky(K[:b, :b])
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(K[:b + 1, :b + 1])
        with pytest.raises(np.linalg.LinAlgError, match=f'pivot {b} '):
            R.cholesky_ld(K.astype(np.longdouble))
