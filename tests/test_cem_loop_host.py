"""CPU: FusedCemMpc.solve and MultiModelCemMpc.solve run one CEM iteration loop.  The rollout and ranking wrappers are
replaced by fakes that record their calls; both solves must make the same sequence for the same (E, P, H, k, iterations):
a rollout from (mean, std) first, then rollouts from the elite rows where the refit runs in the rollout's prologue, with
the rankings asking for rows or for the refit accordingly."""
import pytest
import torch

from safe_exploration_amd import _lib, cem_mpc
from safe_exploration_amd.cem_mpc import FusedCemMpc, MultiModelCemMpc


class _Ssm:
    """An exact GP as far as the host-side plan reads it (never launched: the wrappers are fakes)."""
    num_states, num_actions, kernel_family = 2, 1, 'rbf'

    def __init__(self, n_train=60):
        m = _lib.SxGpModel()
        m.n_s, m.n_u, m.n_train = 2, 1, n_train
        m.n_pad = (n_train + 1 + 2 + 1 + 15) // 16 * 16   # sx_gp.hpp: gp_n_pad
        self.device_model = m


def _fakes(monkeypatch, k, dists=None):
    """Records the calls; `dists` (a list) receives the (mean, std) every rollout from the distribution samples from.
    Ranking i (counted from 1 in `calls`) refits to mean i, std 10 i."""
    calls = []

    def rollout(x0, horizon, noise, elite_rows, status, mean=None, std=None):
        calls.append(('rollout', 'rows' if elite_rows is not None else 'dist'))
        if dists is not None and elite_rows is None:
            dists.append((mean.clone(), std.clone()))
        E, P = x0.size(0), noise.size(1)
        return dict(actions=torch.zeros((E, P, horizon, 1), dtype=torch.float64), obj_cost=torch.zeros((E, P)),
                    con_cost=torch.zeros((E, P)), traj=None, sigma=None, status=status)

    def rank(con, obj, actions, kk, want_rows=False, want_refit=True):
        assert kk == k
        calls.append(('rank', want_rows, want_refit))
        E, L, i = con.size(0), actions[0, 0].numel(), sum(c[0] == 'rank' for c in calls)
        full = lambda v, *shape: torch.full(shape, float(v), dtype=torch.float64)
        return dict(elite_rows=full(0, E, k, 2 + L) if want_rows else None, mean=full(i, E, L) if want_refit else None,
                    std=full(10 * i, E, L) if want_refit else None, best=full(0, E, L),
                    best_ok=torch.zeros(E, dtype=torch.int32))

    monkeypatch.setattr(cem_mpc, 'cem_rollout', lambda ssm, env, x0, horizon, *, noise, elite_rows=None, status=None,
                        mean=None, std=None, **kw: rollout(x0, horizon, noise, elite_rows, status, mean, std))
    monkeypatch.setattr(cem_mpc, 'cem_rollout_multi', lambda ssms, env, x0, horizon, *, noise, elite_rows=None,
                        status=None, mean=None, std=None, **kw: rollout(x0, horizon, noise, elite_rows, status, mean, std))
    monkeypatch.setattr(cem_mpc, 'cem_rank_refit_any', rank)
    return calls


@pytest.mark.parametrize('E, P, H, k, iters, in_prologue', [
    (3, 256, 5, 20, 4, True),      # the ranking counts in one launch: rows go to the next rollout's prologue
    (8, 4096, 5, 40, 3, False),    # 8 problems of 4096 candidates rank one workgroup each: the ranking refits
    (2, 256, 400, 20, 3, False),   # 2 H n_u > 256 (1 + n_s): the refit does not fit the prologue
])
def test_single_and_multi_model_solves_make_the_same_calls(monkeypatch, E, P, H, k, iters, in_prologue):
    calls = _fakes(monkeypatch, k)
    x0 = torch.zeros((E, 2), dtype=torch.float64)
    single = FusedCemMpc(_Ssm(), None, H, P, k, iters, device='cpu', init_std=0.2)
    best, ok, _, status = single.solve(x0)
    assert tuple(best.shape) == (E, H, 1) and tuple(ok.shape) == (E,) and tuple(status.shape) == (1,)
    single_calls = list(calls)
    calls.clear()
    multi = MultiModelCemMpc([_Ssm(60 + 10 * e) for e in range(E)], None, H, P, k, iters, device='cpu', init_std=0.2)
    best, ok, status = multi.solve(x0)
    assert tuple(best.shape) == (E, H, 1) and tuple(ok.shape) == (E,) and tuple(status.shape) == (E,)
    first = [('rollout', 'dist'), ('rank', in_prologue, not in_prologue)]
    later = [('rollout', 'rows' if in_prologue else 'dist'), ('rank', in_prologue, not in_prologue)]
    assert single_calls == calls == first + later * (iters - 1)


def test_refits_reach_the_next_rollout_and_the_multi_model_start_is_per_problem(monkeypatch):
    """Where the ranking refits (8 problems of 4096 particles), rollout i + 1 samples from ranking i's (mean, std); the
    multi-model solve starts problem e from solvers[e]'s distribution."""
    E, P, H, k, iters = 8, 4096, 5, 40, 3
    dists = []
    calls = _fakes(monkeypatch, k, dists)
    x0 = torch.zeros((E, 2), dtype=torch.float64)
    FusedCemMpc(_Ssm(), None, H, P, k, iters, device='cpu', init_std=0.2).solve(x0)
    calls.clear()
    solvers = [FusedCemMpc(_Ssm(60 + 10 * e), None, H, P, k, iters, device='cpu', init_std=0.1 * (e + 1))
               for e in range(E)]
    MultiModelCemMpc([s._ssm for s in solvers], None, H, P, k, iters, device='cpu', solvers=solvers).solve(x0)
    assert len(dists) == 2 * iters
    single, multi = dists[:iters], dists[iters:]
    assert torch.equal(single[0][0], torch.zeros((E, H, 1), dtype=torch.float64))
    assert torch.equal(single[0][1], torch.full((E, H, 1), 0.2, dtype=torch.float64))
    assert torch.equal(multi[0][0], torch.zeros((E, H, 1), dtype=torch.float64))
    assert torch.equal(multi[0][1], torch.tensor([0.1 * (e + 1) for e in range(E)], dtype=torch.float64)
                       .view(E, 1, 1).expand(E, H, 1))
    for i in range(1, iters):
        for mean, std in (single[i], multi[i]):
            assert tuple(mean.shape) == tuple(std.shape) == (E, H, 1)
            assert torch.all(mean == i) and torch.all(std == 10 * i)


def test_patched_sample_noise_is_called_once_per_iteration(monkeypatch):
    calls = _fakes(monkeypatch, 20)
    mpc = FusedCemMpc(_Ssm(), None, 5, 256, 20, 4, device='cpu')
    draws = []
    mpc.sample_noise = lambda episodes=1: draws.append(episodes) or torch.zeros((episodes, 256, 5, 1), dtype=torch.float64)
    mpc.solve(torch.zeros((2, 2), dtype=torch.float64))
    assert draws == [2] * 4 and mpc._last_noise is None
    assert [c for c in calls if c[0] == 'rollout'] == [('rollout', 'dist')] + [('rollout', 'rows')] * 3
