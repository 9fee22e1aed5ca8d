"""Randomised check of sx_cem_rank_refit (both kernels, chosen by shape and output mode) against the oracle's ranking: random
shapes, few distinct constraint costs, exact ties, NaNs, +-inf, strided candidate rows, all four output modes.  elite_idx is
compared exactly with the order the kernel that ran promises.  The tool stands alone: `kernel_of` and `order_of` restate
the launcher's rule and the order contracts here; tests/test_rank_host.py holds them against
tests/rank_reference.py's, so the two cannot drift apart.
python tools/rank_fuzz.py [cases] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cem as ocem  # noqa: E402  (checker only)

KERNELS = ('count', 'select4', 'select8', 'select16')
MODES = ((True, True), (True, False), (False, True), (False, False))     # (rows, refit)


def kernel_of(E, P, rows, refit):
    """The kernel sx_cem_rank_refit takes (csrc/sx_rank.hip): counting where sx_cem_rank_counts says so and the refit, if
    asked for, has the rows to read back; else one workgroup per problem with 4 / 8 / 16 candidates per thread."""
    from safe_exploration_amd import _lib
    if int(_lib.lib().sx_cem_rank_counts(E, P)) != 0 and (rows or not refit):
        return 'count'
    slots = -(-P // 1024)
    return 'select4' if slots <= 4 else 'select8' if slots <= 8 else 'select16'


def order_of(con, obj, k, kernel):
    """elite_idx of one problem: counting returns rank order, one workgroup the best first and the rest in index order."""
    order = [int(i) for i in ocem.rank(con, obj, k)]
    return order if kernel == 'count' else [order[0]] + sorted(order[1:])


def draw(rng):
    """One random case: (E, P, k, L, con, obj, act, strided, rows, refit)."""
    E = int(rng.choice([1, 1, 2, 3, 5, 8, 70]))
    P = int(rng.choice([rng.integers(1, 40), rng.integers(40, 600), rng.integers(600, 8193), rng.integers(8193, 16385)],
                       p=[.2, .3, .4, .1]))
    L = int(rng.choice([1, 3, 15, 30, 33, 70]))
    if E == 70:                     # many problems: bounded inputs (they all reach cem_rank_kernel<4>)
        P, L = min(P, 2000), min(L, 15)
    elif E >= 5:
        L = min(L, 30)
    k = int(rng.integers(1, min(P, 2048) + 1)) if rng.random() < .3 else max(1, min(P, 2048) // int(rng.integers(2, 20)))
    con = rng.choice([0., 0., 0., 3., 10., 13., 20., 23.], size=(E, P))
    if rng.random() < .3:
        con = rng.normal(size=(E, P)).round(int(rng.integers(0, 3)))         # arbitrary doubles, many ties
    obj = rng.normal(size=(E, P))
    if rng.random() < .5:
        obj = obj.round(int(rng.integers(0, 3)))                             # exact ties in the objective too
    for arr in (con, obj):
        if rng.random() < .3:
            arr[rng.integers(0, E), rng.integers(0, P)] = rng.choice([np.nan, np.inf, -np.inf])
    act = rng.normal(size=(E, P, L))
    strided = bool(rng.random() < .3)
    rows, refit = MODES[int(rng.integers(0, 4))]
    return E, P, k, L, con, obj, act, strided, rows, refit


def kernels_of(cases, seed):
    """How many of the first `cases` cases of `seed` each kernel takes (no GPU: the launcher's rule is host code)."""
    rng = np.random.default_rng(seed)
    took = dict.fromkeys(KERNELS, 0)
    for _ in range(cases):
        E, P, _, _, _, _, _, _, rows, refit = draw(rng)
        took[kernel_of(E, P, rows, refit)] += 1
    return took


def main(cases, seed):
    import torch
    from safe_exploration_amd.cem_mpc import cem_rank_refit
    rng = np.random.default_rng(seed)
    dev = torch.device('cuda:0')
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    bad = 0
    took = dict.fromkeys(KERNELS, 0)
    for case in range(cases):
        E, P, k, L, con, obj, act, strided, rows, refit = draw(rng)
        kernel = kernel_of(E, P, rows, refit)
        took[kernel] += 1
        if strided:       # candidate-row layout: [con, obj, actions...] rows, as after the multi-GPU exchange
            flat = T(np.concatenate((con[..., None], obj[..., None], act), axis=2)).reshape(-1)
            out = cem_rank_refit(flat, flat[1:], flat[2:], k, cost_stride=2 + L, act_stride=2 + L, row_len=L, num_candidates=P,
                                 num_problems=E, want_rows=rows, want_refit=refit)
        else:
            out = cem_rank_refit(T(con), T(obj), T(act), k, want_rows=rows, want_refit=refit)
        out = {name: (t.cpu().numpy() if t is not None else None) for name, t in out.items()}
        for e in range(E):
            want = order_of(con[e], obj[e], k, kernel)
            got = out['elite_idx'][e]
            ok = got.tolist() == want
            ok = ok and np.array_equal(bits(out['best'][e]), bits(act[e][want[0]])) and int(out['best_ok'][e]) == int(con[e][want[0]] == 0)
            if rows:
                r = out['elite_rows'][e]
                ok = ok and np.array_equal(bits(r[:, 2:]), bits(act[e][want])) and np.array_equal(r[:, 0], con[e][want], equal_nan=True) \
                    and np.array_equal(r[:, 1], obj[e][want], equal_nan=True)
            if refit:
                m, sd = ocem.refit(act[e][want])
                ok = ok and np.allclose(out['mean'][e], m, rtol=1e-11, atol=1e-13) and np.allclose(out['std'][e], sd, rtol=1e-11, atol=1e-13)
            if not ok:
                bad += 1
                print(f'MISMATCH case {case}: E={E} P={P} k={k} L={L} strided={strided} rows={rows} refit={refit} '
                      f'kernel={kernel} problem {e}', flush=True)
    print(f'{cases} cases (' + ', '.join(f'{k} {n}' for k, n in took.items()) + f'), {bad} mismatches')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 300, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
