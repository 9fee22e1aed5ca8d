"""Polytopes for the rollout checks (TEST INFRASTRUCTURE - see oracle/__init__.py).

A constraint check only tells a kernel from a wrong one where the polytope is active: some particles leave it and some do
not, each row that cuts is the only one some particle crosses, the terminal and the every-step constraint disagree on
some particle, and no ellipsoid touches a face to within rounding (so that `con_cost` can be compared exactly).  The
trajectory of a rollout does not depend on the polytope, so `active_polytope` picks one from the oracle's trajectory of
the very particles that are to be checked.
"""
import numpy as np

from . import reachability as reach


def support(traj_p, traj_q, h):
    """h.p + sqrt(h^T Q h) per particle and step for one unit row h: traj_p [P x H x n_s], traj_q [P x H x n_s x n_s]."""
    return traj_p @ h + np.sqrt(np.einsum('i,phij,j->ph', h, traj_q, h))


def _cut(s, start, other=None, target=0.5):
    """(offset, score) of the best cut of the support values s [P x H] of one row: an offset half-way between two of them,
    above the start's support, preferring (1) particles that cross and particles that do not (nor the row `other` [P],
    "crosses another cutting row", where given), (2) particles that cross this row alone and particles that cross `other`
    alone, (3) a particle that crosses before its last step but not at it, (4) a distance of at least 1e-6 (relative) to
    every support value, (5) a share of crossing particles close to `target`."""
    H = s.shape[1]
    vals = np.unique(s.ravel())
    vals = vals[np.isfinite(vals)]
    cand, gap = 0.5 * (vals[:-1] + vals[1:]), vals[1:] - vals[:-1]
    keep = cand > start
    cand, gap = cand[keep], gap[keep]
    if cand.size == 0:
        return None
    viol_all = np.nanmax(s, 1)[None] > cand[:, None]                       # [K x P]
    viol_end = s[None, :, -1] > cand[:, None]
    other = np.zeros(s.shape[0], bool) if other is None else np.asarray(other, bool)
    frac = viol_all.mean(1)
    split = viol_all.any(1) & ~(viol_all | other[None]).all(1) & viol_end.any(1)
    alone = (viol_all & ~other[None]).any(1) & ((other[None] & ~viol_all).any(1) | ~other.any())
    differs = (viol_all & ~viol_end).any(1) if H > 1 else np.ones(cand.size, bool)
    wide = gap > 2e-6 * (1.0 + np.abs(cand))
    score = [(bool(split[k]), bool(alone[k]), bool(differs[k]), bool(wide[k]), -abs(frac[k] - target))
             for k in range(cand.size)]
    i = max(range(cand.size), key=lambda k: score[k])
    return cand[i], score[i]


def cutting_rows(m):
    """The rows of an m-row polytope that cut the particles: the last one and, for m > 1, one in another group of the
    lanes that check rows r, r + 4, r + 8, r + 12 side by side (sx_rollout_rw.hpp), in the last pass of the row loop where
    there is one beyond row 11, i.e. rows 12 - 14 at m = 16."""
    if m == 1:
        return [0]
    others = [r for r in range(m - 1) if r % 4 != (m - 1) % 4]
    late = [r for r in others if r >= 12]
    return [(late or others)[(7 * m) % len(late or others)], m - 1]


def active_polytope(rng, traj_p, traj_q, start_p, start_q=None, m=4, tries=64):
    """(h_mat [m x n_s], h_vec [m x 1]) with unit rows in random directions.  The rows of `cutting_rows(m)` cut the
    particles: for each, of `tries` random directions (and the ellipsoids' axes) the one whose best cut (`_cut`) scores
    highest, the second chosen
    so that some particles cross it alone and some the first alone.  Every other row lies beyond all the particles, each
    at its own distance.  start_p [n_s] or [E x n_s], start_q likewise ([n_s x n_s] / [E x n_s x n_s]) or None: the starts
    of E problems lie inside every row."""
    n_s = traj_p.shape[-1]
    P, H = traj_p.shape[:2]
    q = np.zeros((P, H, n_s, n_s)) + traj_q
    start_p = np.asarray(start_p, dtype=np.float64).reshape(-1, n_s)
    start_q = np.zeros((len(start_p), n_s, n_s)) + (0.0 if start_q is None else np.asarray(start_q).reshape(-1, n_s, n_s))

    def unit():
        h = rng.normal(size=n_s)
        return h / np.linalg.norm(h)

    def start_support(h):
        return float(np.max(start_p @ h + np.sqrt(np.einsum('i,eij,j->e', h, start_q, h))))

    h_mat, h_vec = np.empty((m, n_s)), np.empty((m, 1))
    cutting = cutting_rows(m)
    for r in range(m):
        if r in cutting:
            continue
        h = unit()
        s = support(traj_p, q, h)
        top = max(float(np.nanmax(s)), start_support(h))
        h_mat[r], h_vec[r, 0] = h, top + (0.02 + 0.05 * rng.uniform()) * (1.0 + abs(top))
    # besides random directions, the principal axes of the ellipsoids at the last step and directions among the thinner
    # ones: where the ellipsoids grow fast in one direction, random rows all cross the same largest ellipsoids first
    w, V = np.linalg.eigh(np.nanmean(q[:, -1], axis=0))
    thin = V[:, :max(1, n_s - 1)]
    axes = [sgn * V[:, j] for j in range(n_s) for sgn in (1.0, -1.0)]
    crossed = None          # particles crossing the first cutting row at some step
    for r in reversed(cutting):
        best = None
        mixes = [thin @ rng.normal(size=thin.shape[1]) for _ in range(tries // 4)]
        for h in [unit() for _ in range(tries)] + axes + [v / np.linalg.norm(v) for v in mixes]:
            cut = _cut(support(traj_p, q, h), start_support(h), crossed, 0.3 if len(cutting) > 1 else 0.5)
            if cut is not None and (best is None or cut[1] > best[2]):
                best = (h, cut[0], cut[1])
        if best is None:      # (one particle and one step: nothing to cut between; a row beyond it)
            h = unit()
            best = (h, max(float(np.nanmax(support(traj_p, q, h))), start_support(h)) + 0.05, None)
        h_mat[r], h_vec[r, 0] = best[0], best[1]
        crossed = np.nanmax(support(traj_p, q, best[0]), 1) > best[1]
    return h_mat, h_vec


def crossings(traj_p, traj_q, h_mat, h_vec):
    """[P x m]: particle p crosses row r at some step (its safety distance to the row is >= 0)."""
    P, H, n_s = traj_p.shape
    d = reach.lin_ellipsoid_safety_distance(traj_p.reshape(P * H, n_s), traj_q.reshape(P * H, n_s, n_s), h_mat, h_vec)
    return (d.reshape(P, H, -1) >= 0).any(1)


def min_abs_distance(traj_p, traj_q, h_mat, h_vec):
    """The smallest |lin_ellipsoid_safety_distance| over every particle, step and row."""
    P, H, n_s = traj_p.shape
    d = reach.lin_ellipsoid_safety_distance(traj_p.reshape(P * H, n_s), traj_q.reshape(P * H, n_s, n_s), h_mat, h_vec)
    return float(np.nanmin(np.abs(d)))
