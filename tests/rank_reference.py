"""What the ranking tests share (no GPU, no torch): which kernel sx_cem_rank_refit takes for a shape and an output mode, the
elite order each kernel promises, a high-precision refit with the error an f64 kernel may show against it,
and the table of cases tests/test_rank_host.py checks on the CPU and tests/test_gpu_rank_kernels.py runs on the GPU.

A case names the kernel it is there for, the output mode (`via`) in which the launcher takes that kernel, and the structural
properties of its inputs that make it reach the branch it is meant for (`props`, checked by `check_props`)."""
import zlib
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

from oracle import cem as ocem

KERNELS = ('count', 'select4', 'select8', 'select16')
# output modes (rows, refit): rows and refit / rows only (multi-GPU local stage, prologue refit) / refit only (the newer
# solvers) / neither (idx and best only)
MODES = ((True, True), (True, False), (False, True), (False, False))
ROWS_REFIT, ROWS_ONLY, REFIT_ONLY, NEITHER = MODES
SELECT_THREADS = 1024     # cem_rank_kernel: candidates per register slot
U = 2.0 ** -53


def expected_kernel(E, P, rows, refit):
    """The launcher's rule (csrc/sx_rank.hip): counting where sx_cem_rank_counts says so AND the refit, if asked for, has the
    rows to read back; else one workgroup per problem, 4 / 8 / 16 candidates per thread."""
    from safe_exploration_amd import _lib
    if int(_lib.lib().sx_cem_rank_counts(E, P)) != 0 and (rows or not refit):
        return 'count'
    slots = -(-P // SELECT_THREADS)
    return 'select4' if slots <= 4 else 'select8' if slots <= 8 else 'select16'


def expected_order(con, obj, k, kernel):
    """elite_idx of one problem: counting returns rank order, one workgroup the best first and the rest in index order."""
    order = [int(i) for i in ocem.rank(np.asarray(con), np.asarray(obj), k)]
    if kernel == 'count':
        return order
    assert kernel in KERNELS
    return [order[0]] + sorted(order[1:])


def refit_hp(rows):
    """mean and unbiased std over axis 0 in np.longdouble, two passes; std = 0 at k = 1."""
    x = np.asarray(rows, dtype=np.longdouble)
    k = x.shape[0]
    mean = x.sum(axis=0) / k
    if k == 1:
        return mean, np.zeros_like(mean)
    d = x - mean[None]
    return mean, np.sqrt((d * d).sum(axis=0) / (k - 1))


def refit_bounds(rows):
    """(mean bound, std bound), absolute, per column: what an f64 two-pass refit may differ from refit_hp by, whatever its
    summation order.  u = 2^-53.  Mean: a sum of k terms in any order, then one division: delta = k u max|x|.  Std: the sum
    of k squares, the subtraction, the square, the division and the root are (k + 4) u relative, and a mean off by delta adds
    (delta / s)^2 relative (sum (x - m - e)^2 = sum (x - m)^2 + k e^2); where s = 0, delta absolute."""
    x = np.asarray(rows, dtype=np.longdouble)
    k = x.shape[0]
    delta = k * U * np.abs(x).max(axis=0)
    s = refit_hp(rows)[1]
    safe = np.where(s > 0, s, 1)
    return delta, np.where(s > 0, s * ((k + 4) * U + (delta / safe) ** 2), delta)


def sortable_key(x):
    """The kernels' 64-bit key of a double (csrc/sx_rank.hpp): unsigned order == numeric order, -0.0 == +0.0, NaN last."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = (x + 0.0).view(np.uint64)
    key = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    key[np.isnan(x)] = ~np.uint64(0)
    return key


def differing_bytes(keys, ref):
    """Byte positions (0 = lowest) in which any of `keys` differs from `ref`: the kernel's hdiff."""
    dif = int(np.bitwise_or.reduce(keys ^ ref)) if len(keys) else 0
    return {b for b in range(8) if (dif >> (8 * b)) & 255}


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    E: int
    P: int
    k: int
    L: int
    kernel: str                 # the kernel the case is there for ...
    via: tuple                  # ... and the output mode (rows, refit) in which the launcher takes it
    make: Callable              # rng -> (con [E x P], obj [E x P], act [E x P x L])
    props: dict = field(default_factory=dict)
    same_order: bool = False    # count order == select order (all keys tied, ...): the kernel's identity is not observable
    plain: bool = False         # standard-normal actions: the project's rtol 1e-12 / atol 1e-14 against oracle.cem.refit too
    strided: bool = False       # candidate-row layout: cost_stride = act_stride = 2 + L, views into one buffer
    seed: str = ''              # cases that share their inputs name the same seed (default: the case's name)

    def data(self):
        con, obj, act = self.make(np.random.default_rng(zlib.crc32((self.seed or self.name).encode())))
        con, obj, act = (np.ascontiguousarray(a, dtype=np.float64) for a in (con, obj, act))
        assert con.shape == obj.shape == (self.E, self.P) and act.shape == (self.E, self.P, self.L), self.name
        return con, obj, act


def generic(E, P, L):
    """Problem 0: few constraint costs, many objective ties.  Problem 1: every key equal.  Problem 2: nothing feasible."""
    def make(rng):
        con = rng.choice([0., 0., 3., 10., 13., 20.], size=(E, P))
        obj = rng.integers(0, max(2, P // 6), size=(E, P)).astype(np.float64) / 8 - 1
        if E > 1:
            con[1], obj[1] = 3.0, 0.25
        if E > 2:
            con[2] = rng.choice([3., 10.], size=P)
        return con, obj, rng.normal(size=(E, P, L))
    return make


def tie_cut(con, obj, kmax):
    """A k <= kmax whose cut falls inside a run of equal keys (k-th and (k + 1)-th tied), nearest to kmax / 3; None if none."""
    order = ocem.rank(con, obj, len(con))
    kc, ko = sortable_key(con)[order], sortable_key(obj)[order]
    tied = np.nonzero((kc[1:] == kc[:-1]) & (ko[1:] == ko[:-1]))[0] + 1      # k with key[k - 1] == key[k]
    tied = tied[tied <= kmax]
    return int(tied[np.argmin(np.abs(tied - max(1, kmax // 3)))]) if len(tied) else None


def width_cases():
    """Template widths and ragged edges of the one-workgroup kernel (refit-only mode forces it at any shape)."""
    out = []
    for P in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 16384):
        kernel = 'select4' if P <= 4096 else 'select8' if P <= 8192 else 'select16'
        for E in (1, 3):
            base = Case(f'width_P{P}_E{E}', E, P, 1, 3, kernel, REFIT_ONLY, generic(E, P, 3), plain=True)
            con, obj, _ = base.data()
            kmax = min(P, 2048)
            kt = tie_cut(con[0], obj[0], min(kmax, P - 1))
            for k in sorted({1, min(2, P), kmax} | ({kt} if kt else set())):
                props = {'cut_in_tie': True} if k == kt else {}
                out.append(Case(f'{base.name}_k{k}', E, P, k, 3, kernel, REFIT_ONLY, base.make, props, plain=True,
                                seed=base.name))        # (the inputs `tie_cut` saw)
    return out


def boundary_indices(P):
    """Index groups that straddle the one-workgroup kernel's wave (64) and slot (1024) boundaries, and the ragged end."""
    groups = [range(60, 68), range(1020, 1030), range(P - 5, P), range(126, 130), range(190, 195), range(1086, 1090)]
    if P > 4100:
        groups[4:] = [range(4094, 4099), range(2046, 2051)]
    return [np.array(g) for g in groups]


def con_structure_cases():
    out = []
    three, up = 3.0, np.nextafter(3.0, 4.0)
    ulps = [np.float64(three)]
    for _ in range(6):
        ulps.append(np.nextafter(ulps[-1], 4.0))

    def ladder(values, P):
        """The last value everywhere, the others in small groups at the boundary indices: the k-th key has the last value."""
        def make(rng):
            con = np.full((1, P), values[-1])
            for v, idx in zip(values[:-1], boundary_indices(P)):
                con[0, idx] = v
            return con, rng.normal(size=(1, P)).round(1), rng.normal(size=(1, P, 4))
        return make

    def drawn(values, P, p=None):
        def make(rng):
            con = rng.choice(values, size=(1, P), p=p)
            return con, rng.normal(size=(1, P)).round(1), rng.normal(size=(1, P, 4))
        return make

    def nan_but_three(P):
        def make(rng):
            con = np.full((1, P), np.nan)
            con[0, [63, 64, P - 1]] = [3.0, 0.0, 10.0]
            return con, rng.normal(size=(1, P)).round(1), rng.normal(size=(1, P, 4))
        return make

    for P, kernel in ((1500, 'select4'), (5000, 'select8')):
        k = P // 7
        mk = lambda tag, kk, make, props, **kw: out.append(Case(f'con_{tag}_P{P}', 1, P, kk, 4, kernel, REFIT_ONLY, make, props,
                                                                 plain=True, **kw))
        mk('one_value', k, drawn([3.0], P), {'con_distinct': 1, 'con_bytes': set()})
        mk('five_values_kth_in_5th', k, ladder([0., 3., 10., 13., 20.], P), {'con_distinct': 5, 'kth_in_distinct': 5})
        mk('six_values_kth_in_6th', k, ladder([0., 3., 10., 13., 20., 23.], P),
           {'con_distinct': 6, 'kth_in_distinct': 6, 'con_bytes': {7, 6}})
        mk('forty_integers', k, drawn(10.0 * np.arange(40), P), {'con_distinct': 40, 'con_bytes': {7, 6, 5}})
        mk('arbitrary_doubles', k, lambda rng, P=P: (rng.normal(size=(1, P)) * 10.0 ** rng.integers(-30, 30, size=(1, P)),
                                                     rng.normal(size=(1, P)), rng.normal(size=(1, P, 4))),
           {'con_bytes': set(range(8))})
        mk('low_byte_two_values', k, drawn([three, up], P, p=[0.05, 0.95]),
           {'con_distinct': 2, 'kth_in_distinct': 2, 'con_bytes': {0}})
        mk('low_byte_seven_values', k, ladder(ulps, P), {'con_distinct': 7, 'kth_in_distinct': 7, 'con_bytes': {0}})
        mk('nan_but_three', k, nan_but_three(P), {'con_distinct': 4, 'kth_in_distinct': 4})
        mk('all_nan', k, drawn([np.nan], P), {'con_distinct': 1, 'best_con': 'nan'})
        mk('infinities', k, drawn([-np.inf, 0.0, 3.0, np.inf, np.nan], P), {'con_distinct': 5})
    return out


def obj_structure_cases():
    out = []
    x, xu = 1.5, np.nextafter(1.5, 2.0)
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, -1e-310, 1.0, -1.0]

    def one_con(obj_of):
        def make(rng):
            obj = np.ascontiguousarray(obj_of(rng), dtype=np.float64)[None]
            return np.zeros_like(obj), obj, rng.normal(size=obj.shape + (4,))
        return make

    def top_bin(P, k):
        """k objectives in [1, 2) (one top byte of the key), the others >= 1024: the first radix pass selects the whole bin.
        The smallest of the k sits at a late index."""
        def obj_of(rng):
            obj = 1024.0 + rng.uniform(0, 1e6, size=P)
            idx = np.sort(rng.choice(P, size=k, replace=False))
            obj[idx] = rng.uniform(1.0, 2.0, size=k)
            obj[idx[-3]] = 1.0
            return obj
        return obj_of

    for P, kernel in ((1500, 'select4'), (5000, 'select8')):
        # x and its upper neighbour interleaved: halves at P = 1500; at P = 5000 x is every 4th, so that a cut inside the
        # upper value stays within the 2048 elites the kernels take
        every = 2 if P // 2 + P // 4 <= 2048 else 4
        inter = lambda rng, P=P, every=every: np.where(np.arange(P) % every == 0, x, xu)
        mk = lambda tag, kk, obj_of, props, **kw: out.append(Case(f'obj_{tag}_P{P}', 1, P, kk, 4, kernel, REFIT_ONLY,
                                                                   one_con(obj_of), dict(props, con_distinct=1), plain=True, **kw))
        mk('all_equal', P // 7, lambda rng, P=P: np.full(P, 1.25), {'obj_bytes': set(), 'cut_in_tie': True}, same_order=True)
        # (index order is rank order inside either half: the cut in the lower half is the all-equal case again)
        mk('neighbours_cut_in_lower_half', P // (2 * every), inter, {'obj_bytes': {0}, 'cut_in_tie': True, 'obj_low_byte_cut': True},
           same_order=True)
        mk('neighbours_cut_in_upper_half', P // every + P // 8, inter, {'obj_bytes': {0}, 'cut_in_tie': True, 'obj_low_byte_cut': True})
        mk('top_byte_bin', P // 5, top_bin(P, P // 5), {'best_in_ties': True})
        mk('specials', P // 3, lambda rng, P=P: rng.choice(specials, size=P), {})
    return out


def row_width_cases():
    """k either side of the rows the refit's first gather covers (8 row groups of threads / min(L, 256) rows each); L at the
    column_totals branch edge (16 L <= threads), the 256-column chunk edge, a last chunk of one column, 2 + L around 32."""
    def make_of(L):
        def make(rng):
            con, obj, act = generic(1, 600, L)(rng)
            con[0, [500, 400, 300]], obj[0, [500, 400, 300]] = 0.0, [-9.0, -8.0, -7.0]   # the best three, in falling index order
            return con, obj, act
        return make
    out = []
    for kernel, via, Ls in (('select4', REFIT_ONLY, (1, 16, 64, 65, 256, 257, 300, 513)),
                            ('count', ROWS_REFIT, (1, 30, 31, 32, 33, 256, 257, 513))):
        for L in Ls:
            for k in (3, 40, 600):
                out.append(Case(f'rows_{kernel}_L{L}_k{k}', 1, 600, k, L, kernel, via, make_of(L), plain=True))
    return out


def refit_cases():
    out = []

    def scaled(f):
        def make(rng):
            con, obj, act = generic(1, 600, 7)(rng)
            return con, obj, f(act)
        return make
    for tag, f in (('offset_1e8', lambda a: 1e8 + a), ('scale_1e-150', lambda a: a * 1e-150)):
        for k in (1, 2, 40):
            out.append(Case(f'refit_{tag}_k{k}', 1, 600, k, 7, 'select4', REFIT_ONLY, scaled(f)))
    return out


def best_ok_cases():
    def best_at(value):
        def make(rng):
            con, obj, act = generic(1, 100, 3)(rng)
            con[0] = np.where(con[0] == 0, 3.0, con[0])
            con[0, 37] = value
            return con, obj, act
        return make
    out = [Case(f'best_{tag}', 1, 100, 9, 3, 'select4', REFIT_ONLY, best_at(v), {'best_con': tag, 'best_ok': ok}, plain=True)
           for tag, v, ok in (('negzero', -0.0, 1), ('negative', -1.0, 0), ('denormal', 5e-324, 0))]
    out.append(Case('best_all_nan', 1, 100, 9, 3, 'select4', REFIT_ONLY,
                    lambda rng: (np.full((1, 100), np.nan), np.full((1, 100), np.nan), rng.normal(size=(1, 100, 3))),
                    {'best_con': 'nan', 'best_ok': 0}, plain=True, same_order=True))
    return out


SPLIT_TENTH = np.float64(np.array([0x3FB9999900000000], dtype=np.uint64).view(np.float64)[0])   # 0.1 with a zero low half


def counting_cases():
    out = []
    for P in (1, 15, 16, 17, 127, 128, 129, 1024, 4097):
        out.append(Case(f'count_P{P}', 1, P, max(1, min(P, 2048) // 3), 5, 'count', ROWS_REFIT, generic(1, P, 5), plain=True))

    def equal_tile(P, tile):
        def make(rng):
            con, obj, act = generic(1, P, 5)(rng)
            con[0, 16 * tile:16 * tile + 16], obj[0, 16 * tile:16 * tile + 16] = 0.0, -5.0     # the 16 best, ties by index
            return con, obj, act
        return make
    for tag, tile in (('first', 0), ('middle', 6), ('last', 12)):      # 200 candidates: tile 12 has 8
        out.append(Case(f'count_equal_tile_{tag}', 1, 200, 150, 5, 'count', ROWS_REFIT, equal_tile(200, tile),
                        {'equal_tile': tile}, plain=True))

    def one_wide(P, at, wide, beside):
        """Small integers (zero low half of the key: 96-bit compares) but ONE constraint cost whose key has a non-zero low
        half (it is the larger), and neighbours that differ from it in that half only.  Its objective is the smallest, the
        neighbours' the largest: a compare that drops the low half orders them by objective, i.e. wrongly."""
        def make(rng):
            con, obj, act = generic(1, P, 5)(rng)
            near = [(at + d) % P for d in (-16 * 9, -1, 1, 16 * 9)]
            con[0, near], obj[0, near] = beside, 50.0
            con[0, at], obj[0, at] = wide, -50.0
            return con, obj, act
        return make
    for P in (256, 1024):
        for where, at in (('first_eighth', 5), ('last_eighth', P - 3), ('middle', P // 2 + 1)):
            out.append(Case(f'count_wide_tenth_{where}_P{P}', 1, P, P, 5, 'count', ROWS_REFIT,
                            one_wide(P, at, 0.1, SPLIT_TENTH), {'wide_at': at}, plain=True))
            out.append(Case(f'count_wide_ulp_{where}_P{P}', 1, P, P, 5, 'count', ROWS_REFIT,
                            one_wide(P, at, np.nextafter(3.0, 4.0), 3.0), {'wide_at': at}, plain=True))
    # the grid limit: 768 workgroups count, 784 do not
    out.append(Case('count_grid_E48_P256', 48, 256, 20, 3, 'count', ROWS_REFIT, generic(48, 256, 3), plain=True))
    out.append(Case('count_grid_E64_P192', 64, 192, 20, 3, 'count', ROWS_REFIT, generic(64, 192, 3), plain=True))
    out.append(Case('count_grid_E49_P256', 49, 256, 20, 3, 'select4', ROWS_REFIT, generic(49, 256, 3), plain=True))
    return out


def layout_cases():
    """Candidate rows [con, obj, actions...] in one buffer, as after the multi-GPU exchange (num_candidates = C k)."""
    return [Case('layout_E3_select4', 3, 4 * 50, 50, 6, 'select4', REFIT_ONLY, generic(3, 200, 6), plain=True, strided=True),
            Case('layout_E70_select4', 70, 96, 12, 6, 'select4', ROWS_REFIT, generic(70, 96, 6), plain=True, strided=True),
            Case('layout_E2_count', 2, 4 * 50, 50, 6, 'count', ROWS_REFIT, generic(2, 200, 6), plain=True, strided=True)]


def build_cases():
    cases = (width_cases() + con_structure_cases() + obj_structure_cases() + row_width_cases() + refit_cases()
             + best_ok_cases() + counting_cases() + layout_cases())
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = build_cases()


def check_props(case, con, obj):
    """Asserts the structural properties the case claims (problem 0), from the kernels' keys."""
    k, P = case.k, case.P
    kc, ko = sortable_key(con[0]), sortable_key(obj[0])
    order = ocem.rank(con[0], obj[0], P)
    best, kth = order[0], order[k - 1]
    distinct = np.unique(kc)
    for name, want in case.props.items():
        if name == 'con_distinct':
            assert len(distinct) == want, (case.name, name, len(distinct))
        elif name == 'kth_in_distinct':
            assert int(np.searchsorted(distinct, kc[kth])) + 1 == want, (case.name, name)
        elif name == 'con_bytes':
            assert differing_bytes(kc, kc[best]) == want, (case.name, name, differing_bytes(kc, kc[best]))
        elif name == 'obj_bytes':
            assert differing_bytes(ko, ko[best]) == want, (case.name, name, differing_bytes(ko, ko[best]))
        elif name == 'cut_in_tie':
            assert k < P and kc[kth] == kc[order[k]] and ko[kth] == ko[order[k]], (case.name, name)
        elif name == 'obj_low_byte_cut':
            # the objective keys either side of the k-th key's run differ from it in their lowest byte only
            vals = np.unique(ko[kc == kc[kth]])
            j = int(np.searchsorted(vals, ko[kth]))
            near = [vals[i] for i in (j - 1, j + 1) if 0 <= i < len(vals)]
            assert near and all(0 < int(v ^ ko[kth]) < 256 for v in near), (case.name, name)
        elif name == 'best_in_ties':
            # the first objective pass ends the select: the k-th key's top-byte bin holds exactly the elites that are left,
            # the best is one of them and not the first of them by index
            same_con = kc == kc[kth]
            ties = np.nonzero(same_con & (ko >> np.uint64(56) == ko[kth] >> np.uint64(56)))[0]
            less = np.count_nonzero((kc < kc[kth]) | (same_con & (ko >> np.uint64(56) < ko[kth] >> np.uint64(56))))
            assert less + len(ties) == k and best in ties and best != ties.min(), (case.name, name)
        elif name == 'best_con':
            v = con[0][best]
            ok = {'negzero': v == 0 and np.signbit(v), 'negative': v < 0, 'denormal': 0 < v < 2.3e-308, 'nan': np.isnan(v)}
            assert ok[want], (case.name, name, v)
        elif name == 'best_ok':
            assert int(con[0][best] == 0) == want, (case.name, name)
        elif name == 'equal_tile':
            t = slice(16 * want, min(16 * want + 16, P))
            assert len(np.unique(kc[t])) == 1 and len(np.unique(ko[t])) == 1 and set(range(P)[t]) <= set(order[:k].tolist())
        elif name == 'wide_at':
            low = kc & np.uint64(0xffffffff)
            assert np.nonzero(low)[0].tolist() == [want], (case.name, name)
            beside = np.nonzero((kc >> np.uint64(32) == kc[want] >> np.uint64(32)) & (low == 0))[0]
            assert len(beside) >= 3, (case.name, name)
            # ranked by the full key every neighbour is in front of the wide value; by the high half and the objective it
            # would be behind it
            pos = {int(i): r for r, i in enumerate(order)}
            assert all(pos[int(b)] < pos[want] and ko[b] > ko[want] for b in beside), (case.name, name)
        else:
            raise AssertionError(f'{case.name}: unknown property {name}')
