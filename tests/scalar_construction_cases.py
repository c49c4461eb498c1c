"""The models of the scalar construction tests: each case builds the same problem twice from an all-unassigned start -- as an oracle
Model and as a GpuScoreDirector -- so that the CPU mirror tests and the GPU parity tests construct exactly the same inputs."""
import numpy as np


class Case:
    def __init__(self, name, n, n_values, oracle, gpu, value_lists=None):
        self.name, self.n, self.n_values, self.value_lists = name, n, n_values, value_lists
        self._oracle, self._gpu = oracle, gpu

    def oracle(self, sfo, start=None):
        """A fresh oracle model; start = the values to begin from (default: all unassigned)."""
        o = self._oracle(sfo, np.full(self.n, -1, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64))
        if self.value_lists is not None:
            o.set_value_lists(self.value_lists)
        return o

    def gpu(self, n_replicas=1, allows_unassigned=True):
        d = self._gpu(np.full(self.n, -1, dtype=np.int64), n_replicas, allows_unassigned)
        if self.value_lists is not None:
            d.set_value_lists(0, 0, self.value_lists)
        return d


def _clique(n):
    off = np.arange(n + 1, dtype=np.uint32) * np.uint32(n - 1)
    adj = np.asarray([v for u in range(n) for v in range(n) if v != u], dtype=np.uint32)
    return off, adj


def _graph_case(name, g, value_lists=None, pair_ir=False):
    import solverforge_amd as sfa
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, PairOp, SelectorKind

    def gpu(start, R, nullable):
        if nullable and not pair_ir:
            return sfa.build_graph_coloring(dict(g, colors=start), n_replicas=R)
        d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=R)  # build_graph_coloring with a required variable / an interpreted join
        d.add_entity_class(0, g["n"])
        d.add_scalar_variable(0, 0, g["n_colors"], nullable, start)
        d.add_fact_csr(1, g["adj_off"], g["adj"])
        d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
        if pair_ir:
            d.add_pair_join(0, [(PairOp.CSR_CONTAINS, 0, 1), (PairOp.VALUE_EQ, 1)], level=0, weight=1)
        else:
            d.add_constraint(ConstraintKind.CROSS_ADJACENT_EQUAL, 0, fact=1, level=0, weight=1)
        d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
        d.add_selector(SelectorKind.SCALAR_SWAP, 0)
        return d

    return Case(name, g["n"], g["n_colors"], lambda sfo, start: sfo.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], start), gpu, value_lists)


def graph(n, e, k, seed, value_lists=None, pair_ir=False):
    from solverforge_amd import datasets

    return _graph_case(f"graph{n}x{e}x{k}", datasets.make_graph(n, e, k, seed=seed), value_lists, pair_ir)


def clique(n, k):
    off, adj = _clique(n)
    return _graph_case(f"clique{n}x{k}", {"n": n, "n_colors": k, "adj_off": off, "adj": adj})


def four_join_graph(n, e, k, seed):
    """Graph colouring with its one join split into FOUR disjoint joins (the pairs {u, v} by (u + v) % 4) on the oracle's level and weight:
    a four-join class whose score equals the oracle's single join in every state (the construction of test_gpu_multi_join.py's split)."""
    from solverforge_amd import datasets
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, PairOp, SelectorKind

    g = datasets.make_graph(n, e, k, seed=seed)

    def part(q):
        rows = [[int(v) for v in g["adj"][g["adj_off"][u]:g["adj_off"][u + 1]] if (u + int(v)) % 4 == q] for u in range(n)]
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(r) for r in rows])
        return off, np.asarray([v for r in rows for v in r], dtype=np.uint32)

    def gpu(start, R, nullable):
        d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=R)
        d.add_entity_class(0, n)
        d.add_scalar_variable(0, 0, k, nullable, start)
        d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
        for q in range(4):
            off, adj = part(q)
            d.add_fact_csr(20 + q, off, adj)
            if q == 0:  # one preset among three programs
                d.add_constraint(ConstraintKind.CROSS_ADJACENT_EQUAL, 0, fact=20, level=0, weight=1)
            else:
                d.add_pair_join(0, [(PairOp.CSR_CONTAINS, 0, 20 + q), (PairOp.VALUE_EQ, 1)], level=0, weight=1)
        d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
        d.add_selector(SelectorKind.SCALAR_SWAP, 0)
        return d

    return Case(f"fourjoin{n}", n, k, lambda sfo, start: sfo.Model.graph_coloring(k, g["adj_off"], g["adj"], start), gpu)


def nqueens(n):
    import solverforge_amd as sfa

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_nqueens(start, n_replicas=R)

    return Case(f"queens{n}", n, n, lambda sfo, start: sfo.Model.nqueens(start), gpu)


def shift_schedule(n_nurses=4, n_days=14, per_day=2, presence=None):
    """28 shifts, 4 nurses: the runs table; presence = (lo, hi, cap): its indexed-presence variant."""
    import solverforge_amd as sfa

    day = np.repeat(np.arange(n_days), per_day).astype(np.int64)
    kw = dict(limit=2, w_streak=3, count_weight=1) if presence is None else dict(w_streak=3, count_weight=1, presence=presence)

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_shift_schedule(start, day, n_nurses, n_replicas=R, **kw)

    return Case("shifts" if presence is None else "presence", len(day), n_nurses, lambda sfo, start: sfo.Model.shift_schedule(start, day, n_nurses, **kw), gpu)


def balance(n=30, n_bins=6, cap=-3, seed=5):
    """Self-join + grouped + (cap -3) the f64 balance step."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    sizes = (datasets.stream(seed, n) % np.uint64(9)).astype(np.int64) + 1

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_balance(start, sizes, n_bins, n_replicas=R, cap=cap)

    return Case(f"balance{cap}", n, n_bins, lambda sfo, start: sfo.Model.balance(n_bins, start, sizes, cap=cap), gpu)


def assignment(n=30, n_values=7, seed=11, value_lists=None):
    """Value cost (a random matrix with zeros and ties) + exists."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    cost = (datasets.stream(seed, n * n_values) % np.uint64(6)).astype(np.int64).reshape(n, n_values)
    row_w = (datasets.stream(seed + 1, n_values) % np.uint64(4)).astype(np.int64) + 1

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_assignment(start, cost, n_values, n_replicas=R, row_w=row_w)

    return Case("assignment", n, n_values, lambda sfo, start: sfo.Model.assignment(start, cost, n_values, row_w=row_w), gpu, value_lists)


def retry_assignment(n=12, n_values=4):
    """A live-refresh case whose kept entities ARE assigned on a retry: opening a value row costs one hard (exists, row weight 1) -- a tie with
    the unassigned penalty it removes -- and every cost is positive except two rewards, so an entity keeps current until an entity with a
    reward has opened a row; the assignment reopens the kept entities and the open row takes them."""
    import solverforge_amd as sfa

    cost = np.full((n, n_values), 2, dtype=np.int64)
    cost[7, 1], cost[9, 3] = -1, -2
    cost[3, :] = [1, 4, 1, 5]
    row_w = np.ones(n_values, dtype=np.int64)

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_assignment(start, cost, n_values, n_replicas=R, row_w=row_w, ex_level=0)

    return Case("retry", n, n_values, lambda sfo, start: sfo.Model.assignment(start, cost, n_values, row_w=row_w, ex_level=0), gpu)


def long_retry_assignment(n=150, opener=120):
    """retry_assignment with a kept list longer than one 64-lane chunk: entities 0 .. opener-1 keep current (a row costs what the unassigned
    penalty gives back, every cost is positive) until entity `opener`, the one with a reward, opens row 1.  Every third entity has no
    value 1 in its list and keeps on keeping, so the assignments that follow leave the kept list from its MIDDLE, one per restart."""
    import solverforge_amd as sfa

    n_values = 4
    cost = np.full((n, n_values), 2, dtype=np.int64)
    cost[opener, 1] = -1
    row_w = np.ones(n_values, dtype=np.int64)
    lists = [[0, 2, 3] if e % 3 == 1 else [0, 1, 2, 3] for e in range(n)]

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_assignment(start, cost, n_values, n_replicas=R, row_w=row_w, ex_level=0)

    return Case("longretry", n, n_values, lambda sfo, start: sfo.Model.assignment(start, cost, n_values, row_w=row_w, ex_level=0), gpu, lists)


class BruteTimetable:
    """The four-join timetable of tests/test_gpu_multi_join.py (three hard COL_EQ && VALUE_EQ conflicts, one soft COL_LT && |dv| <= 1 join of
    weight 3) as a brute-force count over all pairs, behind the oracle Model's primitives (the oracle has no timetable model)."""

    def __init__(self, cols, start):
        self.cols, self.vals = cols, np.asarray(start, dtype=np.int64).copy()

    def _score_of(self, v):
        on = v >= 0
        pair = np.triu(on[:, None] & on[None, :], 1)
        eq = pair & (v[:, None] == v[None, :])
        hard = -int((~on).sum()) - sum(int((eq & (c[:, None] == c[None, :])).sum()) for c in self.cols[:3])
        c = self.cols[3]
        soft = -3 * int((pair & (c[:, None] < c[None, :]) & (np.abs(v[:, None] - v[None, :]) <= 1)).sum())
        return np.asarray([hard, soft, 0, 0], dtype=np.int64)

    def get_vars(self, desc=0, var=0):
        return self.vals.copy()

    def score(self):
        return self._score_of(self.vals)

    fresh_score = score

    def evaluate_moves(self, records):
        sc = np.zeros((len(records), 4), dtype=np.int64)
        do = np.zeros(len(records), dtype=np.int32)
        for i, (_, e, _, _, _, v) in enumerate(records):
            do[i] = self.vals[e] != v
            t = self.vals.copy()
            t[e] = v
            sc[i] = self._score_of(t)
        return sc, do

    def apply_move(self, record):
        self.vals[record[1]] = record[5]


def timetable(n=64, k=8, seed=11):
    from solverforge_amd import datasets
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, PairOp as P, SelectorKind

    r = datasets.stream(seed, 5 * n)
    cols = [(r[(q + 1) * n:(q + 2) * n] % np.uint64(m)).astype(np.int32) for q, m in enumerate((9, 7, 6, 40))]  # teacher, group, room, a soft key
    progs = [([(P.COL_EQ, 0, 50 + q, -1, 0), (P.VALUE_EQ, 1, -1, -1, 0)], 0, 1) for q in range(3)]
    progs.append(([(P.COL_LT, 0, 53, -1, 0), (P.VALUE_ABSDIFF_LE, 1, -1, -1, 1)], 1, 3))

    def gpu(start, R, nullable):
        d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=R)
        d.add_entity_class(0, n)
        d.add_scalar_variable(0, 0, k, nullable, start)
        for q, c in enumerate(cols):
            d.add_fact_column_i32(50 + q, c)
        d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
        for prog, level, weight in progs:
            d.add_pair_join(0, prog, level=level, weight=weight)
        d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
        d.add_selector(SelectorKind.SCALAR_SWAP, 0)
        return d

    return Case("timetable", n, k, lambda sfo, start: BruteTimetable(cols, start), gpu)


RETRY_ENTITY_KEYS = [0, 1, 2] * 4


def retry_value_keys(heuristic):
    """Value keys under which the heuristic's forager reaches value 1, the row a reward opens: the weakest-fit heuristics (2, 3) need it
    weakest, the others take it as the first of the two strongest."""
    return [3, 0, 1, 3] if heuristic in (2, 3) else [0, 3, 1, 3]


def jobshop(n_jobs=6, n_machines=4):
    """The scalar class of a mixed model: operations choose a machine, the machine sequences (the list class) stay empty."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    p = datasets.make_jobshop(n_jobs, n_machines)

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_jobshop(dict(p, machine_idx=start), n_replicas=R)

    return Case("jobshop", p["n_ops"], n_machines, lambda sfo, start: sfo.Model.jobshop(p["job"], start, p["sequences"]), gpu)


# what the oracle's own construct_first_fit gives on the issue's inputs: (case, unassigned after, trials, values or None)
def first_fit_inputs():
    return [
        (graph(120, 700, 3, 1), 46, 279, None),
        (clique(70, 80), 0, 2485, list(range(70))),          # first-fit hits in the second 64-lane chunk
        (clique(130, 140), 0, 8515, list(range(130))),       # 16-bit values, third chunk
        (clique(66, 64), 2, 2208, list(range(64)) + [-1, -1]),  # exactly one full chunk without a hit
        (nqueens(8), 3, 39, [0, 2, 4, 1, 3, -1, -1, -1]),
    ]


def other_first_fit_cases():
    return [shift_schedule(), shift_schedule(presence=(2, 9, 3)), balance(), assignment(), jobshop(), four_join_graph(60, 260, 4, 2)]


def ragged_lists(n, n_values, seed=3):
    """Per-entity value lists: ragged, one empty, one of a single value, the rest a seeded subset in a seeded order."""
    from solverforge_amd import datasets

    r = datasets.stream(seed, n * n_values).reshape(n, n_values)
    lists = []
    for e in range(n):
        keep = [v for v in np.argsort(r[e], kind="stable").tolist() if int(r[e][v]) % 3 != 0]
        lists.append(keep)
    lists[2] = []
    lists[5] = [n_values - 1]
    return lists


def keys(n, mod, seed):
    """Order keys with ties."""
    from solverforge_amd import datasets

    return (datasets.stream(seed, n) % np.uint64(mod)).astype(np.int64)


# ---- placements wider than one 64-lane chunk ----------------------------------------------------------------------------------------------
WIDE = 130                                   # two full chunks and a tail of two
BEST_FIT_ORDINALS = [0, 63, 64, 65, 127, 128, 129]
BEST_FIT_VALUES = BEST_FIT_ORDINALS + [10, 70, 0]  # what CheapestInsertion gives entities 0..9 of best_fit_assignment(ex_level=-1)


def best_fit_assignment(ex_level=-1, n=24):
    """A cost matrix whose best entry sits at a chosen ordinal of a 130-value placement: every cost is in 5..8 (seeded, so the other entities
    tie inside and across chunks), entity e < 7 has its only cost 1 at BEST_FIT_ORDINALS[e], entity 7 has cost 1 at ordinals 10 AND 70 (the
    first wins), entity 8 has cost 2 at 10 and cost 1 at 70 (the later, better one wins), entity 9 has all costs equal (ordinal 0 wins).
    ex_level=-1: no exists node (no per-value tables); ex_level=0: opening a row costs one hard, as in retry_assignment -- every cost is
    positive, so under PreserveUnassigned the baseline beats every one of the 130 trials."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    cost = (datasets.stream(41, n * WIDE) % np.uint64(4)).astype(np.int64).reshape(n, WIDE) + 5
    for e, k in enumerate(BEST_FIT_ORDINALS):
        cost[e, k] = 1
    cost[7, 10] = cost[7, 70] = 1
    cost[8, 10], cost[8, 70] = 2, 1
    cost[9, :] = 6
    row_w = np.ones(WIDE, dtype=np.int64)

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_assignment(start, cost, WIDE, n_replicas=R, row_w=row_w, ex_level=ex_level)

    return Case(f"bestfit{ex_level}", n, WIDE, lambda sfo, start: sfo.Model.assignment(start, cost, WIDE, row_w=row_w, ex_level=ex_level), gpu)


INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def strength_keys(weakest):
    """name -> (value keys of a 130-value range, value_candidate_limit, the ordinal every placement must take) for the weakest-fit
    (weakest=True: the extreme is the least key) or the strongest-fit heuristics.  The sentinel rows make every key equal to what the
    kernel puts on the invalid lanes of a ragged last chunk."""
    ext, sentinel = (-7, INT64_MAX) if weakest else (7, INT64_MIN)
    base = (np.arange(WIDE, dtype=np.int64) * 5) % 3  # 0..2, with ties everywhere

    def at(*ordinals):
        k = base.copy()
        k[list(ordinals)] = ext
        return k

    return {
        "at64": (at(64), 0, 64), "at127": (at(127), 0, 127), "at129": (at(129), 0, 129),
        "twice_in_two_chunks": (at(70, 128), 0, 70), "twice_from_lane63": (at(63, 64), 0, 63),
        "all_equal": (np.full(WIDE, 4, dtype=np.int64), 0, 0),
        "sentinel65": (np.full(WIDE, sentinel, dtype=np.int64), 65, 0), "sentinel130": (np.full(WIDE, sentinel, dtype=np.int64), 0, 0),
    }


WIDE_STRONGEST, WIDE_WEAKEST = 77, 33   # the values that carry the only greatest / the only least key of wide_list_keys()
WIDE_LENGTHS = [1, 63, 64, 65, 128, 129, 130]
# entity -> (list length, ordinal of WIDE_STRONGEST, ordinal of WIDE_WEAKEST): lane 0 and lane 63 of the later chunks, and the last ordinals
WIDE_PLACED = {0: (130, 64, 127), 1: (130, 127, 64), 2: (129, 128, 0), 3: (128, 5, 127), 4: (65, 64, 3), 5: (64, 63, 0), 6: (63, 62, 1),
               7: (130, 129, 128), 8: (130, 0, 129)}


def wide_list_keys():
    """Value keys with ties and one greatest (WIDE_STRONGEST) and one least (WIDE_WEAKEST) value."""
    from solverforge_amd import datasets

    k = (datasets.stream(43, WIDE) % np.uint64(9)).astype(np.int64)
    k[WIDE_STRONGEST], k[WIDE_WEAKEST] = 100, -100
    return k


def wide_lists(n, seed=47):
    """Per-entity value lists of the lengths 1, 63, 64, 65, 128, 129 and 130 in a seeded order, each a seeded arrangement of distinct values of
    the 130-value range; the entities of WIDE_PLACED carry the two extreme values of wide_list_keys() at the ordinals named there."""
    from solverforge_amd import datasets

    r = datasets.stream(seed, n * WIDE).reshape(n, WIDE)
    pick = datasets.stream(seed + 1, n)
    lists = []
    for e in range(n):
        full = np.argsort(r[e], kind="stable").tolist()
        if e in WIDE_PLACED:
            length, at_strong, at_weak = WIDE_PLACED[e]
            rest = [v for v in full if v not in (WIDE_STRONGEST, WIDE_WEAKEST)][:length - 2]
            lst = [None] * length
            lst[at_strong], lst[at_weak] = WIDE_STRONGEST, WIDE_WEAKEST
            it = iter(rest)
            lst = [next(it) if v is None else v for v in lst]
        else:
            lst = full[:WIDE_LENGTHS[int(pick[e] % np.uint64(len(WIDE_LENGTHS)))]]
        lists.append([int(v) for v in lst])
    return lists


def wide_assignment(n=24, value_lists=None):
    """assignment() at 130 rows: the cost join and the exists node (the per-value tables hold 130 values)."""
    return assignment(n=n, n_values=WIDE, seed=53, value_lists=value_lists)


def wide_clique(n, value_lists=None):
    """A clique with 130 colours: the first-fit forager of entity i has to pass the i colours that are taken."""
    off, adj = _clique(n)
    return _graph_case(f"clique{n}x{WIDE}", {"n": n, "n_colors": WIDE, "adj_off": off, "adj": adj}, value_lists)


# entity -> the ordinal at which its first strictly-improving candidate must fall
ROTATED_HITS_70 = {63: 63, 66: 64, 69: 63, 68: 64}
ROTATED_HITS_130 = {90: 63, 100: 64, 129: 127, 127: 127, 128: 64}


def rotated_clique(n, k, hits, seed=59):
    """A clique of n with k >= n colours whose value lists are rotations of the range: entity e's list starts at colour s_e <= e, the colours
    s_e .. e - 1 are taken by the entities before it (entity i takes colour i), so its first strictly-improving candidate is colour e at
    ordinal e - s_e.  `hits` fixes that ordinal for the named entities, the others get a seeded one."""
    from solverforge_amd import datasets

    r = datasets.stream(seed, n)
    lists = []
    for e in range(n):
        s = e - hits[e] if e in hits else int(r[e] % np.uint64(e + 1))
        lists.append([(s + j) % k for j in range(k)])
    off, adj = _clique(n)
    return _graph_case(f"rotated{n}x{k}", {"n": n, "n_colors": k, "adj_off": off, "adj": adj}, lists)


WIDE_RETRY_ROWS = (70, 129)  # the rows the two rewards open: the second chunk, and the last ordinal of the ragged third


def wide_retry_assignment(n=12):
    """retry_assignment with 130 rows: the rewards open rows 70 and 129, every other cost is positive."""
    import solverforge_amd as sfa

    cost = np.full((n, WIDE), 2, dtype=np.int64)
    cost[7, WIDE_RETRY_ROWS[0]], cost[9, WIDE_RETRY_ROWS[1]] = -1, -2
    cost[3, :] = np.tile([1, 4, 1, 5], WIDE)[:WIDE]
    row_w = np.ones(WIDE, dtype=np.int64)

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_assignment(start, cost, WIDE, n_replicas=R, row_w=row_w, ex_level=0)

    return Case("wideretry", n, WIDE, lambda sfo, start: sfo.Model.assignment(start, cost, WIDE, row_w=row_w, ex_level=0), gpu)


def wide_retry_value_keys(heuristic):
    """retry_value_keys for wide_retry_assignment: row 70 is the weakest value (heuristics 2, 3), or the first of the two strongest (70 and
    129, in different chunks); under AllocateToValueFromQueue it sorts to ordinal 128."""
    k = np.full(WIDE, 2, dtype=np.int64)
    if heuristic in (2, 3):
        k[:] = 3
        k[WIDE_RETRY_ROWS[0]], k[100] = 0, 1
    else:
        k[0], k[71] = 0, 1
        k[list(WIDE_RETRY_ROWS)] = 3
    return k


# ---- per-value tables wider than the wave -------------------------------------------------------------------------------------------------
def table_keys(n_values, least, seed=61):
    """Value keys with ties whose extreme -- the greatest key, or with least=True the least one -- occurs at values >= 64 only, first at
    value 64: the strongest-fit heuristics take it with least=False, AllocateToValueFromQueue's ascending order starts with it with least=True."""
    from solverforge_amd import datasets

    r = datasets.stream(seed, n_values)
    k = (r % np.uint64(2)).astype(np.int64)
    k[64:] = (r[64:] % np.uint64(3)).astype(np.int64)
    k[64] = 2
    return -k if least else k


def rotated_lists(n, n_values):
    """Entity e's values are the range rotated to start at n_values - 1 - 3 e (mod n_values): first-fit picks start at the last value and
    spread over the whole range."""
    return [[(n_values - 1 - 3 * e + j) % n_values for j in range(n_values)] for e in range(n)]


def wide_table_models():
    """name -> a function (value_lists) -> Case: models whose per-value tables hold 65 to 130 values, with more entities than 64 so that the
    constructed values reach indices >= 64.  12 * n_values is no multiple of 16 at 65, 70 and 130 values: the runs table of the shift models
    starts at the aligned end of the count table, not at its end."""
    models = {}
    for bins in (65, 130):
        for cap in (-1, 4, -2, -3):
            models[f"balance{cap}x{bins}"] = lambda lists, bins=bins, cap=cap: _with_lists(balance(n=bins + 10, n_bins=bins, cap=cap, seed=7), lists)
    models["assignment130"] = lambda lists: assignment(n=140, n_values=WIDE, seed=53, value_lists=lists)
    for nurses in (65, 70):
        models[f"shifts{nurses}"] = lambda lists, nurses=nurses: _with_lists(shift_schedule(n_nurses=nurses, n_days=40), lists)
        models[f"presence{nurses}"] = lambda lists, nurses=nurses: _with_lists(shift_schedule(n_nurses=nurses, n_days=40, presence=(2, 9, 3)), lists)
    return models


def _with_lists(case, lists):
    case.value_lists = lists
    return case


# ---- construction at a launch of several residencies --------------------------------------------------------------------------------------
AT_SIZE_SEED, AT_SIZE_SEARCH_STEPS, AT_SIZE_SHIFT = 9_100, 18, 5


def at_size_graph():
    """40 vertices, 3 colours, dense: FirstFit leaves vertices unassigned."""
    return graph(40, 180, 3, 13)


def at_size_entity_keys():
    return keys(40, 4, 67)


def at_size_start(sfo, case, r):
    """The start of replica r on the CPU: the all-unassigned model after AT_SIZE_SEARCH_STEPS steps of the scalar search seeded AT_SIZE_SEED + r."""
    o = case.oracle(sfo)
    o.configure(leaves=sfo.LEAF_SCALAR_CHANGE | sfo.LEAF_SCALAR_SWAP, random_seed=AT_SIZE_SEED + r)
    o.phase_start()
    o.steps(AT_SIZE_SEARCH_STEPS)
    return o.get_vars(0, 0)


# ---- the LDS gate of the per-value tables -------------------------------------------------------------------------------------------------
def gate_starts(n_values, n=40):
    """One head / reward value per entity, spread over the range: both ends, both sides of the first chunk boundary and of 64 KiB of tables."""
    marks = [n_values - 1, 0, 64, n_values - 2, 63, min(5460, n_values - 3), n_values // 2, min(5459, n_values - 4)]
    return [marks[e % len(marks)] for e in range(n)]


def gate_balance(n_values, n=40):
    """balance (the BalanceConstraint's statistic over the whole count table) whose value lists are rotations of the range: entities that
    share a head push each other to the next bins, at both ends of the tables."""
    heads = gate_starts(n_values, n)
    lists = [np.roll(np.arange(n_values), -h).tolist() for h in heads]
    return _with_lists(balance(n=n, n_bins=n_values, cap=-3, seed=7), lists)


def gate_assignment(n_values, n=40):
    """assignment with the exists node on the soft level: every cost is in 5..8 except one reward per entity (gate_starts) and a runner-up
    next to it, so CheapestInsertion has to find its value among all the chunks of the placement."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    cost = (datasets.stream(73, n * n_values) % np.uint64(4)).astype(np.int64).reshape(n, n_values) + 5
    for e, v in enumerate(gate_starts(n_values, n)):
        cost[e, v] = -50 - e
        cost[e, (v + 1) % n_values] = -40
    row_w = (datasets.stream(74, n_values) % np.uint64(4)).astype(np.int64) + 1

    def gpu(start, R, nullable):
        assert nullable
        return sfa.build_assignment(start, cost, n_values, n_replicas=R, row_w=row_w)

    return Case(f"gateassign{n_values}", n, n_values, lambda sfo, start: sfo.Model.assignment(start, cost, n_values, row_w=row_w), gpu)
