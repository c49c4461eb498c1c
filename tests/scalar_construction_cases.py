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
