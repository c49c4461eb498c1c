"""LimitedNeighborhood and the union scheduler restated over an oracle Model (test infrastructure: the oracle's UnionScheduler has no
per-child budget, so it cannot run a limited child, a limited root or a VND neighbourhood that is a composition).

Sources (paths under crates/solverforge-solver/src/):
    heuristic/selector/decorator/limited.rs:14-94       LimitedMoveCursor: `yielded < limit` is tested before the inner cursor is touched; a pull
                                                        the inner cursor answers counts one, a None counts nothing; the rest passes through
    heuristic/selector/decorator/limited/tests.rs:100-118   inner total 100, limit 3: three pulls, three inner generations, then None
    heuristic/selector/decorator/vec_union.rs:119-124   union_child_context: every child opens with the parent's context unchanged
    heuristic/selector/decorator/vec_union.rs:190-365   UnionScheduler: the five orders, fixed weights, offset and stride drawn over ITS child count
    builder/selector/types/composite.rs:72-89, composite/state.rs:89-106,190-193,265-267    Limited wraps a leaf or a union; the budget is per step
    phase/localsearch/vnd/phase.rs:79-80                VND opens neighbourhood k's composition alone and pulls it to its end

The step rule (HillClimbing / LateAcceptance under BestScore / AcceptedCount) is tests/scalar_ruin_mirror.py's Search.step as it stands; the
VND rule (pick, accepts, the counters) is tests/vnd_mirror.py's."""
import json
import os

import numpy as np

import scalar_ruin_mirror as srm
import vnd_mirror as vm

SEQUENTIAL, ROUND_ROBIN, ROTATING_ROUND_ROBIN, RANDOM, STRATIFIED_RANDOM = range(5)
ORDERS = (SEQUENTIAL, ROUND_ROBIN, ROTATING_ROUND_ROBIN, RANDOM, STRATIFIED_RANDOM)
SALT_OFFSET, SALT_STRIDE, SALT_DRAW = 0xA11CE5E1EC700001, 0xA11CE5E1EC700002, 0xA11CE5E1EC701000
MASK = (1 << 64) - 1
COUNTERS = srm.COUNTERS


def golden_file():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "limited_goldens.json")) as f:
        return json.load(f)


class ListCursor:
    """A cursor over a list that counts how often it generated (the reference test's CountingCursor)."""

    def __init__(self, items):
        self.items, self.generated = list(items), 0

    def next(self):
        if self.generated >= len(self.items):
            return None
        self.generated += 1
        return self.items[self.generated - 1]


class LimitedCursor:
    """LimitedMoveCursor (limited.rs:60-73).  limit None = the inner cursor itself."""

    def __init__(self, inner, limit):
        self.inner, self.limit, self.yielded = inner, limit, 0

    def next(self):
        if self.limit is not None and self.yielded >= self.limit:
            return None  # the inner cursor is not touched
        item = self.inner.next()
        if item is None:
            return None  # counts nothing
        self.yielded += 1
        return item


def limited(stream, n):
    """What a LimitedMoveCursor of limit n yields over `stream`, and how often the inner cursor generated."""
    inner = ListCursor(stream)
    cursor = LimitedCursor(inner, n)
    out = []
    while True:
        item = cursor.next()
        if item is None:
            break
        out.append(item)
    assert cursor.next() is None
    return out, inner.generated


class UnionCursor:
    """VecUnionMoveCursor over child cursors (vec_union.rs:190-365).  next() -> (child, item) or None."""

    def __init__(self, sfo, cursors, order, step_index, step_seed, weights=None):
        n = len(cursors)
        self.sfo, self.cursors, self.order, self.idx, self.seed = sfo, cursors, order, step_index, step_seed
        self.weights = [1] * n if weights is None else [int(w) for w in weights]
        assert len(self.weights) == n
        assert order in (RANDOM, STRATIFIED_RANDOM) or all(w == 1 for w in self.weights)
        self.exhausted = [w == 0 for w in self.weights]
        self.live = sum(1 for e in self.exhausted if not e)
        self.total = sum(self.weights)
        L = sfo.lib()
        self.offset = int(L.sfo_ctx_random_index(step_index, step_seed, n, SALT_OFFSET)) if order in (ROTATING_ROUND_ROBIN, STRATIFIED_RANDOM) else 0
        self.stride = int(L.sfo_ctx_random_stride(step_index, step_seed, n, SALT_STRIDE)) if order == STRATIFIED_RANDOM else 1
        self.current = 0 if order == STRATIFIED_RANDOM else self.offset
        self.draws = 0
        self.running = [0] * n

    def _drop(self, c):
        self.exhausted[c] = True
        self.live -= 1
        self.total -= self.weights[c]

    def next(self):
        n = len(self.cursors)
        if self.order == SEQUENTIAL:
            while self.current < n:
                item = self.cursors[self.current].next()
                if item is not None:
                    return self.current, item
                self.current += 1
            return None
        if self.order in (ROUND_ROBIN, ROTATING_ROUND_ROBIN):
            while self.live > 0:
                c = self.current % n
                self.current = (self.current + 1) % n
                if self.exhausted[c]:
                    continue
                item = self.cursors[c].next()
                if item is not None:
                    return c, item
                self.exhausted[c] = True
                self.live -= 1
            return None
        if self.order == RANDOM:
            while self.live > 0:
                draw = int(self.sfo.lib().sfo_ctx_mixed_seed(self.idx, self.seed, (SALT_DRAW + self.draws) & MASK)) % self.total
                self.draws += 1
                cumulative, c = 0, None
                for i, w in enumerate(self.weights):
                    if self.exhausted[i]:
                        continue
                    cumulative += w
                    if draw < cumulative:
                        c = i
                        break
                item = self.cursors[c].next()
                if item is not None:
                    return c, item
                self._drop(c)
            return None
        while self.live > 0:  # StratifiedRandom: the smooth weighted round-robin in rotated order
            sel, sel_w = None, None
            for pos in range(n):
                c = (self.offset + pos * self.stride) % n
                if self.exhausted[c]:
                    continue
                self.running[c] += self.weights[c]
                if sel is None or self.running[c] > sel_w:
                    sel, sel_w = c, self.running[c]
            self.running[sel] -= self.total
            item = self.cursors[sel].next()
            if item is not None:
                return sel, item
            self._drop(sel)
        return None


def union_stream(sfo, lengths, order, step_index, step_seed, weights=None, child_limits=None, root_limit=None):
    """The pulls of a step's cursor over children of the given lengths: [(child, index in child)].  child_limits: per child or None;
    root_limit: around the union.  A lone child is the child itself (no union node), limited the same way."""
    child_limits = [None] * len(lengths) if child_limits is None else list(child_limits)
    cursors = [LimitedCursor(ListCursor(range(n)), lim) for n, lim in zip(lengths, child_limits)]
    if len(cursors) == 1:
        class Lone:
            def next(self_inner):
                item = cursors[0].next()
                return None if item is None else (0, item)
        inner = Lone()
    else:
        inner = UnionCursor(sfo, cursors, order, step_index, step_seed, weights)
    root = LimitedCursor(inner, root_limit)
    out = []
    while True:
        item = root.next()
        if item is None:
            return out
        out.append(item)


class _NoRuinLeaf:
    """Search wants a ruin leaf: this one holds none and answers the model's score."""

    def __init__(self, model, levels):
        self.m, self.levels = model, levels

    def score(self):
        return tuple(int(x) for x in self.m.score()[:self.levels])

    def open(self, ctx, advance=True):
        return []


class LimitedSearch(srm.Search):
    """Local search whose step cursor is the (limited) union of `leaves` (oracle leaf bits in child order): the candidates of a step are the
    union stream's, everything else is Search.step."""

    def __init__(self, sfo, model, leaves, random_seed, union_order=STRATIFIED_RANDOM, weights=None, child_limits=None, root_limit=None, levels=2, **kw):
        super().__init__(sfo, model, _NoRuinLeaf(model, levels), random_seed, before=("union",), **kw)
        self.leaves, self.union_order, self.weights = list(leaves), union_order, weights
        self.child_limits, self.root_limit = child_limits, root_limit

    def stream(self, step_index, seed, order):
        """[(child, index in child, record)] of one step's cursor, and the child lists."""
        children = [self.m.enumerate(b, step_index, seed, order) for b in self.leaves]
        pulls = union_stream(self.sfo, [len(c) for c in children], self.union_order, step_index, seed, self.weights, self.child_limits, self.root_limit)
        return pulls, children

    def _enumerated(self, bits, seed):
        pulls, children = self.stream(self.step_index, seed, self.order)
        self.last_lengths = [len(c) for c in children]
        out = []
        if pulls:
            moves = np.array([children[c][i] for c, i in pulls], dtype=children[0].dtype)
            sc, dv = self.m.evaluate_moves(moves)
            for (c, i), mv, row, ok in zip(pulls, moves, sc, dv):
                out.append({"record": tuple(int(x) for x in mv.tolist()), "score": tuple(int(x) for x in row[:self.leaf.levels]), "doable": bool(ok),
                            "move": mv, "row": None, "child": c, "index": i})
        return out

    def step(self, dry_run=False):
        rec = super().step(dry_run)
        rec["lengths"] = self.last_lengths
        return rec


class LimitedVnd(vm.VndPhase):
    """The VND phase over neighbourhoods that are compositions.  hoods: [(leaf indices, union order, limit or None)] over `leaf_bits` (the
    declared leaves); child_limits: per declared leaf.  A record's `children` are global leaf indices."""

    def __init__(self, sfo, model, leaf_bits, hoods, seed_of_step, child_limits=None, levels=2):
        self.sfo, self.leaf_bits = sfo, list(leaf_bits)
        self.child_limits = [None] * len(self.leaf_bits) if child_limits is None else list(child_limits)
        super().__init__(model, hoods, seed_of_step, levels)

    def step(self):
        assert not self.done
        k = self.k
        members, order, limit = self.leaves[k]
        seed = self.seed_of_step(self.step_index)
        children = [self.m.enumerate(self.leaf_bits[l], self.step_index, seed, vm.ORDER_ORIGINAL) for l in members]
        pulls = union_stream(self.sfo, [len(c) for c in children], order, self.step_index, seed, None, [self.child_limits[l] for l in members], limit)
        moves = np.array([children[c][i] for c, i in pulls], dtype=children[0].dtype) if pulls else children[0][:0]
        sc, dv = self.m.evaluate_moves(moves) if len(moves) else ([], [])
        scores = [tuple(int(x) for x in row[:self.levels]) for row in sc]
        doable = [bool(x) for x in dv]
        sel = vm.pick(scores, doable, self.current)
        n_doable = sum(doable)
        best = [s for s, ok in zip(scores, doable) if ok and vm.accepts(s, self.current)]
        st = self.stats
        st["step_count"] += 1
        st["moves_generated"] += len(moves)
        st["moves_evaluated"] += len(moves)
        st["score_calculations"] += n_doable
        st["moves_not_doable"] += len(moves) - n_doable
        rec = {"k": k, "step_index": self.step_index, "cursor": len(moves), "pick": sel, "ties": sum(1 for s in best if s == max(best)) if best else 0,
               "moves": moves, "scores": scores, "doable": doable, "children": [members[c] for c, _ in pulls], "lengths": [len(c) for c in children],
               "offset_stride": None}
        if len(members) > 1 and order == STRATIFIED_RANDOM:
            L = self.sfo.lib()
            rec["offset_stride"] = tuple((int(L.sfo_ctx_random_index(self.step_index, seed, n, SALT_OFFSET)), int(L.sfo_ctx_random_stride(self.step_index, seed, n, SALT_STRIDE)))
                                         for n in (len(members), len(self.leaf_bits)))
        if sel is None:
            self.k += 1
            self.idle_steps += 1
        else:
            self.m.apply_move(moves[sel])
            self.current = scores[sel]
            assert self._score() == self.current
            if self.current > self.best_score:
                self.best_score = self.current
            st["moves_accepted"] += 1
            st["moves_applied"] += 1
            self.k = 0
        self.step_index += 1
        rec["score"] = self.current
        return rec
