"""The scalar ruin-and-recreate leaf restated over an oracle Model (test infrastructure; the oracle itself cannot run the leaf).

Sources (paths under crates/solverforge-solver/src/):
    heuristic/selector/scalar_neighborhood/cursor.rs:234-256    one SmallRng per solve: seed_from_u64(scoped_seed(random_seed, descriptor, variable,
                                                                "scalar_ruin_recreate_move_selector")); every cursor open draws from it
    scalar_neighborhood/cursor/ruin.rs:13-48                    generate_ruin_batches: identity, ruin count (no draw when min == max), partial
                                                                Fisher-Yates, the first ruin_count entries in swap order
    scalar_neighborhood/cursor.rs:144-175, move_selector/iter.rs:87-157   apply_selection_order(0x5CA1_A2C0_7A11_0001 ^ slot identity)
    scalar_neighborhood/cursor/ruin.rs:87-141                   emission against the snapshot taken at open
    scalar_neighborhood/move/apply.rs:337-450                   run_ruin_recreate, choose_first_fit, choose_cheapest_insertion
    phase/localsearch/acceptor/{hill_climbing,late_acceptance}.rs, forager.rs   the step rule of the one-leaf case (the files csrc/sf_step.h cites)
rand's xoshiro256++ and random_range (Canon's method) are restated from the published algorithm, as in oracle/sfo_core.hpp.

A model is anything with score(), get_vars(desc, var), apply_move(move) and evaluate_moves(moves) -- an oracle Model, or a test double."""
import json
import os

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
OFFSET_MIX = 0xD1B54A32D192ED03
STRIDE_SALT_MIX = 0xA24BAED4963EE407
SALT_ORDER = 0x5CA1A2C07A110001
SELECTOR_KIND = "scalar_ruin_recreate_move_selector"
ORDER_ORIGINAL, ORDER_RANDOM, ORDER_SHUFFLED = 0, 3, 4
FIRST_FIT, CHEAPEST_INSERTION = 0, 1
HILL_CLIMBING, LATE_ACCEPTANCE = 0, 1
ACCEPTED_COUNT, BEST_SCORE = 0, 2
KIND_CHANGE, KIND_SCALAR_RUIN = 0, 11
COUNTERS = ["step_count", "moves_generated", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations", "moves_not_doable"]


def golden_file():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalar_ruin_goldens.json")) as f:
        return json.load(f)


def check_bounds(min_ruin_count, max_ruin_count):
    """spec.rs:126-131: the reference's two bound errors (None = the spec is accepted)."""
    if min_ruin_count < 1:
        return "min_ruin_count must be at least 1"
    if max_ruin_count < min_ruin_count:
        return "max_ruin_count must be >= min_ruin_count"
    return None


class Stream:
    """SmallRng (xoshiro256++) from the oracle's seeding and generator; next_u32 is the upper half of next_u64."""

    def __init__(self, sfo, seed):
        self.sfo = sfo
        self.state = np.zeros(4, dtype=np.uint64)
        sfo.lib().sfo_small_rng_seed(seed & MASK, self.state.ctypes.data)
        self.buf, self.pos = np.zeros(0, dtype=np.uint64), 0

    def next_u64(self):
        if self.pos >= len(self.buf):
            buf = np.zeros(max(1024, 2 * len(self.buf)), dtype=np.uint64)
            self.sfo.lib().sfo_xoshiro256pp(self.state.ctypes.data, len(buf), buf.ctypes.data)  # the stream from its start: a prefix of it is what we had
            self.buf = buf
        v = int(self.buf[self.pos])
        self.pos += 1
        return v

    def next_u32(self):
        return self.next_u64() >> 32

    def random_range(self, low, high):
        """UniformInt<u32>::sample_single_inclusive: Canon's method with one extra step."""
        rng = high - low + 1
        m = self.next_u32() * rng
        result, lo_order = m >> 32, m & 0xFFFFFFFF
        if lo_order > ((1 << 32) - rng) & 0xFFFFFFFF:
            new_hi = (self.next_u32() * rng) >> 32
            if lo_order + new_hi > 0xFFFFFFFF:
                result += 1
        return low + result


def generate_ruin_batches(entity_count, min_ruin_count, max_ruin_count, moves_per_step, rng):
    mn, mx = min(min_ruin_count, entity_count), min(max_ruin_count, entity_count)
    permutation = list(range(entity_count))
    batches = []
    for _ in range(moves_per_step):
        if entity_count == 0:
            batches.append([])
            continue
        for index in range(entity_count):
            permutation[index] = index
        ruin_count = mn if mn == mx else rng.random_range(mn, mx)
        for index in range(ruin_count):
            swap_index = rng.random_range(index, entity_count - 1)
            permutation[index], permutation[swap_index] = permutation[swap_index], permutation[index]
        batches.append(permutation[:ruin_count])
    return batches


class Context:
    """MoveStreamContext (iter.rs:14-207) from splitmix64."""

    def __init__(self, sfo, step_index, step_seed, order):
        self.sfo, self.step_index, self.step_seed, self.order = sfo, step_index, step_seed, order

    def mixed_seed(self, salt):
        return self.sfo.splitmix64(self.step_seed ^ ((self.step_index * GOLDEN) & MASK) ^ salt)

    def random_index(self, n, salt):
        return 0 if n <= 1 else self.mixed_seed(salt) % n

    def random_stride(self, n, salt):
        if n <= 1:
            return 1
        stride = self.mixed_seed(salt) % (n - 1) + 1
        while np.gcd(stride, n) != 1:
            stride = 1 if stride == n - 1 else stride + 1
        return stride

    def selection_index(self, offset, n, salt):
        if self.order in (0, 1, 2):
            return offset
        if self.order == ORDER_RANDOM:
            return self.random_index(n, salt ^ ((offset * OFFSET_MIX) & MASK))
        start = self.random_index(n, salt)
        stride = self.random_stride(n, salt ^ STRIDE_SALT_MIX)
        return (start + offset * stride) % n

    def apply_selection_order(self, values, salt):
        if self.order in (0, 1, 2):
            return list(values)
        return [values[self.selection_index(offset, len(values), salt)] for offset in range(len(values))]


class RuinLeaf:
    """The leaf over a model.  value_lists: per-entity canonical lists, or None for the range 0..n_values."""

    def __init__(self, sfo, model, n_entities, n_values, random_seed, descriptor_index=0, variable_index=0, variable_name="value", min_ruin_count=2,
                 max_ruin_count=5, moves_per_step=10, value_candidate_limit=None, recreate=FIRST_FIT, allows_unassigned=True, value_lists=None,
                 levels=2):
        assert check_bounds(min_ruin_count, max_ruin_count) is None
        self.sfo, self.m, self.n, self.n_values = sfo, model, n_entities, n_values
        self.desc, self.var = descriptor_index, variable_index
        self.mn, self.mx, self.mps = min_ruin_count, max_ruin_count, max(moves_per_step or 10, 1)
        self.limit, self.recreate, self.allows_unassigned, self.value_lists, self.levels = value_candidate_limit, recreate, allows_unassigned, value_lists, levels
        self.rng = Stream(sfo, sfo.scoped_seed(random_seed, descriptor_index, variable_name, SELECTOR_KIND))
        self.inner_trials = 0

    def score(self):
        return tuple(int(x) for x in self.m.score()[:self.levels])

    def values(self):
        return [int(x) for x in self.m.get_vars(self.desc, self.var)]

    def candidates(self, entity):
        c = list(range(self.n_values)) if self.value_lists is None else list(self.value_lists[entity])
        return c if self.limit is None else c[:self.limit]

    def _change(self, entity, value):
        self.m.apply_move((KIND_CHANGE, entity, 0, 0, 0, value))

    def do_move(self, batch):
        """run_ruin_recreate: returns (old values, the value every entity of the batch ends with)."""
        cur = self.values()
        old = [cur[e] for e in batch]
        for e in batch:
            if cur[e] >= 0:
                self._change(e, -1)
        result = []
        for e in batch:
            cands = self.candidates(e)
            baseline = self.score() if self.allows_unassigned else None
            chosen = None
            if cands:
                sc, dv = self.m.evaluate_moves([(KIND_CHANGE, e, 0, 0, 0, v) for v in cands])
                self.inner_trials += len(cands)
                scores = [tuple(int(x) for x in row[:self.levels]) for row in sc]
                if self.recreate == FIRST_FIT:
                    for k, v in enumerate(cands):
                        if dv[k] and (baseline is None or scores[k] > baseline):
                            chosen = v
                            break
                else:
                    best = None
                    for k, v in enumerate(cands):
                        if dv[k] and (best is None or scores[k] > scores[best]):
                            best = k
                    if best is not None and (baseline is None or scores[best] >= baseline):
                        chosen = cands[best]
            if chosen is not None:
                self._change(e, chosen)
            result.append(-1 if chosen is None else chosen)
        return old, result

    def undo(self, batch, old):
        cur = self.values()
        for e, o in zip(batch, old):
            if cur[e] != o:
                self._change(e, o)

    def is_doable(self, batch):
        """apply.rs:66-90 == the cursor's emission test (cursor/ruin.rs:87-141)."""
        cur = self.values()
        if not batch or not any(cur[e] >= 0 for e in batch):
            return False
        return self.allows_unassigned or all(cur[e] < 0 or len(self.candidates(e)) > 0 for e in batch)

    def open(self, ctx, advance=True):
        """One cursor open: the ordered batch table, every emitted batch with the result values and the score of its trial."""
        pos = self.rng.pos
        batches = generate_ruin_batches(self.n, self.mn, self.mx, self.mps, self.rng)
        if not advance:
            self.rng.pos = pos
        identity = ((self.desc << 32) ^ self.var) & MASK
        table = []
        for batch in ctx.apply_selection_order(batches, SALT_ORDER ^ identity):
            row = {"entities": list(batch), "emitted": self.is_doable(batch), "values": None, "score": None}
            if row["emitted"]:
                old, row["values"] = self.do_move(batch)
                row["score"] = self.score()
                self.undo(batch, old)
            table.append(row)
        return table

    def commit(self, row):
        cur = self.values()
        for e in row["entities"]:
            if cur[e] >= 0:
                self._change(e, -1)
        for e, v in zip(row["entities"], row["values"]):
            if v >= 0:
                self._change(e, v)


def public_table(table):
    return [{"entities": r["entities"], "emitted": r["emitted"], "values": r["values"]} for r in table]


class Search:
    """Local search over a Sequential union [before..., the ruin leaf, after...]: `before` / `after` = oracle leaf bits enumerated by the
    model itself.  acceptor HILL_CLIMBING (strictly better than the last step score, hill_climbing.rs) or LATE_ACCEPTANCE (not worse than the
    last step score or than the score `la_size` steps ago, late_acceptance.rs); forager BEST_SCORE (the whole cursor) or ACCEPTED_COUNT(limit)
    (the step ends at the limit-th accepted candidate); the pick is the best accepted score, the first of equals (random_ties off)."""

    def __init__(self, sfo, model, leaf, random_seed, acceptor=HILL_CLIMBING, la_size=5, forager=BEST_SCORE, limit=4, order=ORDER_RANDOM, before=(), after=()):
        self.sfo, self.m, self.leaf, self.seed = sfo, model, leaf, random_seed
        self.acceptor, self.la_size, self.forager, self.limit, self.order = acceptor, la_size, forager, limit, order
        self.before, self.after = list(before), list(after)
        self.step_index = 0
        self.current = leaf.score()
        self.best_score = self.current
        self.history = [self.current] * la_size
        self.stats = dict.fromkeys(COUNTERS, 0)

    def accepts(self, score, late):
        if self.acceptor == HILL_CLIMBING:
            return score > self.current
        return score >= self.current or score >= late

    def _enumerated(self, bits, seed):
        out = []
        moves = self.m.enumerate(bits, self.step_index, seed, self.order)
        if len(moves):
            sc, dv = self.m.evaluate_moves(moves)
            for mv, row, ok in zip(moves, sc, dv):
                out.append({"record": tuple(int(x) for x in mv.tolist()), "score": tuple(int(x) for x in row[:self.leaf.levels]), "doable": bool(ok), "move": mv, "row": None})
        return out

    def step(self, dry_run=False):
        seed = self.sfo.lib().sfo_step_seed(self.seed, self.step_index)
        ctx = Context(self.sfo, self.step_index, seed, self.order)
        table = self.leaf.open(ctx, advance=not dry_run)
        cands = []
        for bits in self.before:
            cands += self._enumerated(bits, seed)
        for ordinal, row in enumerate(table):
            if row["emitted"]:
                cands.append({"record": (KIND_SCALAR_RUIN, ordinal, len(row["entities"]), row["entities"][0], 0, 0), "score": row["score"], "doable": True, "move": None, "row": row})
        for bits in self.after:
            cands += self._enumerated(bits, seed)
        rec = {"step_index": self.step_index, "table": table, "candidates": cands}
        if dry_run:
            return rec
        late = self.history[self.step_index % self.la_size]
        accepted, consumed, pick = [], 0, None
        for i, c in enumerate(cands):
            consumed += 1
            ok = c["doable"] and self.accepts(c["score"], late)
            accepted.append(ok)
            if ok and (pick is None or c["score"] > cands[pick]["score"]):
                pick = i
            if self.forager == ACCEPTED_COUNT and sum(accepted) >= self.limit:
                break
        st = self.stats
        n_doable = sum(1 for c in cands[:consumed] if c["doable"])
        st["step_count"] += 1
        st["moves_generated"] += consumed
        st["moves_evaluated"] += consumed
        st["moves_accepted"] += sum(accepted)
        st["score_calculations"] += n_doable
        st["moves_not_doable"] += consumed - n_doable
        if pick is not None:
            c = cands[pick]
            if c["row"] is not None:
                self.leaf.commit(c["row"])
            else:
                self.m.apply_move(c["move"])
            self.current = c["score"]
            assert self.leaf.score() == self.current, (self.leaf.score(), self.current)
            st["moves_applied"] += 1
            if self.current > self.best_score:
                self.best_score = self.current
        self.history[self.step_index % self.la_size] = self.current
        self.step_index += 1
        rec.update(consumed=consumed, accepted=accepted, pick=pick, score=self.current)
        return rec
