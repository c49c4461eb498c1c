"""The TabuSearch acceptor of the reference restated in plain Python, for 1..4 score levels, with the four move signatures that have a
fixed size.  No device packing lives in the rules: tokens and identities are general tuples and only their equality is used, as in the
reference.  The GPU tests compare the device with this mirror; tests/test_tabu_mirror.py pins it to the reference's own unit tests
(tests/golden/tabu_goldens.json) and to the edge scripts below.

Restated from crates/solverforge-solver/src:
  phase/localsearch/acceptor/tabu_search.rs:12-62    TabuSearchPolicy: four optional tenures, an explicit 0 panics, one dimension at least
  builder/acceptor.rs:383-405                        normalize_tabu_search_policy: all four absent = move_only(10)
  tabu_search.rs:64-104                              TabuMemory: a FIFO of at most `tenure` entries; record evicts the oldest when full,
                                                     record_many pushes every token in order (no de-duplication)
  tabu_search.rs:162-173                             is_tabu: any entity token / any destination value token / move_id in the move memory /
                                                     move_id in the undo memory
  tabu_search.rs:181-236                             is_accepted (aspiration is strict and reads the acceptor's own best), phase_started,
                                                     phase_ended, step_ended (record, then best = max(best, step score) on every step)
  heuristic/move/metadata.rs:32-58,161-181           MoveTabuScope, scoped tokens, scoped_move_identity, ordered_coordinate_pair
  heuristic/move/change.rs:189-220, swap.rs:228-260, list_kernel/change.rs:28-34,155-204, list_kernel/swap.rs:110-155   the signatures

The reference hashes names and values (hash_str, hash_debug) into the u64 components; here the name / the value itself stands in its
place (None for NONE_ID), which compares equal exactly when the hashes would (barring SipHash collisions, which the reference ignores).

Also here: StampMemory, the stamp-table formulation of a TabuMemory that the device uses for the entity and value memories
(csrc/sf_tabu.h), checked against the FIFO by tests/test_tabu_mirror.py; DensePacker / ModelPacker, which map mirror signatures to the
device packing; the scripts in the form sf_debug_tabu_script takes them."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tabu_goldens.json")
MEMORIES = ("entity", "value", "move", "undo")


# ---- policy ----------------------------------------------------------------------------------------------------------------------
def normalize_policy(policy):
    """policy = [entity, value, move, undo, aspiration_enabled] (None = absent) or {"move_only": n} -> the validated five-tuple.
    ValueError with the reference's panic message for an explicit 0."""
    if isinstance(policy, dict):
        policy = [None, None, policy["move_only"], None, True]
    sizes, aspiration = list(policy[:4]), bool(policy[4])
    if all(s is None for s in sizes):
        sizes = [None, None, 10, None]  # TabuSearchPolicy::move_only(10)
    for name, s in zip(MEMORIES, sizes):
        if s == 0:
            raise ValueError("tabu_search field `%s_tabu_size` must be greater than 0" % ("undo_move" if name == "undo" else name))
    assert any(s is not None for s in sizes), "tabu_search requires at least one tabu dimension"
    return tuple(sizes) + (aspiration,)


# ---- memories --------------------------------------------------------------------------------------------------------------------
class TabuMemory:
    def __init__(self, tenure):
        self.tenure, self.entries, self.pushes = tenure, [], 0

    def contains(self, entry):
        return entry in self.entries

    def record(self, entry):
        if self.tenure is None:
            return
        if len(self.entries) >= self.tenure:
            self.entries.pop(0)
        self.entries.append(entry)
        self.pushes += 1

    def record_many(self, entries):
        for e in entries:
            self.record(e)

    def clear(self):
        self.entries, self.pushes = [], 0


class StampMemory:
    """The same memory as a stamp table: the 1-based ordinal of every token's latest push and a push counter.  The FIFO holds the last
    min(tenure, pushes) pushes; a token is among them exactly when its latest push is."""

    def __init__(self, tenure):
        self.tenure, self.stamp, self.pushes = tenure, {}, 0

    def contains(self, entry):
        st = self.stamp.get(entry, 0)
        return self.tenure is not None and st != 0 and self.pushes - st < self.tenure

    def record(self, entry):
        if self.tenure is None:
            return
        self.pushes += 1
        self.stamp[entry] = self.pushes

    def clear(self):
        self.stamp, self.pushes = {}, 0


# ---- signatures ------------------------------------------------------------------------------------------------------------------
class Sig:
    """MoveTabuSignature: entity tokens and destination value tokens are (scope, id) pairs, identities are tuples."""

    def __init__(self, scope, entities, values, move_id, undo_move_id):
        self.scope = tuple(scope)
        self.entity_tokens = [(self.scope, e) for e in entities]
        self.value_tokens = [(self.scope, v) for v in values]
        self.move_id, self.undo_move_id = tuple(move_id), tuple(undo_move_id)

    def __repr__(self):
        return "Sig(%r, %r, %r, %r, %r)" % (self.scope, [e for _, e in self.entity_tokens], [v for _, v in self.value_tokens], self.move_id, self.undo_move_id)


def change_signature(scope, entity, frm, to):
    """ChangeMove::tabu_signature (change.rs:189-220); frm / to = values, None = unassigned."""
    d, var = scope
    return Sig(scope, [entity], [to], (d, var, entity, frm, to), (d, var, entity, to, frm))


def swap_signature(scope, left, right, left_value, right_value):
    """SwapMove::tabu_signature (swap.rs:228-260): destination values are the right value then the left value; one ordered identity."""
    d, var = scope
    mid = ("swap", d, var, min(left, right), max(left, right))
    return Sig(scope, [left, right], [right_value, left_value], mid, mid)


def adjusted_destination(a, i, b, j):
    """ChangeCoordinates::adjusted_destination (list_kernel/change.rs:28-34)."""
    return j - 1 if a == b and j > i else j


def list_change_signature(scope, a, i, b, j, moved):
    """change_tabu_signature (list_kernel/change.rs:155-204): element `moved` from (a, i) to (b, j), j before the removal."""
    d, var = scope
    ja = adjusted_destination(a, i, b, j)
    return Sig(scope, [a] + ([b] if b != a else []), [moved], (d, var, a, i, b, ja, moved), (d, var, b, ja, a, i, moved))


def list_swap_signature(scope, a, i, first_value, b, j, second_value):
    """swap_tabu_signature (list_kernel/swap.rs:110-155): (a, i) holds first_value, (b, j) holds second_value."""
    d, var = scope
    p, q = sorted([(a, i), (b, j)])
    mid = ("list_swap", d, var, p[0], p[1], q[0], q[1])
    return Sig(scope, [a] + ([b] if b != a else []), [second_value, first_value], mid, mid)


# ---- the acceptor ----------------------------------------------------------------------------------------------------------------
class TabuSearch:
    def __init__(self, policy):
        e, v, m, u, self.aspiration_enabled = normalize_policy(policy)
        self.tenures = (e, v, m, u)
        self.mem = {"entity": TabuMemory(e), "value": TabuMemory(v), "move": TabuMemory(m), "undo": TabuMemory(u)}
        self.best = None

    def tabu_reasons(self, sig):
        """The memories that hold the signature (is_tabu = any)."""
        out = set()
        if any(self.mem["entity"].contains(t) for t in sig.entity_tokens):
            out.add("entity")
        if any(self.mem["value"].contains(t) for t in sig.value_tokens):
            out.add("value")
        if self.mem["move"].contains(sig.move_id):
            out.add("move")
        if self.mem["undo"].contains(sig.move_id):  # the candidate's move id against the stored undo ids
            out.add("undo")
        return out

    def is_aspirational(self, move_score):
        return self.best is not None and self.aspiration_enabled and tuple(move_score) > self.best

    def is_accepted(self, last_step_score, move_score, sig):
        if sig is None:
            raise RuntimeError("tabu search requires move signatures")
        return self.is_aspirational(move_score) or not self.tabu_reasons(sig)

    def _clear(self):
        for m in self.mem.values():
            m.clear()

    def phase_started(self, initial):
        self._clear()
        self.best = tuple(initial)

    def phase_ended(self):
        self._clear()
        self.best = None

    def step_ended(self, step_score, sig):
        if sig is not None:
            self.mem["entity"].record_many(sig.entity_tokens)
            self.mem["value"].record_many(sig.value_tokens)
            self.mem["move"].record(sig.move_id)
            self.mem["undo"].record(sig.undo_move_id)
        if self.best is None or tuple(step_score) > self.best:
            self.best = tuple(step_score)

    def state(self):
        """(best, pushes per memory, set of tabu entity tokens, set of tabu value tokens, move ids oldest first, undo ids oldest first)."""
        return (self.best, tuple(self.mem[k].pushes for k in MEMORIES), set(self.mem["entity"].entries), set(self.mem["value"].entries),
                list(self.mem["move"].entries), list(self.mem["undo"].entries))


# ---- scripts ---------------------------------------------------------------------------------------------------------------------
def _load(script):
    s = dict(script)
    s["sigs"] = {k: Sig(v["scope"], v["entities"], v["values"], v["move_id"], v["undo_move_id"]) for k, v in script.get("sigs", {}).items()}
    return s


def golden_file():
    with open(GOLDEN) as f:
        return json.load(f)


def goldens():
    """The reference's acceptor tests that are call sequences (the zero-tenure test is a list of refused policies: policy_error_golden)."""
    return [_load(s) for s in golden_file()["scripts"] if "ops" in s]


def policy_error_golden():
    return [s for s in golden_file()["scripts"] if "policy_errors" in s][0]


def run(script):
    """The mirror over a script: [(op, result, reasons)] with result = the decision of an is_accepted ("panics" where it raised) and
    reasons = the memories that held the candidate.  AssertionError where the script's own expectation differs."""
    a = TabuSearch(script["policy"])
    out = []
    for op in script["ops"]:
        res = reasons = None
        if op[0] == "phase_started":
            a.phase_started(op[1])
        elif op[0] == "is_accepted":
            sig = script["sigs"][op[3]] if op[3] is not None else None
            try:
                res = a.is_accepted(op[1], op[2], sig)
                reasons = a.tabu_reasons(sig)
            except RuntimeError:
                res = "panics"
            assert res == op[4], (script["name"], op, res)
        elif op[0] == "step_ended":
            a.step_ended(op[1], script["sigs"][op[2]] if op[2] is not None else None)
        elif op[0] == "phase_ended":
            a.phase_ended()
        else:
            raise ValueError(op[0])
        out.append((op, res, reasons, a.state()))
    return out


P, A, E = "phase_started", "is_accepted", "step_ended"
S, S2 = (0, "x"), (1, "y")


def raw(entities=(), values=(), move_id=(0,), undo_move_id=(0,), scope=S):
    return Sig(scope, list(entities), list(values), move_id, undo_move_id)


def _edge(name, policy, levels, sigs, ops):
    return {"name": name, "source": "hand-written", "levels": levels, "policy": policy, "sigs": sigs, "ops": ops}


def _steps(names, score=(-9,)):
    return [[E, list(score), n] for n in names]


# Every edge is asserted on the mirror by tests/test_tabu_mirror.py (EDGE_CHECKS there, one per script).
EDGE_SCRIPTS = [
    # tenure 1 in each memory: the one recorded entry is tabu, and the next record replaces it
    _edge("tenure_1_each_memory", [1, 1, 1, 1, False], 1,
          {"a": raw([1], [2], (3,), (4,)), "b": raw([5], [6], (7,), (8,)), "pe": raw([1], [], (100,), (101,)), "pv": raw([], [2], (102,), (103,)),
           "pm": raw([], [], (3,), (104,)), "pu": raw([], [], (4,), (105,))},
          [[P, [-10]], [E, [-9], "a"], [A, [-9], [-9], "pe", False], [A, [-9], [-9], "pv", False], [A, [-9], [-9], "pm", False], [A, [-9], [-9], "pu", False],
           [E, [-9], "b"], [A, [-9], [-9], "pe", True], [A, [-9], [-9], "pv", True], [A, [-9], [-9], "pm", True], [A, [-9], [-9], "pu", True]]),
    # two tokens recorded into a tenure-1 memory: only the second survives
    _edge("two_tokens_tenure_1", [1, 1, None, None, False], 1,
          {"s": raw([1, 2], [3, 4], (9,), (9,)), "e1": raw([1]), "e2": raw([2]), "v3": raw([], [3]), "v4": raw([], [4])},
          [[P, [-10]], [E, [-9], "s"], [A, [-9], [-9], "e1", True], [A, [-9], [-9], "e2", False], [A, [-9], [-9], "v3", True], [A, [-9], [-9], "v4", False]]),
    # one entity recorded in two consecutive steps takes two slots and leaves only when both are evicted
    _edge("entity_twice_two_slots", [3, None, None, None, False], 1,
          {"a": raw([1], [], (1,)), "b": raw([1], [], (2,)), "c": raw([2], [], (3,)), "d": raw([3], [], (4,)), "e": raw([4], [], (5,)), "p": raw([1], [], (6,))},
          [[P, [-10]]] + _steps("abc") + [[A, [-9], [-9], "p", False]] + _steps("d") + [[A, [-9], [-9], "p", False]] + _steps("e") + [[A, [-9], [-9], "p", True]]),
    # eviction at exactly `tenure` later pushes and not one earlier, in a stamp table and in a ring
    _edge("eviction_at_exactly_tenure", [3, None, 3, None, False], 1,
          {"m1": raw([1], [], (1,)), "m2": raw([2], [], (2,)), "m3": raw([3], [], (3,)), "m4": raw([4], [], (4,)), "pe": raw([1], [], (50,)), "pm": raw([], [], (1,))},
          [[P, [-10]]] + _steps(["m1", "m2", "m3"]) + [[A, [-9], [-9], "pe", False], [A, [-9], [-9], "pm", False]] + _steps(["m4"]) +
          [[A, [-9], [-9], "pe", True], [A, [-9], [-9], "pm", True]]),
    # a token that was never recorded, queried while fewer than `tenure` pushes exist (a stamp of 0 must not read as "pushed at ordinal 0")
    _edge("never_recorded_below_tenure", [5, 5, 5, 5, False], 1,
          {"a": raw([1], [1], (1,), (2,)), "fresh": raw([0], [0], (7,), (8,)), "fresh9": raw([9], [9], (9,), (9,))},
          [[P, [-10]], [A, [-10], [-10], "fresh", True], [E, [-9], "a"], [A, [-9], [-9], "fresh", True], [A, [-9], [-9], "fresh9", True], [A, [-9], [-9], "a", False]]),
    # the move ring wrapped at least three times
    _edge("move_ring_wraps_three_times", [None, None, 2, None, False], 1,
          dict({"m%d" % k: raw([], [], (k,), (100 + k,)) for k in range(1, 8)}),
          [[P, [-10]]] + _steps(["m%d" % k for k in range(1, 8)]) + [[A, [-9], [-9], "m5", True], [A, [-9], [-9], "m6", False], [A, [-9], [-9], "m7", False]]),
    # X -> Y applied: Y -> X is refused by the undo memory alone, X -> Y again by the move memory alone
    _edge("undo_alone_then_move_alone", [None, None, 1, 1, False], 1,
          {"xy": change_signature(S, 3, 0, 1), "yx": change_signature(S, 3, 1, 0), "other": change_signature(S, 4, 0, 1)},
          [[P, [-10]], [E, [-9], "xy"], [A, [-9], [-9], "yx", False], [A, [-9], [-9], "xy", False], [A, [-9], [-9], "other", True]]),
    # a swap is its own undo: refused by both
    _edge("swap_refused_by_both", [None, None, 1, 1, False], 1,
          {"s": swap_signature(S, 2, 5, 0, 1), "flipped": swap_signature(S, 5, 2, 0, 1)},
          [[P, [-10]], [E, [-9], "s"], [A, [-9], [-9], "flipped", False]]),
    # to = None is a value token of its own
    _edge("to_none", [None, 2, None, None, False], 1,
          {"unassign": change_signature(S, 1, 2, None), "other_unassign": change_signature(S, 5, 0, None), "assign0": change_signature(S, 5, None, 0)},
          [[P, [-10]], [E, [-9], "unassign"], [A, [-9], [-9], "other_unassign", False], [A, [-9], [-9], "assign0", True]]),
    # an intra-list change carries one entity token, and its identity the adjusted destination
    _edge("intra_list_change_one_entity", [2, None, 2, None, False], 1,
          {"intra": list_change_signature(S, 0, 1, 0, 3, 7), "from0": list_change_signature(S, 0, 0, 1, 0, 8), "from1": list_change_signature(S, 1, 0, 2, 0, 9),
           "same_adjusted": list_change_signature(S, 0, 1, 0, 3, 7)},
          [[P, [-10]], [E, [-9], "intra"], [A, [-9], [-9], "from0", False], [A, [-9], [-9], "from1", True], [A, [-9], [-9], "same_adjusted", False]]),
    # aspiration is strict, decided on the last of four levels
    _edge("four_levels_equal_not_aspirational", [1, None, None, None, True], 4,
          {"a": raw([1], [], (1,)), "p": raw([1], [], (2,))},
          [[P, [0, -1, 0, -10]], [E, [0, -1, 0, -10], "a"], [A, [0, -1, 0, -10], [0, -1, 0, -10], "p", False], [A, [0, -1, 0, -10], [0, -1, 0, -9], "p", True],
           [A, [0, -1, 0, -10], [0, -1, 0, -11], "p", False]]),
    _edge("aspiration_off", [1, None, None, None, False], 1,
          {"a": raw([1], [], (1,)), "p": raw([1], [], (2,))},
          [[P, [-10]], [E, [-9], "a"], [A, [-9], [1000], "p", False]]),
    # best is the acceptor's own: unchanged by an equal step score and by a step that applied nothing; raised by a step without a move too
    _edge("best_unchanged_by_equal_and_empty_steps", [1, None, None, None, True], 1,
          {"a": raw([1], [], (1,)), "p": raw([1], [], (2,))},
          [[P, [-10]], [E, [-10], "a"], [E, [-12], None], [A, [-12], [-10], "p", False], [A, [-12], [-9], "p", True], [E, [-8], None], [E, [-8], None],
           [A, [-8], [-8], "p", False], [A, [-8], [-7], "p", True]]),
    # the same ids under two scopes are different tokens and different identities
    _edge("same_id_two_scopes", [2, 2, 2, 2, False], 1,
          {"in_x": change_signature(S, 3, 0, 1), "in_y": change_signature(S2, 3, 0, 1), "back_in_y": change_signature(S2, 3, 1, 0)},
          [[P, [-10]], [E, [-9], "in_x"], [A, [-9], [-9], "in_y", True], [A, [-9], [-9], "back_in_y", True], [A, [-9], [-9], "in_x", False]]),
    # all four tenures absent: move-only 10
    _edge("all_absent_is_move_only_10", [None, None, None, None, True], 1,
          dict({"m%d" % k: raw([1], [1], (k,), (k,)) for k in range(1, 13)}),
          [[P, [-10]]] + _steps(["m%d" % k for k in range(1, 11)]) + [[A, [-9], [-9], "m1", False], [A, [-9], [-9], "m12", True]] + _steps(["m11"]) +
          [[A, [-9], [-9], "m1", True], [A, [-9], [-9], "m2", False]]),
]


def all_scripts():
    return goldens() + EDGE_SCRIPTS


# ---- the device packing (csrc/sf_tabu.h) ------------------------------------------------------------------------------------------
NO_TOKEN = 0xFFFFFFFF
OP_CHANGE, OP_SWAP, OP_LIST_CHANGE, OP_LIST_SWAP = 1, 2, 3, 4
FIELD_LIMIT = 1 << 24


def tabu_pack(op, scope_id, f0=0, f1=0, f2=0, f3=0, f4=0):
    assert all(0 <= f < FIELD_LIMIT for f in (f0, f1, f2, f3, f4)) and 0 <= scope_id < 256
    return ((op << 56) | (scope_id << 48) | (f0 << 24) | f1, (f2 << 48) | (f3 << 24) | f4)


class ModelPacker:
    """Mirror signatures of a model's moves -> the device packing.  scopes: {scope: (scope number, entity token base, value token base)};
    values are value indices (None = unassigned) or element ids."""

    def __init__(self, scopes):
        self.scopes = dict(scopes)

    def entity(self, token):
        return self.scopes[token[0]][1] + token[1]

    def value(self, token):
        return self.scopes[token[0]][2] + (0 if token[1] is None else token[1] + 1)

    def identity(self, t):
        v1 = lambda v: 0 if v is None else v + 1  # noqa: E731
        if t[0] == "swap":
            return tabu_pack(OP_SWAP, self.scopes[(t[1], t[2])][0], t[3], t[4])
        if t[0] == "list_swap":
            return tabu_pack(OP_LIST_SWAP, self.scopes[(t[1], t[2])][0], t[3], t[4], t[5], t[6])
        sid = self.scopes[(t[0], t[1])][0]
        if len(t) == 5:
            return tabu_pack(OP_CHANGE, sid, t[2], v1(t[3]), v1(t[4]))
        assert len(t) == 7
        return tabu_pack(OP_LIST_CHANGE, sid, t[2], t[3], t[4], t[5], v1(t[6]))

    def sig(self, s):
        pad = lambda xs: (xs + [NO_TOKEN, NO_TOKEN])[:2]  # noqa: E731
        return {"entity": pad([self.entity(t) for t in s.entity_tokens]), "value": pad([self.value(t) for t in s.value_tokens]),
                "move_id": self.identity(s.move_id), "undo_move_id": self.identity(s.undo_move_id)}


class DensePacker(ModelPacker):
    """For scripts, whose tokens and identities are arbitrary: every distinct token gets the next index of its table, every distinct
    identity the next serial number (operation tag 15, which no builder uses).  Injective by construction."""

    def __init__(self):
        self.ent, self.val, self.ids = {}, {}, {}

    def entity(self, token):
        return self.ent.setdefault(token, len(self.ent))

    def value(self, token):
        return self.val.setdefault(token, len(self.val))

    def identity(self, t):
        return (15 << 56) | self.ids.setdefault(tuple(t), len(self.ids)), 0


# ---- a script as sf_debug_tabu_script runs it ------------------------------------------------------------------------------------
OP_PHASE_STARTED, OP_DECIDE, OP_STEP_ENDED = 0, 1, 2
MASKED_LANES = (7, 40)  # candidates that never reach the acceptor: their ballot bit must stay 0
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _candidates(a, sig, sc, levels):
    """64 (signature, score) pairs for one decide record.  Lane 0 is the script's own candidate.  The others: for every live entry of every
    memory a signature that only that memory holds, one that all of them hold, one that none holds, and the script's own; each with a score
    below, at and above the acceptor's best (the last level moved by one), and with the script's score."""
    fresh = ("fresh", 0)
    sigs = [sig, Sig(sig.scope, [fresh], [fresh], ("fresh",), ("fresh",))]
    ent, val = sorted(a.mem["entity"].entries, key=repr), sorted(a.mem["value"].entries, key=repr)
    mov, und = list(a.mem["move"].entries), list(a.mem["undo"].entries)

    def make(e, v, m):
        s = Sig(sig.scope, [], [], m if m is not None else ("fresh",), ("fresh",))
        s.entity_tokens, s.value_tokens = ([e] if e is not None else []), ([v] if v is not None else [])
        return s

    sigs += [make(e, None, None) for e in ent[-2:]] + [make(None, v, None) for v in val[-2:]] + [make(None, None, m) for m in mov[-2:] + und[-2:]]
    if ent and val:
        sigs.append(make(ent[0], val[0], mov[0] if mov else (und[0] if und else None)))
    if ent and sig.entity_tokens:  # two tokens, the second one tabu
        s = make(fresh, None, None)
        s.entity_tokens = [fresh, ent[-1]]
        sigs.append(s)
    best = list(a.best)
    scores = [tuple(sc)]
    for d in (0, 1, -1):
        c = list(best)
        c[levels - 1] = min(max(c[levels - 1] + d, I64_MIN), I64_MAX)
        scores.append(tuple(c))
    if levels > 1:  # a higher level decides against the last one
        scores.append(tuple([best[0] + 1] + [x - 5 for x in best[1:]]))
        scores.append(tuple([best[0] - 1] + [x + 5 for x in best[1:]]))
    out = [(sig, tuple(sc))]
    k = 0
    while len(out) < 64:
        out.append((sigs[k % len(sigs)], scores[(k // len(sigs) + k) % len(scores)]))
        k += 1
    return out


def device_plan(script, packer=None):
    """The records of a script and what the mirror says of each: (plan, packer); plan = a list of dicts {op, score, cands (64 (packed
    signature, score) pairs) or None, sig (packed) or None, reach, accept (the expected ballot), state}.  phase_ended has no record (the
    device has no phase end: a phase start clears everything), nor has an is_accepted without a signature (the device cannot express it).
    state = (best padded to 4, pushes[4], sorted packed tabu entity tokens, sorted packed tabu value tokens, packed move ids oldest first,
    packed undo ids oldest first)."""
    packer = packer or DensePacker()
    a = TabuSearch(script["policy"])
    levels = script["levels"]
    reach = (1 << 64) - 1
    for lane in MASKED_LANES:
        reach &= ~(1 << lane)
    pad = lambda t: tuple(t) + (0,) * (4 - len(t))  # noqa: E731
    plan = []
    for op in script["ops"]:
        rec = None
        if op[0] == "phase_started":
            a.phase_started(op[1])
            rec = {"op": OP_PHASE_STARTED, "score": pad(op[1]), "cands": None, "sig": None, "reach": 0, "accept": 0}
        elif op[0] == "is_accepted":
            if op[3] is None:
                continue
            cands = _candidates(a, script["sigs"][op[3]], op[2], levels)
            ballot, kinds = 0, set()
            for lane, (s, c) in enumerate(cands):
                ok = a.is_accepted(op[1], c, s)
                kinds.add((frozenset(a.tabu_reasons(s)), tuple(c) > a.best))  # (the memories that hold it, its score beats the acceptor's best)
                if (reach >> lane) & 1 and ok:
                    ballot |= 1 << lane
            assert bool(ballot & 1) == op[4]
            rec = {"op": OP_DECIDE, "score": pad(op[1]), "cands": [(packer.sig(s), pad(c)) for s, c in cands], "sig": None, "reach": reach, "accept": ballot,
                   "kinds": kinds}
        elif op[0] == "step_ended":
            sig = script["sigs"][op[2]] if op[2] is not None else None
            a.step_ended(op[1], sig)
            rec = {"op": OP_STEP_ENDED, "score": pad(op[1]), "cands": None, "sig": packer.sig(sig) if sig is not None else None, "reach": 0, "accept": 0}
        elif op[0] == "phase_ended":
            a.phase_ended()
        if rec is not None:
            rec["state"] = packed_state(a, packer)
            plan.append(rec)
    return plan, packer


def packed_state(a, packer):
    best, pushes, ent, val, mov, und = a.state()
    pad = lambda t: tuple(t) + (0,) * (4 - len(t))  # noqa: E731
    return (pad(best), pushes, sorted(packer.entity(t) for t in ent), sorted(packer.value(t) for t in val), [packer.identity(t) for t in mov],
            [packer.identity(t) for t in und])
