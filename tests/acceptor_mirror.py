"""The GreatDeluge and StepCountingHillClimbing acceptors restated for scores of 1..4 levels, and the scripts they are tested on.

A score is a tuple of ints, compared lexicographically (hard_soft.rs:130-137, bendable.rs:210-230).  Integer arithmetic is i64 and wraps,
as the reference does in release builds.

  GreatDeluge               phase/localsearch/acceptor/great_deluge.rs:89-129
  StepCountingHillClimbing  phase/localsearch/acceptor/step_counting.rs:85-129
  Score::multiply           solverforge-core/src/score/macros.rs:61-63, bendable.rs:142-152: per level `(x as f64 * r).round() as i64`

A script is a dict {name, source, acceptor ("great_deluge" / "step_counting"), param (rain_speed / step_count_limit), levels, ops}; an op
is ["phase_started", score], ["is_accepted", last_step_score, move_score, expected bool], ["step_ended", step_score],
["since", expected steps_since_improvement] or ["phase_ended"].  tests/golden/acceptor_goldens.json holds the reference's own unit tests
in this form; EDGE_SCRIPTS below are hand-written, with `expect` naming what tests/test_acceptor_mirror.py asserts each one reaches."""
import json
import math
import os

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acceptor_goldens.json")


def wrap(x):
    """i64 wrap-around."""
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def as_f64(x):
    """`x as f64`: the nearest double, ties to even (Python's int -> float conversion rounds the same way)."""
    return float(x)


def f64_as_i64(v):
    """`v as i64`: NaN -> 0, saturating."""
    if v != v:
        return 0
    if v >= 9223372036854775808.0:
        return I64_MAX
    if v <= -9223372036854775808.0:
        return I64_MIN
    return int(v)


def round_half_away(v):
    """f64::round: half away from zero.  Exact: at |v| >= 2^52 a double is an integer already."""
    if v != v or math.isinf(v) or abs(v) >= 4503599627370496.0:
        return v
    t = float(math.trunc(v))
    return t + math.copysign(1.0, v) if abs(v - t) >= 0.5 else t


def multiply_level(x, r):
    return f64_as_i64(round_half_away(as_f64(x) * r))


class GreatDeluge:
    def __init__(self, rain_speed):
        self.rain_speed = float(rain_speed)
        self.water = None
        self.abs0 = None

    def phase_started(self, initial):  # :108-111
        self.water = tuple(initial)
        self.abs0 = tuple(wrap(-x) if x < 0 else x for x in initial)  # i64::abs; |i64::MIN| wraps

    def is_accepted(self, cur, sc):  # :90-106
        if tuple(sc) > tuple(cur):
            return True
        return True if self.water is None else tuple(sc) >= self.water

    def increment(self):
        return tuple(multiply_level(x, self.rain_speed) for x in self.abs0)

    def step_ended(self, step_score):  # :113-123
        if self.water is not None:
            self.water = tuple(wrap(w + i) for w, i in zip(self.water, self.increment()))

    def phase_ended(self):  # :125-128
        self.water = self.abs0 = None

    def state(self):
        """(level, increment, since) as sf_get_acceptor_state reports them."""
        return self.water, self.increment(), 0


class StepCounting:
    def __init__(self, step_count_limit):
        self.limit = int(step_count_limit)
        self.since = 0
        self.best = None

    def phase_started(self, initial):  # :101-104
        self.best = tuple(initial)
        self.since = 0

    def is_accepted(self, cur, sc):  # :86-99
        if tuple(sc) > tuple(cur):
            return True
        return self.since < self.limit

    def step_ended(self, step_score):  # :106-123
        if self.best is None or tuple(step_score) > self.best:
            self.best = tuple(step_score)
            self.since = 0
        else:
            self.since += 1

    def phase_ended(self):  # :125-128
        self.best = None
        self.since = 0

    def state(self):
        return self.best, tuple(0 for _ in self.best), self.since


def make(script):
    return GreatDeluge(script["param"]) if script["acceptor"] == "great_deluge" else StepCounting(script["param"])


def run(script):
    """The mirror over a script: the list of (op, result) with result = the decision of an is_accepted, the count of a since, else None.
    Raises AssertionError where the script's own expectation differs."""
    a = make(script)
    out = []
    for op in script["ops"]:
        res = None
        if op[0] == "phase_started":
            a.phase_started(op[1])
        elif op[0] == "is_accepted":
            res = a.is_accepted(op[1], op[2])
            assert res == op[3], (script["name"], op, res)
        elif op[0] == "step_ended":
            a.step_ended(op[1])
        elif op[0] == "since":
            res = a.since
            assert res == op[1], (script["name"], op, res)
        elif op[0] == "phase_ended":
            a.phase_ended()
        else:
            raise ValueError(op[0])
        out.append((op, res))
    return out


def goldens():
    with open(GOLDEN) as f:
        return json.load(f)["scripts"]


def _gd(name, expect, param, levels, ops):
    return {"name": name, "source": "hand-written", "acceptor": "great_deluge", "param": param, "levels": levels, "ops": ops, "expect": expect}


def _sc(name, expect, param, levels, ops):
    return {"name": name, "source": "hand-written", "acceptor": "step_counting", "param": param, "levels": levels, "ops": ops, "expect": expect}


P, A, E = "phase_started", "is_accepted", "step_ended"
BIG = (1 << 53) + 1
U64_MAX = (1 << 64) - 1

# expect: {"increment": per level} after the first phase start; {"product": the exact f64 product of level 0}; {"water_above_cur": True}: some
# is_accepted with move == last step score is refused while the water stands above it; {"since_max": the largest count the script reaches};
# {"reset_at": the count that an improving step_ended resets}
EDGE_SCRIPTS = [
    # |x| x r lands on .5 exactly: round half away from zero gives 3 (half to even would give 2), for both signs of the initial level
    _gd("half_negative_initial", {"increment": [3], "product": 2.5}, 0.5, 1,
        [[P, [-5]], [A, [-5], [-5], True], [A, [-5], [-6], False], [E, [-5]], [A, [0], [-2], True], [A, [0], [-3], False], [E, [-5]], [A, [2], [1], True], [A, [2], [0], False]]),
    _gd("half_positive_initial", {"increment": [3], "product": 2.5}, 0.5, 1,
        [[P, [5]], [A, [5], [5], True], [E, [5]], [A, [5], [5], False], [A, [5], [8], True], [A, [5], [7], True], [A, [4], [4], False]]),
    _gd("half_negative_speed", {"increment": [-3], "product": -2.5}, -0.5, 1,
        [[P, [5]], [E, [5]], [A, [5], [2], True], [A, [5], [1], False], [E, [5]], [A, [5], [-1], True], [A, [5], [-2], False]]),
    # an initial level of 0: the increment is 0 at any speed
    _gd("zero_initial", {"increment": [0]}, 1000.0, 1, [[P, [0]], [E, [0]], [E, [0]], [A, [0], [0], True], [A, [0], [-1], False], [A, [-3], [-2], True]]),
    _gd("zero_speed", {"increment": [0, 0]}, 0.0, 2,
        [[P, [-7, -300]], [E, [-7, -300]], [E, [-7, -250]], [A, [-7, -250], [-7, -300], True], [A, [-7, -250], [-7, -301], False]]),
    _gd("negative_speed", {"increment": [-1, -30]}, -0.1, 2,
        [[P, [-7, -300]], [A, [-7, -300], [-7, -301], False], [E, [-7, -300]], [A, [-7, -300], [-8, -330], True], [A, [-7, -300], [-8, -331], False]]),
    _gd("tiny_speed", {"increment": [0]}, 1e-300, 1, [[P, [-(1 << 62)]], [E, [-(1 << 62)]], [A, [-(1 << 62)], [-(1 << 62)], True], [A, [-(1 << 62)], [-(1 << 62) - 1], False]]),
    # four levels, the first three equal everywhere: the last level alone decides
    _gd("four_levels_last_decides", {"increment": [0, 1, 0, 10]}, 0.1, 4,
        [[P, [0, -10, 0, -100]], [E, [0, -10, 0, -100]],
         [A, [0, -9, 0, -100], [0, -9, 0, -90], True], [A, [0, -9, 0, -91], [0, -9, 0, -91], False], [A, [0, -9, 0, -91], [0, -9, 0, -90], True]]),
    # |initial| = 2^53 + 1 is no double: the conversion rounds to 2^53 before the multiply
    _gd("initial_past_2_53", {"increment": [1 << 53], "product": float(1 << 53)}, 1.0, 1,
        [[P, [-BIG]], [E, [-BIG]], [A, [0], [-1], True], [A, [0], [-2], False]]),
    # the water rises above the last step score: a candidate equal to it is refused
    _gd("water_above_cur", {"increment": [10], "water_above_cur": True}, 0.1, 1,
        [[P, [-100]], [A, [-100], [-100], True], [E, [-100]], [A, [-100], [-100], False], [A, [-100], [-95], True], [A, [-100], [-90], True]]),
    _sc("limit_0", {"since_max": 2}, 0, 1, [[P, [-100]], [A, [-100], [-100], False], [A, [-100], [-99], True], [E, [-100]], [E, [-100]], [A, [-100], [-101], False]]),
    _sc("limit_1", {"since_max": 1}, 1, 1, [[P, [-100]], [A, [-100], [-110], True], [E, [-110]], [A, [-110], [-110], False], [A, [-110], [-109], True]]),
    _sc("limit_u64_max", {"since_max": 3}, U64_MAX, 1, [[P, [-100]], [E, [-110]], [E, [-120]], [E, [-130]], [A, [-130], [-(1 << 62)], True]]),
    # an improving step exactly at since == limit - 1 resets the count before it closes the door; later it does reach the limit
    _sc("reset_at_limit_minus_1", {"since_max": 3, "reset_at": 2}, 3, 2,
        [[P, [0, -100]], [E, [0, -110]], [E, [0, -120]], ["since", 2], [A, [0, -120], [0, -130], True], [E, [0, -90]], ["since", 0],
         [E, [0, -95]], [E, [0, -95]], ["since", 2], [A, [0, -95], [0, -95], True], [E, [0, -95]], [A, [0, -95], [0, -95], False], [A, [0, -95], [0, -94], True]]),
    # a step score equal to the best counts as not improved
    _sc("equal_is_not_improved", {"since_max": 2}, 2, 1, [[P, [-100]], [E, [-100]], ["since", 1], [E, [-100]], ["since", 2], [A, [-100], [-100], False]]),
]


def all_scripts():
    return goldens() + EDGE_SCRIPTS


# ---- a script as sf_debug_acceptor_script runs it ----------------------------------------------------------------------------------
OP_PHASE_STARTED, OP_DECIDE, OP_STEP_ENDED = 0, 1, 2
NOT_DOABLE_LANES = (7, 40)  # candidates that never reach the acceptor: their ballot bit must stay 0


def candidates(cur, sc, threshold, levels):
    """64 trial scores for one decide record: lane 0 is the script's own candidate, the rest straddle the last step score and the
    threshold (one level moved by -3..3 at a time), clamped to i64."""
    out = [tuple(sc)]
    for d in (0, -1, 1, -2, 2, -3, 3):
        for base in (threshold, cur, sc):
            for k in range(levels - 1, -1, -1):
                c = list(base)
                c[k] = min(max(c[k] + d, I64_MIN), I64_MAX)
                if len(out) < 64:
                    out.append(tuple(c))
    while len(out) < 64:
        out.append(tuple(cur))
    return out


def device_plan(script):
    """The records of a script and what the mirror says of each: a list of dicts {op, cur, sc (64 tuples) or None, doable (u64 mask),
    accept (expected u64 ballot), state (level[4], increment[4], since)}.  `since` and `phase_ended` ops have no record: the device has no
    phase end (a phase start rewrites every word), and the state after every record is compared anyway."""
    a = make(script)
    levels = script["levels"]
    doable = (1 << 64) - 1
    for lane in NOT_DOABLE_LANES:
        doable &= ~(1 << lane)
    pad = lambda t: tuple(t) + (0,) * (4 - len(t))
    plan = []
    for op in script["ops"]:
        rec = None
        if op[0] == "phase_started":
            a.phase_started(op[1])
            rec = {"op": OP_PHASE_STARTED, "cur": pad(op[1]), "sc": None, "doable": 0, "accept": 0}
        elif op[0] == "is_accepted":
            cur = tuple(op[1])
            thr = a.water if script["acceptor"] == "great_deluge" else cur
            sc = candidates(cur, tuple(op[2]), thr, levels)
            ballot = 0
            for lane, c in enumerate(sc):
                if (doable >> lane) & 1 and a.is_accepted(cur, c):
                    ballot |= 1 << lane
            assert bool(ballot & 1) == op[3]
            rec = {"op": OP_DECIDE, "cur": pad(cur), "sc": [pad(c) for c in sc], "doable": doable, "accept": ballot}
        elif op[0] == "step_ended":
            a.step_ended(op[1])
            rec = {"op": OP_STEP_ENDED, "cur": pad(op[1]), "sc": None, "doable": 0, "accept": 0}
        elif op[0] == "phase_ended":
            a.phase_ended()
        if rec is not None:
            level, incr, since = a.state()
            rec["state"] = (pad(level), pad(incr), since)
            plan.append(rec)
    return plan
