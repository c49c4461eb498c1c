"""The Variable Neighborhood Descent phase restated over an oracle Model (test infrastructure; the oracle itself cannot run the phase).

Source: crates/solverforge-solver/src/phase/localsearch/vnd/phase.rs:31-167 (solve_vnd_with_resources) and :181-404
(find_best_improving_move); the neighbourhoods are compiled with SelectionOrder::Original (runtime/compiler/local_search.rs:55-89).

    k = 0, current = the score at phase start; while k < n (and below the step limit):
        draw the step seed (one u64, whatever the order), open the cursor of neighbourhood k alone, pull it to its end
        a candidate that is not doable is released (a requires_*_improvement gate would release it too; no leaf admitted here has one)
        every other candidate is scored; kept when score > current AND score > the kept one's, both strictly: the first of equal bests stays
        found:     apply, current = its score, update the best solution, count the step, k = 0
        not found: count the step, k += 1 -- a step that applies nothing is still a step: step index and seed draw advance
    counters: generated / evaluated per pull as in local search (evaluate_candidate / record_evaluated_move); moves_accepted and
    moves_applied count the applied pick only, once per found step (phase.rs:117-127)."""
import json
import os

ORDER_ORIGINAL = 0
COUNTERS = ["step_count", "moves_generated", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations", "moves_not_doable"]


def golden_file():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vnd_goldens.json")) as f:
        return json.load(f)


def accepts(score, current):
    """vnd_accepts: strictly better than the current score (phase.rs:339)."""
    return tuple(score) > tuple(current)


def pick(scores, doable, current):
    """find_best_improving_move's choice over one cursor: the index of the first strictly best strictly improving candidate, or None.
    scores: one tuple per pull; doable: one truth value per pull."""
    best, best_score = None, None
    for i, (sc, ok) in enumerate(zip(scores, doable)):
        if not ok:
            continue
        sc = tuple(sc)
        if accepts(sc, current) and (best is None or sc > best_score):
            best, best_score = i, sc
    return best


def run_scores(neighborhoods, initial, step_limit=None):
    """The phase over neighbourhoods given as data: each a list of (doable, score) whose move sets the solution's score to `score`
    (the reference's own test double, vnd/tests.rs:97-118).  Returns (final score, picks per step)."""
    current, k, picks = (initial,), 0, []
    while k < len(neighborhoods) and (step_limit is None or len(picks) < step_limit):
        hood = neighborhoods[k]
        sel = pick([(s,) for _, s in hood], [d for d, _ in hood], current)
        picks.append(sel)
        if sel is None:
            k += 1
        else:
            current, k = (hood[sel][1],), 0
    return current[0], picks


class VndPhase:
    """The phase over an oracle Model.  leaves: the neighbourhoods as oracle leaf bits in order; seed_of_step(step_index) -> the step
    seed (the solver's draw).  step() runs one step and returns its record."""

    def __init__(self, model, leaves, seed_of_step, levels=2):
        self.m, self.leaves, self.seed_of_step, self.levels = model, list(leaves), seed_of_step, levels
        self.k, self.step_index, self.idle_steps = 0, 0, 0
        self.current = self._score()
        self.best_score = self.current
        self.stats = dict.fromkeys(COUNTERS, 0)

    def _score(self):
        return tuple(int(x) for x in self.m.score()[:self.levels])

    @property
    def n(self):
        return len(self.leaves)

    @property
    def done(self):
        return self.k >= self.n

    def state(self):
        return {"k": self.k, "n": self.n, "done": self.done, "idle_steps": self.idle_steps}

    def step(self):
        assert not self.done
        k = self.k
        moves = self.m.enumerate(self.leaves[k], self.step_index, self.seed_of_step(self.step_index), ORDER_ORIGINAL)
        sc, dv = self.m.evaluate_moves(moves)
        scores = [tuple(int(x) for x in row[:self.levels]) for row in sc]
        doable = [bool(x) for x in dv]
        sel = pick(scores, doable, self.current)
        n_doable = sum(doable)
        best = [s for s, ok in zip(scores, doable) if ok and accepts(s, self.current)]
        ties = sum(1 for s in best if s == max(best)) if best else 0
        st = self.stats
        st["step_count"] += 1
        st["moves_generated"] += len(moves)
        st["moves_evaluated"] += len(moves)
        st["score_calculations"] += n_doable
        st["moves_not_doable"] += len(moves) - n_doable
        rec = {"k": k, "step_index": self.step_index, "cursor": len(moves), "not_doable": len(moves) - n_doable, "pick": sel, "ties": ties,
               "last_tie": None, "moves": moves, "scores": scores, "doable": doable}
        if sel is None:
            self.k += 1
            self.idle_steps += 1
        else:
            rec["last_tie"] = max(i for i, (s, ok) in enumerate(zip(scores, doable)) if ok and s == scores[sel])
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

    def run(self, max_steps=10 ** 6):
        out = []
        while not self.done and len(out) < max_steps:
            out.append(self.step())
        return out


def is_local_optimum(model, leaves, levels=2):
    """No strictly improving doable move in any neighbourhood (Original order: the whole neighbourhood)."""
    cur = tuple(int(x) for x in model.score()[:levels])
    for leaf in leaves:
        moves = model.enumerate(leaf, 0, 0, ORDER_ORIGINAL)
        sc, dv = model.evaluate_moves(moves)
        if any(ok and tuple(int(x) for x in row[:levels]) > cur for row, ok in zip(sc, dv)):
            return False
    return True
