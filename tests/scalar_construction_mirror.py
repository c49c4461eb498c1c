"""A short restatement of the reference's scalar ConstructionHeuristicPhase, driven by the oracle's own primitives.

What it restates (paths under crates/solverforge-solver/src/phase/construction/):
  runtime_slots/placement.rs:73-147,174-227,307-368   heuristic -> entity order, value order, forager, live refresh; the placement cursor
  forager_step.rs:149-332,463-625, decision.rs:50-154 first fit, best fit, weakest / strongest fit and the keep-current baseline
  phase/selection.rs:14-86, frontier.rs:32-50         commit, and "completed" = kept or assigned at the CURRENT solution revision
  phase/phase_type.rs:74-149                          the phase loop: one step per placement

`model` is anything with the oracle Model's `get_vars(desc, var)`, `score()`, `evaluate_moves(records)` -> (scores, doable) and
`apply_move(record)`; records are (kind, a, a_pos, b, b_pos, value) with kind 0 = Change.  The cursor is restated LITERALLY -- with live
refresh every placement re-walks the order from its head and consults the frontier -- so that it is an independent check of the device
kernel's kept-list formulation."""

FIRST_FIT, FIRST_FIT_DECREASING, WEAKEST_FIT, WEAKEST_FIT_DECREASING, STRONGEST_FIT, STRONGEST_FIT_DECREASING = 0, 1, 2, 3, 4, 5
CHEAPEST_INSERTION, ALLOCATE_ENTITY_FROM_QUEUE, ALLOCATE_TO_VALUE_FROM_QUEUE = 6, 7, 8
HEURISTICS = tuple(range(9))
PRESERVE_UNASSIGNED, ASSIGN_WHEN_CANDIDATE_EXISTS = 0, 1

_DESCENDING = (FIRST_FIT_DECREASING, WEAKEST_FIT_DECREASING, STRONGEST_FIT_DECREASING)
_WEAKEST = (WEAKEST_FIT, WEAKEST_FIT_DECREASING)
_STRONGEST = (STRONGEST_FIT, STRONGEST_FIT_DECREASING)
LIVE_REFRESH = tuple(h for h in HEURISTICS if h not in (FIRST_FIT, CHEAPEST_INSERTION))  # requires_live_refresh
NEEDS_ENTITY_KEYS = _DESCENDING + (ALLOCATE_ENTITY_FROM_QUEUE,)
NEEDS_VALUE_KEYS = _WEAKEST + _STRONGEST + (ALLOCATE_TO_VALUE_FROM_QUEUE,)


def _score(row):
    return tuple(int(x) for x in row)


def construct(model, heuristic, obligation=PRESERVE_UNASSIGNED, allows_unassigned=True, n_values=None, value_lists=None,
              value_candidate_limit=0, entity_order_keys=None, value_order_keys=None, desc=0, var=0):
    """Runs the phase on `model` (which is left constructed).  Returns the counters the reference records plus `kept` (placements that kept
    current), `assigned_on_retry` (entities that kept current at least once and were assigned by a later placement), `placements` (the
    entity of every placement, in order) and `candidates` (how many candidate values each placement offered)."""
    st = dict(step_count=0, moves_generated=0, moves_evaluated=0, moves_accepted=0, moves_applied=0, score_calculations=0, moves_not_doable=0,
              kept=0, assigned_on_retry=0, placements=[], candidates=[])
    vals = [int(v) for v in model.get_vars(desc, var)]
    n = len(vals)
    order = list(range(n))
    if heuristic in _DESCENDING:  # sort_by is stable; ties by index
        order.sort(key=lambda e: (-int(entity_order_keys[e]), e))
    elif heuristic == ALLOCATE_ENTITY_FROM_QUEUE:
        order.sort(key=lambda e: (int(entity_order_keys[e]), e))
    baseline_on = bool(allows_unassigned) and obligation == PRESERVE_UNASSIGNED  # keep_current_allowed
    live = heuristic in LIVE_REFRESH

    def values_of(e):
        vs = list(value_lists[e]) if value_lists is not None else list(range(n_values))
        if value_candidate_limit:
            vs = vs[:value_candidate_limit]  # visit_candidate_values: the cut comes before the value order
        if heuristic == ALLOCATE_TO_VALUE_FROM_QUEUE:
            vs = [v for _, v in sorted(enumerate(vs), key=lambda kv: (int(value_order_keys[kv[1]]), kv[0]))]
        return vs

    revision, completed, kept_once = 1, {}, set()
    i = 0
    while True:
        if live:
            i = 0
        placement = None
        while i < n:
            e = order[i]
            i += 1
            if vals[e] >= 0:
                continue
            vs = values_of(e)
            if not vs:
                continue
            if completed.get(e) == revision:
                continue
            placement = (e, vs)
            break
        if placement is None:
            break
        e, vs = placement
        st["placements"].append(e)
        st["candidates"].append(len(vs))
        records = [(0, e, 0, 0, 0, v) for v in vs]
        scores, doable = model.evaluate_moves(records)  # the state does not change inside a placement: one batch, read in pull order
        baseline = _score(model.score()) if baseline_on else None
        chosen = None

        def pulled(k):
            st["moves_generated"] += 1
            st["moves_evaluated"] += 1
            if not doable[k]:
                st["moves_not_doable"] += 1
            return bool(doable[k])

        if heuristic in _WEAKEST + _STRONGEST:
            retained = None
            for k, v in enumerate(vs):
                if not pulled(k):
                    continue
                s = int(value_order_keys[v])
                if retained is None or (s < retained[1] if heuristic in _WEAKEST else s > retained[1]):
                    retained = (k, s)
            if retained is not None:
                if baseline is None:
                    chosen = retained[0]
                else:
                    st["score_calculations"] += 1
                    if _score(scores[retained[0]]) > baseline:
                        chosen = retained[0]
        elif heuristic == CHEAPEST_INSERTION:
            best = None
            for k in range(len(vs)):
                if not pulled(k):
                    continue
                st["score_calculations"] += 1
                s = _score(scores[k])
                if best is None or s > best[1]:
                    best = (k, s)
            if best is not None and not (baseline is not None and baseline > best[1]):
                chosen = best[0]
        else:  # the first-fit forager
            for k in range(len(vs)):
                if not pulled(k):
                    continue
                if baseline is None:
                    chosen = k
                    break
                st["score_calculations"] += 1
                if _score(scores[k]) > baseline:
                    chosen = k
                    break
        st["step_count"] += 1
        if chosen is not None:
            model.apply_move(records[chosen])
            vals[e] = vs[chosen]
            st["moves_accepted"] += 1
            st["moves_applied"] += 1
            revision += 1
            if e in kept_once:
                st["assigned_on_retry"] += 1
        else:
            # should_mark_completion: every keep-current this surface can reach is marked (a nullable variable under either obligation)
            assert allows_unassigned, "a required variable with candidates always selects one"
            completed[e] = revision
            kept_once.add(e)
            st["kept"] += 1
    return st
