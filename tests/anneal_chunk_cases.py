"""Scripted chunk sequences for the SimulatedAnnealing acceptor: the inputs of tests/test_anneal_chunk_cases.py (oracle alone, CPU)
and tests/test_gpu_anneal_chunks.py (sf_debug_anneal_chunks against the oracle).

A search engine decides 64 candidates of the pull order at once (sa_decide) and then commits the acceptor state by the candidates
the forager consumed (sa_commit).  A sequence scripts both choices, which a search never lets a test make: which lane completes the
calibration and where the chunk is cut.  One chunk = (cur, 64 lanes, nconsumed, step_end); a lane is None (no doable candidate) or
its trial score.

The reference is the oracle's acceptor (oracle/sfo_search.hpp, sfo.Annealer).  replay_oracle() feeds it the doable lanes below
nconsumed of each chunk in lane order and step_ended where the chunk says so; lanes at or after nconsumed are speculative on the
device and are not compared.

The tie rule.  The device's exp() may differ from glibc's by one ulp, so a draw with |u - probability| <= TIE_ULPS *
spacing(probability) is undecidable.  No sequence may contain such a draw (assert_no_ties; a seed that produces one is changed,
the rule is not relaxed): it bounds the inputs, it is no tolerance on the kernel, every compared flag must be equal.

Every sequence states the edge it exists for in `expect`; check_expectations() proves on the oracle alone that it gets there."""
import numpy as np

from solverforge_amd import datasets
from solverforge_amd._lib import ANNEAL_CHUNK_DTYPE

TIE_ULPS = 4  # the documented 1-ulp bound of exp() with a margin for the final compare
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
HC = 1.0e-9  # the reference's DEFAULT_HILL_CLIMBING_TEMPERATURE


class Sequence:
    def __init__(self, name, params, chunks, expect):
        self.name, self.params, self.chunks, self.expect = name, params, chunks, expect
        self.levels, self.hard_levels = params["levels"], params["hard_levels"]

    def __repr__(self):
        return self.name

    def device_kwargs(self):
        """The arguments of GpuScoreDirector.debug_anneal_chunks."""
        p = self.params
        return dict(levels=p["levels"], hard_levels=p["hard_levels"], mode=p["mode"], temperatures=p["temperatures"],
                    decay_rate=p["decay_rate"], hill_climbing_temperature=p["hill_climbing_temperature"],
                    never_accept_hard_regression=p["never_accept_hard"], calibration_sample_size=p["sample_size"],
                    target_acceptance_probability=p["target_probability"], fallback_temperature=p["fallback_temperature"],
                    seed=p["seed"])


class _Builder:
    def __init__(self, name, levels=2, hard_levels=1, **params):
        self.name = name
        self.params = dict(mode=2, temperatures=(), levels=levels, hard_levels=hard_levels, decay_rate=0.999985,
                           hill_climbing_temperature=HC, never_accept_hard=False, sample_size=128, target_probability=0.80,
                           fallback_temperature=1.0, seed=0)
        assert set(params) <= set(self.params), params
        self.params.update(params)
        self.rows = []

    def chunk(self, cur, lanes, nconsumed=64, step_end=False):
        assert len(lanes) == 64 and 0 <= nconsumed <= 64
        row = np.zeros((), dtype=ANNEAL_CHUNK_DTYPE)
        L = self.params["levels"]
        row["cur"][:L] = cur  # numpy refuses a value outside int64
        mask = 0
        for l, sc in enumerate(lanes):
            if sc is not None:
                row["sc"][l][:L] = sc
                mask |= 1 << l
        row["doable"] = mask
        row["nconsumed"] = nconsumed
        row["step_end"] = int(step_end)
        self.rows.append(row)
        return len(self.rows) - 1

    def done(self, **expect):
        return Sequence(self.name, self.params, np.array(self.rows, dtype=ANNEAL_CHUNK_DTYPE), expect)


# ---- lanes ---------------------------------------------------------------------------------------------------------------------
def _cur(rng, levels, span=10 ** 6):
    return [int(v) for v in rng.integers(-span, span, size=levels)]


def _tail(rng, sc, level, span):
    """Levels after the first differing one move either way: the acceptor must not look at them."""
    for k in range(level + 1, len(sc)):
        if rng.integers(0, 2):
            sc[k] += int(rng.integers(-span, span + 1))
    return sc


def _worse(rng, cur, level, d, span=1000):
    sc = list(cur)
    sc[level] -= int(d)
    return _tail(rng, sc, level, span)


def _better(rng, cur, level, d, span=1000):
    sc = list(cur)
    sc[level] += int(d)
    return _tail(rng, sc, level, span)


def _filler(rng, cur, hard_worse_level=None):
    """A lane that records no sample and draws nothing: not doable, equal, improving, or -- under never_accept_hard -- a hard
    regression."""
    kind = int(rng.integers(0, 4 if hard_worse_level is not None else 3))
    if kind == 0:
        return None
    if kind == 1:
        return list(cur)
    if kind == 2:
        return _better(rng, cur, int(rng.integers(0, len(cur))), int(rng.integers(1, 1000)))
    return _worse(rng, cur, hard_worse_level, int(rng.integers(1, 1000)))


def _mixed_lanes(rng, cur, levels, p_worse=0.5, dmax=1000, first_level=0):
    """64 random lanes: worsening at a random first differing level, else a filler."""
    lanes = []
    for _ in range(64):
        if rng.random() < p_worse:
            lanes.append(_worse(rng, cur, int(rng.integers(first_level, levels)), int(rng.integers(1, dmax + 1))))
        else:
            lanes.append(_filler(rng, cur))
    return lanes


class _Sampler:
    """Chunks whose sample lanes are placed on purpose (calibration sequences)."""

    def __init__(self, b, rng, dmax=1000):
        self.b, self.rng, self.dmax = b, rng, dmax
        p = b.params
        self.levels = p["levels"]
        self.nah = p["never_accept_hard"]
        self.first = p["hard_levels"] if self.nah else 0  # sample levels: first..levels-1
        assert self.first < self.levels

    def sample(self, cur):
        return _worse(self.rng, cur, int(self.rng.integers(self.first, self.levels)), int(self.rng.integers(1, self.dmax + 1)))

    def filler(self, cur):
        return _filler(self.rng, cur, 0 if self.nah and self.first > 0 else None)

    def lanes(self, cur, sample_at):
        sample_at = set(int(x) for x in sample_at)
        return [self.sample(cur) if l in sample_at else self.filler(cur) for l in range(64)]

    def supply(self, n):
        """n samples over as many whole chunks as it takes, at random lanes."""
        while n > 0:
            k = int(min(n, self.rng.integers(1, 65)))
            cur = _cur(self.rng, self.levels)
            self.b.chunk(cur, self.lanes(cur, self.rng.choice(64, size=k, replace=False)), 64, bool(self.rng.integers(0, 2)))
            n -= k

    def after(self, n=2):
        """Ordinary chunks once the temperatures are installed: draws, and cooling between them."""
        for _ in range(n):
            cur = _cur(self.rng, self.levels)
            self.b.chunk(cur, _mixed_lanes(self.rng, cur, self.levels, dmax=self.dmax), 64, True)


# ---- calibration boundary ------------------------------------------------------------------------------------------------------
CALIB_SIZES = (1, 2, 63, 64, 65, 128)
CALIB_LANES = (0, 31, 32, 63)


def _calib_boundary(S, f, kind, levels):
    seed = 1000 + S * 97 + f * 7 + {"exact": 0, "more": 1, "short": 2}[kind] + levels * 1009
    rng = np.random.default_rng(seed)
    nah = levels == 4 and f in (31, 63)
    b = _Builder(f"calib-S{S}-f{f}-{kind}-L{levels}", levels, 1 if levels <= 2 else 2, sample_size=S, seed=seed,
                 never_accept_hard=nah, decay_rate=0.99, target_probability=0.7)
    s = _Sampler(b, rng)
    cur = _cur(rng, levels)
    if kind == "short":  # a chunk with need - 1 samples, then completion at the first sample of the next chunk
        r = min(S, 1 + int(rng.integers(0, 40)))
        s.supply(S - r)
        b.chunk(cur, s.lanes(cur, rng.choice(64, size=r - 1, replace=False)), 64, False)
        cur = _cur(rng, levels)
        at = [f] + [l for l in range(f + 1, 64) if rng.integers(0, 2)]
    else:  # the chunk holds exactly `need` samples, the last at lane f ("more": and further samples behind it)
        m = min(S, 1 + f // 2)
        s.supply(S - m)
        at = [f] + list(rng.choice(f, size=m - 1, replace=False) if m > 1 else [])
        if kind == "more":
            at += [l for l in range(f + 1, 64) if rng.integers(0, 2)]
    c = b.chunk(cur, s.lanes(cur, at), 64, True)
    s.after()
    return b.done(completes=(c, f))


# ---- cut against completion ----------------------------------------------------------------------------------------------------
def _cut(S, f, nc, levels):
    seed = 5000 + S * 131 + f * 11 + nc * 3 + levels * 1009
    rng = np.random.default_rng(seed)
    b = _Builder(f"cut-S{S}-f{f}-n{nc}-L{levels}", levels, 1 if levels <= 2 else 2, sample_size=S, seed=seed, decay_rate=0.98)
    s = _Sampler(b, rng)
    m = min(S, 1 + f // 2)
    s.supply(S - m)
    cur = _cur(rng, levels)
    before = sorted(int(x) for x in (rng.choice(f, size=m - 1, replace=False) if m > 1 else []))
    at = before + [f] + [l for l in range(f + 1, 64) if rng.integers(0, 2)]
    c = b.chunk(cur, s.lanes(cur, at), nc, True)  # a cut chunk ends the step, as in the engines
    if nc > f:
        done = (c, f)
    else:  # the computed temperatures must not be installed; the next chunk completes from the advanced sample count
        left = m - sum(1 for l in before if l < nc)
        cur = _cur(rng, levels)
        at = sorted(int(x) for x in rng.choice(64, size=max(left, 20), replace=False))
        c2 = b.chunk(cur, s.lanes(cur, at), 64, True)
        done = (c2, at[left - 1])
    s.after()
    return b.done(completes=done, seen_after={c: None} if nc > f else {c: S - m + sum(1 for l in before if l < nc)})


# ---- magnitudes ----------------------------------------------------------------------------------------------------------------
def _exact_total(name, total, n_samples, levels, level, seed, per_chunk=64):
    """Calibration whose level-`level` total is exactly `total` (>= 2^64) from n_samples samples below 2^63."""
    rng = np.random.default_rng(seed)
    b = _Builder(name, levels, 1 if levels <= 2 else 2, sample_size=n_samples, seed=seed, decay_rate=0.97)
    parts, left = [], total
    for i in range(n_samples - 1):  # random parts near total / n, the last one takes the rest
        v = left // (n_samples - i)
        v = int(v) - int(rng.integers(0, max(1, min(v // 4, 1 << 40))))
        parts.append(v)
        left -= v
    parts.append(left)
    assert sum(parts) == total and all(0 < v <= INT64_MAX for v in parts)
    c = 0
    for i in range(0, n_samples, per_chunk):
        cur = [0] * levels
        cur[level] = int(rng.integers(0, 1 << 61))
        lanes = [None] * 64
        for j, v in enumerate(parts[i:i + per_chunk]):  # every other lane, so ranks are not lane numbers
            lanes[(2 * j) % 64 + (2 * j) // 64] = _tail(rng, [cur[k] - (v if k == level else 0) for k in range(levels)], level, 1 << 50)
        c = b.chunk(cur, lanes, 64, False)
    for _ in range(3):  # draws at that temperature: (double)delta / T with 62-bit deltas
        cur = [0] * levels
        cur[level] = int(rng.integers(0, 1 << 61))
        lanes = [[cur[k] - (int(rng.integers(1 << 55, 1 << 62)) if k == level else 0) for k in range(levels)] if l % 3 else None
                 for l in range(64)]
        b.chunk(cur, lanes, 64, True)
    return b.done(total={level: total}, hi_nonzero=True, draws_min=100, completes=(c, None))


def _magnitudes():
    out = []
    for levels, level in ((2, 1), (4, 3), (3, 2), (4, 0)):
        tag = f"L{levels}k{level}"
        out.append(_exact_total(f"total-2^64+2^11-tie-to-even-{tag}", (1 << 64) + (1 << 11), 5, levels, level, 71 + levels))
        out.append(_exact_total(f"total-2^64+2^11+1-sticky-{tag}", (1 << 64) + (1 << 11) + 1, 5, levels, level, 72 + levels))
        out.append(_exact_total(f"total-2^64+3*2^11-tie-up-{tag}", (1 << 64) + 3 * (1 << 11), 6, levels, level, 73 + levels))
        out.append(_exact_total(f"total-2^64-exact-{tag}", 1 << 64, 4, levels, level, 74 + levels))
    rng = np.random.default_rng(75)
    for levels, level in ((2, 1), (4, 2)):
        total = (1 << 70) + int(rng.integers(0, 1 << 62)) | 1
        out.append(_exact_total(f"total-about-2^70-L{levels}k{level}", total, 300, levels, level, 76 + levels))
        out.append(_exact_total(f"total-about-2^66-L{levels}k{level}", (1 << 66) + int(rng.integers(0, 1 << 62)) | 1, 23, levels, level, 78 + levels))
    # +-2^62, INT64_MIN and wrapped deltas: as samples of a calibration and then under the installed temperature
    for levels, level in ((2, 1), (2, 0), (4, 3), (4, 1)):
        rng = np.random.default_rng(80 + levels * 4 + level)
        b = _Builder(f"delta-edges-L{levels}k{level}", levels, 1 if levels <= 2 else 2, sample_size=6, seed=80 + level, decay_rate=0.9)

        def at(cur_v, sc_v, tail=True):
            cur = [0] * levels
            sc = [0] * levels
            cur[level], sc[level] = cur_v, sc_v
            return cur, (_tail(rng, sc, level, 1 << 40) if tail else sc)

        cur, _ = at(1 << 62, 0)
        lanes = [None] * 64
        lanes[0] = at(1 << 62, (1 << 62) + INT64_MIN)[1]       # delta == INT64_MIN exactly: the sample saturates to INT64_MAX
        lanes[1] = at(1 << 62, INT64_MIN)[1]                    # true difference -(2^63 + 2^62): wraps to +2^62, no sample
        lanes[2] = at(1 << 62, 0)[1]                            # -2^62
        lanes[3] = at(1 << 62, INT64_MAX)[1]                    # improving by 2^62 - 1 + ... (no sample)
        lanes[5] = at(1 << 62, -(1 << 62) - 5)[1]               # -(2^63 + 5) wraps to +2^63 - 5, no sample
        lanes[9] = at(1 << 62, (1 << 62) - 1)[1]                # -1
        lanes[63] = at(1 << 62, (1 << 62) + INT64_MIN + 1)[1]   # -(2^63 - 1)
        b.chunk(cur, lanes, 64, True)
        cur, _ = at(-(1 << 61), 0)
        lanes = [None] * 64
        lanes[7] = at(-(1 << 61), -(1 << 61) - (1 << 62))[1]    # -2^62 from a negative score
        lanes[8] = at(-(1 << 61), INT64_MAX)[1]                 # improving, the difference wraps negative: accepted, no sample
        lanes[40] = at(-(1 << 61), INT64_MIN)[1]                # -(2^63 - 2^61): completes (6th sample)
        lanes[41] = at(-(1 << 61), INT64_MIN + 1)[1]            # draws under the installed temperature
        lanes[42] = at(-(1 << 61), -(1 << 61) - (1 << 62))[1]
        c = b.chunk(cur, lanes, 64, True)
        for _ in range(4):  # the same edges as candidates of the Boltzmann test
            cur, _ = at(1 << 62, 0)
            lanes = [None] * 64
            for l in range(64):
                pick = l % 8
                v = [(1 << 62) + INT64_MIN, INT64_MIN, 0, -(1 << 62) - 5, (1 << 62) - int(rng.integers(1, 1 << 60)),
                     int(rng.integers(-(1 << 62), 1 << 62)), INT64_MAX, None][pick]
                lanes[l] = None if v is None else at(1 << 62, v)[1]
            b.chunk(cur, lanes, 64, True)
        out.append(b.done(completes=(c, 40), sample_int64_max=True, hi_nonzero=True, draws_min=60, wrapped_rejected=True))
    return out


# ---- temperatures --------------------------------------------------------------------------------------------------------------
def _temperatures():
    out = []
    up = float(np.nextafter(HC, 1.0))
    for levels in (2, 4):
        hard = 1 if levels <= 2 else 2
        for tag, mode, temps, hc, draws in (("single-at-floor", 0, (HC,), HC, False), ("single-ulp-above-floor", 0, (up,), HC, True),
                                            ("single-zero", 0, (0.0,), HC, False), ("single-zero-floor-zero", 0, (0.0,), 0.0, False),
                                            ("single-denormal-floor-zero", 0, (5e-324,), 0.0, True)):
            rng = np.random.default_rng(200 + levels + len(tag))
            b = _Builder(f"temp-{tag}-L{levels}", levels, hard, mode=mode, temperatures=temps, hill_climbing_temperature=hc,
                         seed=200 + levels, decay_rate=1.0)
            for i in range(4):
                cur = _cur(rng, levels)
                b.chunk(cur, _mixed_lanes(rng, cur, levels), 64 if i != 2 else 17, True)
            out.append(b.done(draws_min=40, prob_zero=True) if draws else b.done(no_draws=True))
        # per level: at the floor, one ulp above it, 0, and an ordinary one; every level meets draws or their absence
        temps = ((HC, 50.0), (up, HC), (0.0, up)) if levels == 2 else ((HC, up, 0.0, 50.0), (50.0, 0.0, HC, up), (up, 50.0, up, 0.0))
        for i, t in enumerate(temps):
            rng = np.random.default_rng(230 + levels * 4 + i)
            b = _Builder(f"temp-per-level-{i}-L{levels}", levels, hard, mode=1, temperatures=t, seed=230 + i, decay_rate=1.0)
            for _ in range(5):
                cur = _cur(rng, levels)
                b.chunk(cur, _mixed_lanes(rng, cur, levels, dmax=100), 64, True)
            out.append(b.done(draws_min=30, draw_levels=sorted(k for k in range(levels) if t[k] > HC)))
        # cooling that reaches the floor inside the sequence: 3 -> 1.5 -> 0.75 -> floor 0.4 (0.375 is below it), then no draw
        rng = np.random.default_rng(260 + levels)
        b = _Builder(f"temp-decay-to-floor-L{levels}", levels, hard, mode=0, temperatures=(3.0,), decay_rate=0.5,
                     hill_climbing_temperature=0.4, seed=260 + levels)
        for _ in range(7):
            cur = _cur(rng, levels)
            b.chunk(cur, _mixed_lanes(rng, cur, levels, dmax=6), 64, True)
        out.append(b.done(draws_min=60, floor_reached=True, rng_still_after=4))
        # a calibration that leaves levels without samples: they take the fallback temperature (2.5, and 0)
        for fb in (2.5, 0.0):
            rng = np.random.default_rng(270 + levels + int(fb))
            b = _Builder(f"temp-empty-level-fallback-{fb}-L{levels}", levels, hard, sample_size=50, fallback_temperature=fb,
                         seed=270 + levels, decay_rate=0.999)
            s = _Sampler(b, rng)
            s.first = levels - 1  # samples at the last level only
            s.supply(49)
            cur = _cur(rng, levels)
            c = b.chunk(cur, s.lanes(cur, [12, 30]), 64, True)
            for i in range(8):  # small deltas meet the fallback temperature, large ones the calibrated one
                cur = _cur(rng, levels)
                b.chunk(cur, _mixed_lanes(rng, cur, levels, dmax=3000 if i % 2 else 8), 64, True)
            out.append(b.done(completes=(c, 12), empty_levels=list(range(levels - 1)), installed={k: fb for k in range(levels - 1)},
                              draws_min=40, draw_levels=list(range(levels)) if fb > 0 else [levels - 1]))
        # a calibration whose temperatures end at or below the floor: the completing lane and all after it draw nothing
        rng = np.random.default_rng(290 + levels)
        b = _Builder(f"temp-calibrated-below-floor-L{levels}", levels, hard, sample_size=30, fallback_temperature=0.0,
                     hill_climbing_temperature=1.0e6, seed=290 + levels)
        s = _Sampler(b, rng)
        s.supply(25)
        cur = _cur(rng, levels)
        at = sorted(int(x) for x in rng.choice(64, size=20, replace=False))
        c = b.chunk(cur, s.lanes(cur, at), 64, True)
        s.after()
        out.append(b.done(completes=(c, at[4]), no_draws=True))
    # delta / T from -1e-6 to below -745: probabilities from near 1 through the denormal range to exactly 0.  Level 0 at T = 1e6,
    # level 1 at T = 1.  Above p = 2^-53 (delta / T > -36.7) a draw can fall on either side; below it only u == 0 accepts.
    rng = np.random.default_rng(300)
    b = _Builder("temp-exp-sweep-L2", 2, 1, mode=1, temperatures=(1.0e6, 1.0), seed=300, decay_rate=1.0)
    fine = [1, 2, 3, 5, 8, 13, 21, 30, 36, 37, 38, 50, 100, 300, 600, 700, 708, 709, 710, 720, 730, 740, 744, 745, 746, 750, 1000, 10 ** 6,
            1 << 53, (1 << 53) + 1, 1 << 62]
    for rep in range(12):
        cur = _cur(rng, 2, span=1 << 40)
        lanes = []
        for l in range(64):
            if l % 2 == 0:  # level 0: -1e-6 .. -1e3 in steps a reader can follow, then random
                d = [1, 10, 1000, 10 ** 6, 10 ** 7, 10 ** 9][l // 2 % 6] if rep < 2 else int(rng.integers(1, 4 * 10 ** 7))
                lanes.append(_worse(rng, cur, 0, d))
            else:
                d = fine[(l // 2 + rep * 32) % len(fine)] if rep < 4 else int(rng.integers(1, 40))
                lanes.append([cur[0], cur[1] - d])
        b.chunk(cur, lanes, 64, True)
    out.append(b.done(draws_min=700, prob_zero=True, prob_denormal=True, prob_near_one=True, draw_levels=[0, 1]))
    return out


# ---- levels --------------------------------------------------------------------------------------------------------------------
def _levels():
    out = []
    for levels in (1, 2, 3, 4):
        for hard in range(levels + 1):
            for nah in (False, True):
                for mode in (1, 2):
                    if mode == 2 and nah and hard == levels:
                        continue  # every regression is a hard one: nothing is ever sampled, the calibration never ends
                    seed = 400 + levels * 50 + hard * 10 + nah * 2 + mode
                    rng = np.random.default_rng(seed)
                    b = _Builder(f"levels-L{levels}-H{hard}-{'never-hard' if nah else 'any'}-{'per-level' if mode == 1 else 'calibrated'}",
                                 levels, hard, mode=mode, temperatures=(40.0, 90.0, 200.0, 450.0)[:levels] if mode == 1 else (),
                                 never_accept_hard=nah, sample_size=40, seed=seed, decay_rate=0.95)
                    for i in range(12):
                        cur = _cur(rng, levels)
                        nc = 64 if i % 3 else int(rng.integers(0, 65))
                        b.chunk(cur, _mixed_lanes(rng, cur, levels, p_worse=0.7, dmax=400), nc, nc < 64 or bool(rng.integers(0, 2)))
                    want = [k for k in range(levels) if not (nah and k < hard)]
                    out.append(b.done(draw_levels=want, draws_min=20 if want else 0, no_draws=not want))
    return out


# ---- long mixed runs -----------------------------------------------------------------------------------------------------------
def _long(levels, n_chunks, seed):
    rng = np.random.default_rng(seed)
    r = datasets.stream(seed, n_chunks)  # cuts and step ends from the project's own stream
    b = _Builder(f"long-mixed-L{levels}", levels, 1 if levels <= 2 else 2, sample_size=128, seed=seed, decay_rate=0.9995)
    for i in range(n_chunks):
        cur = _cur(rng, levels)
        cut = int(r[i] % np.uint64(4)) == 0
        nc = int((r[i] >> np.uint64(8)) % np.uint64(65)) if cut else 64
        b.chunk(cur, _mixed_lanes(rng, cur, levels, p_worse=float(rng.random()), dmax=3000), nc,
                nc < 64 or int((r[i] >> np.uint64(20)) % np.uint64(3)) == 0)
    return b.done(draws_min=10000, draw_levels=list(range(levels)))


def _build():
    seqs = []
    for levels in (2, 4):
        for S in CALIB_SIZES:
            for f in CALIB_LANES:
                for kind in ("exact", "more", "short"):
                    seqs.append(_calib_boundary(S, f, kind, levels))
    seqs.append(_calib_boundary(64, 32, "more", 3))
    seqs.append(_calib_boundary(65, 63, "short", 3))
    for levels in (2, 4):
        for S in (5, 64):
            for f in (0, 31, 63):
                for nc in sorted({0, f, f + 1, 64}):
                    seqs.append(_cut(S, f, nc, levels))
    seqs += _magnitudes() + _temperatures() + _levels()
    seqs += [_long(2, 2500, 901), _long(4, 2500, 902)]
    names = [s.name for s in seqs]
    assert len(set(names)) == len(names)
    return seqs


_SEQUENCES = None


def sequences():
    """Every sequence, built once and shared by the tests (treat as read-only)."""
    global _SEQUENCES
    if _SEQUENCES is None:
        _SEQUENCES = _build()
    return _SEQUENCES


# ---- the oracle side -----------------------------------------------------------------------------------------------------------
def _first_level(cur, sc, levels):
    for k in range(levels):
        if cur[k] != sc[k]:
            return k
    return -1


def _u128(st, k):
    return (int(st["total_hi"][k]) << 64) | int(st["total_lo"][k])


class Replay:
    """What the oracle did with one sequence.  Per chunk c: lanes[c] (consumed doable lanes), accepted[c] / drew[c] / u[c] /
    prob[c] (arrays over lanes[c]), after_commit[c] and after_step[c] (sfo.Annealer.state() dicts).  Over the sequence: completes
    (chunk, lane) or None, samples [(level, value)], draw_levels [level per draw], temperatures installed at the completion."""


def replay_oracle(sfo, seq):
    p = seq.params
    a = sfo.Annealer(**p)
    a.phase_started()
    out = Replay()
    out.lanes, out.accepted, out.drew, out.u, out.prob, out.after_commit, out.after_step = [], [], [], [], [], [], []
    out.completes, out.samples, out.draw_levels, out.installed = None, [], [], None
    L = seq.levels
    st = a.state()
    out.initial = st
    for c, ch in enumerate(seq.chunks):
        mask, nc = int(ch["doable"]), int(ch["nconsumed"])
        lanes = [l for l in range(nc) if mask >> l & 1]
        cur = np.zeros(4, dtype=np.int64)
        cur[:L] = ch["cur"][:L]
        mv = np.zeros((len(lanes), 4), dtype=np.int64)
        mv[:, :L] = ch["sc"][lanes, :L] if lanes else 0
        if st["calibrating"]:  # lane by lane: which lane recorded what, and which one completed the calibration
            acc, drew, u, prob = (np.zeros(len(lanes), dtype=t) for t in (bool, bool, np.float64, np.float64))
            for i, l in enumerate(lanes):
                if st["calibrating"]:
                    acc[i], drew[i], u[i], prob[i] = a.is_accepted(cur, mv[i])
                    s2 = a.state()
                    if s2["samples_seen"] != st["samples_seen"]:
                        k = _first_level(cur, mv[i], L)
                        out.samples.append((k, _u128(s2, k) - _u128(st, k)))
                    if not s2["calibrating"]:
                        out.completes = (c, l)
                        out.installed = s2["temperatures"].copy()
                    st = s2
                else:
                    acc[i:], drew[i:], u[i:], prob[i:] = a.is_accepted_many(cur, mv[i:])
                    break
        else:
            acc, drew, u, prob = a.is_accepted_many(cur, mv)
        for i in np.flatnonzero(drew):
            out.draw_levels.append(_first_level(cur, mv[i], L))
        st = a.state()
        out.lanes.append(lanes)
        out.accepted.append(acc)
        out.drew.append(drew)
        out.u.append(u)
        out.prob.append(prob)
        out.after_commit.append(st)
        if ch["step_end"]:
            a.step_ended()
            st = a.state()
        out.after_step.append(st)
    return out


def undecidable_draws(rep):
    """(chunk, lane, u, probability) of every draw within TIE_ULPS spacings of its probability."""
    bad = []
    for c, (lanes, drew, u, prob) in enumerate(zip(rep.lanes, rep.drew, rep.u, rep.prob)):
        tie = drew & (np.abs(u - prob) <= TIE_ULPS * np.spacing(prob))
        bad += [(c, lanes[i], float(u[i]), float(prob[i])) for i in np.flatnonzero(tie)]
    return bad


def check_expectations(seq, rep):
    """Each sequence reaches the edge it is named for (on the oracle alone)."""
    e = dict(seq.expect)
    L = seq.levels
    probs = np.concatenate([p[d] for p, d in zip(rep.prob, rep.drew)]) if rep.prob else np.zeros(0)
    if "completes" in e:
        c, lane = e.pop("completes")
        assert rep.completes is not None and rep.completes[0] == c, (seq.name, rep.completes)
        assert lane is None or rep.completes[1] == lane, (seq.name, rep.completes)
    if "seen_after" in e:
        for c, want in e.pop("seen_after").items():
            st = rep.after_commit[c]
            assert (not st["calibrating"]) if want is None else (st["calibrating"] and st["samples_seen"] == want), (seq.name, c, st)
    if e.pop("hi_nonzero", False):
        assert max(int(st["total_hi"].max()) for st in rep.after_commit) > 0, seq.name
    if "total" in e:
        done = rep.after_commit[rep.completes[0]]
        for k, want in e.pop("total").items():
            assert _u128(done, k) == want, (seq.name, k, _u128(done, k))
    if e.pop("sample_int64_max", False):
        assert any(v == INT64_MAX for _, v in rep.samples), seq.name
    if e.pop("wrapped_rejected", False):  # a lower-comparing score whose wrapped difference is >= 0: rejected without a draw
        seen = 0
        for ch, lanes, acc, drew in zip(seq.chunks, rep.lanes, rep.accepted, rep.drew):
            for i, l in enumerate(lanes):
                cur, sc = [int(v) for v in ch["cur"][:L]], [int(v) for v in ch["sc"][l][:L]]
                k = _first_level(cur, sc, L)
                if sc < cur and sc[k] - cur[k] < INT64_MIN:
                    assert not acc[i] and not drew[i], (seq.name, l)
                    seen += 1
        assert seen >= 4, seq.name
    if "draws_min" in e:
        assert len(probs) >= e.pop("draws_min"), (seq.name, len(probs))
    if e.pop("no_draws", False):
        assert len(probs) == 0, seq.name
        assert all((st["rng"] == rep.initial["rng"]).all() for st in rep.after_step), seq.name
    if "draw_levels" in e:
        assert sorted(set(rep.draw_levels)) == sorted(e.pop("draw_levels")), (seq.name, sorted(set(rep.draw_levels)))
    if e.pop("prob_zero", False):
        assert (probs == 0.0).any(), seq.name
    if e.pop("prob_denormal", False):
        assert ((probs > 0.0) & (probs < np.finfo(np.float64).tiny)).any(), seq.name
    if e.pop("prob_near_one", False):
        assert ((probs > 0.99999) & (probs < 1.0)).any(), seq.name
    if e.pop("floor_reached", False):
        hc = seq.params["hill_climbing_temperature"]
        assert (rep.after_step[-1]["temperatures"][:L] == hc).all() and (rep.after_step[0]["temperatures"][:L] > hc).all(), seq.name
    if "rng_still_after" in e:  # at the floor no draw happens: the rng stops
        c = e.pop("rng_still_after")
        assert (rep.after_step[-1]["rng"] == rep.after_step[c]["rng"]).all() and (rep.after_step[c]["rng"] != rep.initial["rng"]).any(), seq.name
    if "empty_levels" in e:
        done = rep.after_commit[rep.completes[0]]
        for k in e.pop("empty_levels"):
            assert done["count"][k] == 0, (seq.name, k)
    if "installed" in e:
        for k, t in e.pop("installed").items():
            assert rep.installed[k] == t, (seq.name, rep.installed)
    assert not e, (seq.name, "unknown expectation", e)
    # what holds for every sequence: while the oracle calibrates its temperatures are 0.0
    for st in rep.after_step:
        assert not st["calibrating"] or (st["temperatures"] == 0.0).all(), seq.name


# ---- the device side -----------------------------------------------------------------------------------------------------------
W_RNG, W_TEMP, W_CALIBRATING, W_SEEN, W_CNT, W_SUM_LO, W_SUM_HI = 0, 4, 8, 9, 10, 14, 18  # include/solverforge_amd.h


def _compare_words(seq, c, which, w, st, frozen):
    L = seq.levels
    where = (seq.name, c, which)
    assert (w[W_RNG:W_RNG + 4] == st["rng"]).all(), where + ("rng", w[:4], st["rng"])
    assert bool(w[W_CALIBRATING]) == st["calibrating"] and int(w[W_CALIBRATING]) in (0, 1), where + ("calibrating",)
    want_t = st["temperatures"].view(np.uint64).copy()
    want_t[L:] = 0
    assert (w[W_TEMP:W_TEMP + 4] == want_t).all(), where + ("temperatures", w[W_TEMP:W_TEMP + 4].view(np.float64), st["temperatures"])
    # the calibration's counters: the oracle's while it calibrates; once it completes the device stops moving them (the samples of
    # the completing chunk went into the installed temperatures, compared above), so they stay what they last were
    ref = st if st["calibrating"] else frozen
    assert int(w[W_SEEN]) == ref["samples_seen"], where + ("samples_seen", int(w[W_SEEN]), ref["samples_seen"])
    assert (w[W_CNT:W_CNT + 4] == ref["count"]).all(), where + ("count",)
    assert (w[W_SUM_LO:W_SUM_LO + 4] == ref["total_lo"]).all() and (w[W_SUM_HI:W_SUM_HI + 4] == ref["total_hi"]).all(), where + ("total",)


def compare_device(seq, rep, accept, state):
    """accept u64[n], state u64[n, 2, 32] of sf_debug_anneal_chunks against the oracle's replay: every consumed doable lane's
    flag and the whole committed state, chunk by chunk."""
    assert len(accept) == len(seq.chunks) and state.shape[:2] == (len(seq.chunks), 2)
    frozen = rep.initial
    for c in range(len(seq.chunks)):
        got = int(accept[c])
        for i, l in enumerate(rep.lanes[c]):
            assert bool(got >> l & 1) == bool(rep.accepted[c][i]), (seq.name, c, l, "accept flag", rep.drew[c][i], rep.u[c][i], rep.prob[c][i])
        _compare_words(seq, c, "after commit", state[c, 0], rep.after_commit[c], frozen)
        _compare_words(seq, c, "after step end", state[c, 1], rep.after_step[c], frozen)
        if rep.after_step[c]["calibrating"]:
            frozen = rep.after_step[c]
