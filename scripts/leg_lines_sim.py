"""Distinct cache lines per leg gather of the wave engine's replay batch, simulated on the CPU.  Pure numpy, no device.

The model: datasets.make_cvrp(1000, 100, 55, 0), nodes renumbered by the nearest-neighbour chain from the depot as sf_initialize does it
(so the u16 matrix row of node n lies at byte n x 2 x dim), and a lockstep batch as the kernel builds it: lanes 0 - 31 price 32 consecutive
candidates of the change leaf, lanes 32 - 63 of the swap leaf; a source (a list position) emits its max_nearby = 20 nearest assigned nodes as
destinations in index order, consecutive sources are consecutive positions of one list (then of the next list in a random order), and a
batch starts at a random offset inside its first source's 20 -- so a leaf's 32 lanes come from two or three sources.  A change puts x in front
of its neighbour (the source slot and its successor are skipped), a swap pairs x with the neighbour (an intra-list swap with a LATER position
only).  For each of the eight leg gathers the distinct 64-B (and 128-B) lines over the 64 lanes are counted and summed over the eight; the
union over all eight is the batch's footprint under perfect L1 reuse.

Four forms of the leg table (eval_generated_small):
  today     the table as it stands: p3 / m3 fetched and discarded by change and adjacent-swap lanes
  reaim     SF_SPEC_LEG_REAIM: in those lanes p3 and m3 read m1's address
  sym       SF_SPEC_SYM_ROWS: p1 and p2 addressed by the source-side row (a symmetric matrix)
  reaim+sym both
on two solutions: the round-robin start routes, and geographically tight routes (the chain cut into lists of ten).

usage: leg_lines_sim.py [--batches 300] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solverforge_amd import datasets  # noqa: E402

K = 20
FORMS = ("today", "reaim", "sym", "reaim+sym")


def chain_numbering(mat, depot):
    """perm[node] = internal id: a nearest-neighbour chain from the depot, ties by node id (the presorted index's order)."""
    dim = mat.shape[0]
    order = np.lexsort((np.broadcast_to(np.arange(dim), mat.shape), mat), axis=1)  # per row: by (distance, node)
    perm, seen, cur = np.zeros(dim, dtype=np.int64), np.zeros(dim, dtype=bool), depot
    for n in range(dim):
        perm[cur], seen[cur] = n, True
        if n + 1 == dim:
            break
        cur = next(int(t) for t in order[cur] if not seen[t])
    return perm


def legs(form, chg, adj, pa, x, na, pb, vq, nb):
    """(from, to) of the eight gathers p0 p1 p2 p3 m0 m1 m3 m2 of one lane."""
    ca = chg or adj
    m1 = (x, vq if adj else na)
    p1, p2 = (pb if chg else vq, x if ca else na), (x if ca else pb, vq if chg else (nb if adj else x))
    if "sym" in form:
        p1, p2 = (x if ca else na, pb if chg else vq), (x, vq if chg else (nb if adj else pb))
    p3, m3 = (x, nb), (vq, nb)
    if "reaim" in form and ca:
        p3 = m3 = m1
    return [(pa, na if chg else vq), p1, p2, p3, (pa, x), m1, m3, (vq if adj else pb, nb if adj else vq)]


def batch_lanes(routes, pos_of, nearest, rng):
    """64 lanes (chg, adj, pa, x, na, pb, vq, nb) of one lockstep batch; depot = node 0."""
    lanes = []
    live = [r for r in range(len(routes)) if routes[r]]
    for chg in (True, False):
        out, r, i, skip = [], int(rng.choice(live)), None, int(rng.integers(0, K))
        i = int(rng.integers(0, len(routes[r])))
        while len(out) < 32:
            la, rt = len(routes[r]), routes[r]
            x, pa, na = rt[i], (rt[i - 1] if i > 0 else 0), (rt[i + 1] if i + 1 < la else 0)
            emitted = 0
            for y in nearest[x]:
                if emitted == K:
                    break
                b, j = pos_of[y]
                if b < 0:
                    continue
                intra = b == r
                if chg and intra and (j == i or j == i + 1):
                    continue
                if not chg and intra and j <= i:
                    continue
                emitted += 1
                if skip:
                    skip -= 1
                    continue
                lb, rb = len(routes[b]), routes[b]
                pb, nb = (rb[j - 1] if j > 0 else 0), (rb[j + 1] if j + 1 < lb else 0)
                out.append((chg, (not chg) and intra and j == i + 1, pa, x, na, pb, y, nb))
                if len(out) == 32:
                    break
            i += 1
            if i >= la:
                r, i = int(rng.choice(live)), 0
        lanes += out
    return lanes


def simulate(routes, nearest, dim, batches, seed):
    pos_of = {n: (-1, -1) for n in range(dim)}
    for r, rt in enumerate(routes):
        for j, n in enumerate(rt):
            pos_of[n] = (r, j)
    rng = np.random.default_rng(seed)
    forms = FORMS
    acc = {(f, line): [0.0, 0.0] for f in forms for line in (64, 128)}
    for _ in range(batches):
        lanes = batch_lanes(routes, pos_of, nearest, rng)
        for f in forms:
            addr = np.array([[(a * dim + b) * 2 for a, b in legs(f, *ln)] for ln in lanes])  # [64 lanes, 8 gathers]
            for line in (64, 128):
                acc[(f, line)][0] += sum(len(np.unique(addr[:, g] // line)) for g in range(8))
                acc[(f, line)][1] += len(np.unique(addr // line))
    return {k: (v[0] / batches, v[1] / batches) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    p = datasets.make_cvrp(1000, 100, 55, 0)
    mat, dim = p["matrix"], p["matrix"].shape[0]
    perm = chain_numbering(mat, p["depot"])
    inv = np.argsort(perm)
    m = mat[np.ix_(inv, inv)]  # the matrix under the internal numbering; the depot is node 0
    nearest = [[int(t) for t in row if t != n and t != 0] for n, row in enumerate(np.lexsort((np.broadcast_to(np.arange(dim), m.shape), m), axis=1))]
    solutions = {"round-robin routes": [[int(perm[c]) for c in rt] for rt in p["routes"]],
                 "geographically tight routes": [list(range(1 + 10 * v, 11 + 10 * v)) for v in range(100)]}
    print(f"distinct lines per batch of 64 lanes, mean of {args.batches} batches (seed {args.seed}); sum over the eight leg gathers | union over the eight")
    for name, routes in solutions.items():
        res = simulate(routes, nearest, dim, args.batches, args.seed)
        print(name)
        for line in (64, 128):
            base = res[("today", line)][0]
            for f in FORMS:
                s, u = res[(f, line)]
                print(f"  {line:3d}-B lines  {f:10s} {s:6.1f} ({100 * (s / base - 1):+5.1f} %) | {u:6.1f}")


if __name__ == "__main__":
    main()
