#!/usr/bin/env python
"""bench.py — moves-evaluated/sec (M1) and best HardSoftScore@60s (M2) of the MI355X hot path on BASELINE.json's
CVRP-1000 workload.

A plain run (`bench.py --gpus 1 --steps N --warmup W`) sets up, warms up, times the N M1 launches, writes the outputs of the last
one when `--dump-outputs DIR` is given, and prints the result line.  Everything else below -- the rocprofv3 counter passes of
the roofline, the CPU baseline, the M2 solve legs and the CVRP-5000 side leg -- runs only with `--full`.

M1.  One bench "step" = ONE persistent-kernel launch (sf_solve_steps) that runs `--ls-steps` local-search steps
(seeded nearby-list candidate generation -> trial delta score -> LateAcceptance -> AcceptedCount(256) forager ->
apply) for each of `--replicas` independently seeded searches resident on the GPU (the per-GPU batch of the seed
portfolio).  `value` counts CONSUMED candidates (`moves_evaluated`, the reference's counter definition,
evaluation.rs:33-49), not the speculative tail; inputs are resident in HBM before the timed region.

roofline.  The dominant kernel (k_list_search_wave) keeps a replica's whole state in LDS, so HBM is idle (DESIGN.md
§4); what bounds it is instruction issue.  `roofline.bound` names the tightest of three issue rooflines — VALU (achieved =
SQ_INSTS_VALU wave-instructions per second, peak = 1024 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction,
MI355X_MICROARCH.md), SALU (one scalar unit per CU, 1 instruction per clock) and LDS — all three are reported.  The counters
come from rocprofv3 --pmc passes of THIS command (same warm-up and timed launches) that bench.py runs as child
processes after the timed region (FETCH_SIZE and WRITE_SIZE each in a pass of their own, the read side doubled as the
guide prescribes for gfx950); when the passes fail `roofline.frac` / `achieved` / `traffic` are null and
`roofline.pmc_source` says why.  SURVEY.md §8(d)'s algorithmic-bytes figure stays as a labelled side number.

cpu_baseline.  The oracle (C++ restatement of the reference algorithm, 1 thread) runs the SAME local-search step window
as GPU replica 0 (same seed), and when it completes the window its working score is compared bit for bit with
replica 0's (`extra.replica0_matches_cpu_oracle`).

M2 (`--solve-seconds`, default 60).  A fresh portfolio solves for 60 s of wall clock with work-balanced launches
(sf_solve_moves) under the reference's DEFAULT LIST POLICY (`--solve-policy default`: the seven leaves of
default_local_search/policy/list.rs on the generic N-leaf engine; `nearby2` = the two-leaf union M1 is timed on) while the CPU
oracle solves the same problem with the same leaves (seed of replica 0) on one host core for the same
60 s: `extra.best_score_at_60s` = {"gpu": ..., "cpu_oracle": ...}.  `--solve-start savings | savings_capacity` starts both
sides from empty routes with the construction phases of the CVRP domain -- Clarke-Wright savings
(sf_construct_list_clarke_wright), then the route-local 2-opt of ListKOptPhase (sf_construct_list_k_opt) -- built inside the
budget; the start score is reported beside the best score.  `savings` is the reference's stock wiring (savings_hooks::feasible
is structural only, crates/solverforge-cvrp/src/helpers.rs:77-87: the merge ends in ONE route, hard score -4869 at this
size, and no 60 s search repairs it); the default `savings_capacity` is an EXTENSION: the same phases with a capacity-checking
`feasible` hook a model may supply (the capacity part of route_hooks::feasible; no time windows are modelled here).

M2, second leg (`--tuned-seconds`, default 60; `extra.best_score_at_60s.tuned`).  An EXTENSION beside the parity leg, labelled as such: the
same problem, start and leaves as M1 (the two-leaf nearby union on the wave engine), but a configuration a user of the reference may set
through the same facade -- LateAcceptance(5000) + AcceptedCount(1), i.e. classic late-acceptance hill climbing at the step rate the device
sustains (the default's best-of-256 forager makes every step a steepest-descent step: its 60 s curve is flat after ~25 s) -- 1,024 replicas,
and elite migration every 5 s (sf_portfolio_migrate_local: the worse half adopts the best solutions of the top eight).  The CPU oracle runs
the same configuration on one host core beside it.  profiles/r04b_m2_config_sweep_*.jsonl hold the sweep this configuration came from.

Multi-GPU.  `python bench.py --gpus N` spawns N ranks itself (torch.distributed.run, one process per GPU) when it is
not already running under a launcher; it refuses to run with fewer devices than ranks.  Independent seeds per rank
(weak scaling, no data-path collective); at the end every rank contributes its best score to one RCCL all-gather over
xGMI (sf_portfolio_allgather_best) and all ranks name the same winner, whose routes one RCCL broadcast hands to every
rank.  torch.distributed (gloo) is used only for rendezvous / barrier / max-over-ranks.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# SURVEY.md §8(d) algorithmic bytes (C3): one scored list-change/list-swap candidate at route length 10+10 = 368 B;
# nearby generation per source = (N+V)*12 B (the reference probes every destination slot of every source).
B_ALG_CANDIDATE = 368
HBM_PEAK_GBS = 8000.0
# MI355X_MICROARCH.md: 256 CUs x 4 SIMDs, 2.4 GHz max clock, a wave64 VALU instruction issues over 2 cycles;
# one scalar unit per CU (1 SALU instruction per clock), LDS 1 wave-instruction per >= 2 cycles per CU
N_SIMD = 1024
N_CU = 256
CLOCK_HZ = 2.4e9
VALU_PEAK = N_SIMD * CLOCK_HZ / 2.0  # wave-instructions / s
SALU_PEAK = N_CU * CLOCK_HZ
LDS_PEAK = N_CU * CLOCK_HZ / 2.0

# rocprofv3 counter passes hang now and then on this pool (FETCH_SIZE most often, whatever its position: rounds 2-4); every pass has
# its own short deadline and a failed pass only drops its own counters.
# M2 start state (see --solve-start).  M1 is always timed on the round-robin fill (comparable across rounds); M2 starts from the
# Clarke-Wright savings construction with a capacity-checking feasibility hook (an extension over the stock structural hook, see
# the module docstring), built inside the 60 s on both sides (profiles/r02f_solve60_*: best@60 s [0, -92932] from this start vs
# [0, -101064] from the round-robin fill and [-4869, -24557] from the stock structural hook).
SOLVE_START_DEFAULT = "savings_capacity"

# M2 policy: the reference's default list policy (default_local_search/policy/list.rs:24-33 without the precedence pair, which the
# CVRP slot does not declare): nearby change, nearby swap, sublist change, sublist swap, reverse, 3-opt (distance-pruned), ruin --
# LateAcceptance(400) + AcceptedCount(256), StratifiedRandom root union -- on BOTH sides; `nearby2` = the two-leaf union M1 is timed on.
M2_POLICIES = {
    "default": ("nearby_change", "nearby_swap", "sublist_change", "sublist_swap", "list_reverse", "kopt", "ruin"),
    "default6": ("nearby_change", "nearby_swap", "sublist_change", "sublist_swap", "list_reverse", "kopt"),
    "nearby2": ("nearby_change", "nearby_swap"),
}
M2_REPLICAS = {"default": 24576, "default6": 24576, "nearby2": 6144}  # replicas per GPU of the M2 leg: eight residencies of the RUIN instantiation's 12 per CU /
# six of the six-leaf kernel's 16, with 100,000 candidates per replica per launch (round 6, profiles/r06g_launch_shapes.txt: seven-leaf 6.26 G moves/s at
# 6,144 x 30,000 -> 7.15 G at 12,288 x 100,000 -> 7.53 G at 24,576 x 100,000 in the long-step regime; sustained over the 60 s leg 6.53 / 6.68 / 6.75 G at
# 12,288 / 18,432 / 24,576; a launch ends with its slowest replicas, more and longer-running workgroups amortise that tail)
# M2 extension leg (module docstring): what is varied against the parity leg, and nothing else
M1_REPLICAS = 98304  # the timed M1 leg: sixteen residencies of 24 replicas per CU (round 6, profiles/r06g_launch_shapes.txt: 24,576 49.9 G, 49,152 52.3 G, 98,304 53.3 G)
C5_REPLICAS = 2816  # the CVRP-5000 side leg: 11 replicas per CU (launch mode 6)
TUNED = {"leaves": ("nearby_change", "nearby_swap"), "late_acceptance_size": 5000, "accepted_count_limit": 1, "replicas": 1024,
         "migration_period_s": 5.0, "migration_replace_fraction": 0.5, "migration_elite": 8, "launch_move_budget": 200_000}
LEAF_BITS = {"nearby_change": 16, "nearby_swap": 32, "list_reverse": 64, "sublist_change": 128, "sublist_swap": 256, "kopt": 512, "ruin": 1024}

# The instruction counters first (the issue rooflines need them), then the two TCC traffic counters in passes of their own, then the
# wave-cycle shares.  rocprofv3 counter passes hang now and then on this pool (a pass takes 2-10 s when it works; once a box starts
# hanging it tends to keep hanging): every pass has a short deadline and ONE retry, and all passes together share PMC_BUDGET_S so the
# default run stays within a few minutes; a pass that never completes only drops its own counters.
PMC_PASSES = [
    ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_SMEM"],
    # memory-side traffic.  Round 5: the L2's fabric request counters themselves (what FETCH_SIZE / WRITE_SIZE are derived from,
    # MI355X_MICROARCH.md "HBM": FETCH_SIZE = TCC_EA0_RDREQ x 64 B; measured ratio 0.9996, profiles/r05_c5_bench.json) fit ONE pass; FETCH_SIZE
    # and WRITE_SIZE stay as passes of their own at the end and win when they complete.
    ["TCC_EA0_RDREQ_sum", "TCC_EA0_WRREQ_sum"],
    ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_LDS_BANK_CONFLICT"],
    ["FETCH_SIZE"],
    ["WRITE_SIZE"],
]
PMC_BUDGET_S = 240.0
# counter record of the M2 leg's kernel (the generic N-leaf engine): the child replays the leg's first M2_PMC_WARM + M2_PMC_TIMED launches (same seeds, same
# trajectory) under rocprofv3; the parent times the same launch window of its own, unprofiled, leg with HIP events
M2_PMC_WARM, M2_PMC_TIMED = 20, 4  # (2 M candidates per replica in: the long-step regime the leg spends most of its time in)
M2_PMC_PASSES = [["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR"], ["TCC_EA0_RDREQ_sum", "TCC_EA0_WRREQ_sum"],
                 ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"]]
# rocprofv3 --pmc crashes (SIGSEGV inside the tool, 8 of 8 runs) on launches of more than one residency of this kernel (>= 12,288 replicas
# = 3,072 workgroups) on this pool, and collects fine at 6,144 (profiles/r04f_pmc_crash_notes.txt).  The counter passes therefore run the
# SAME command at one residency and the line scales their per-launch counters by the work ratio (consumed candidates of the parent's
# timed launches / of the child's): per-candidate instruction and byte counts do not depend on how many replicas share a launch.
PMC_CHILD_MAX_REPLICAS = 6144
# --dump-outputs: replicas whose routes and counters are written, drawn once with a fixed seed
DUMP_SAMPLE = 64
DUMP_SEED = 20240601


def cpu_baseline(problem, seed, warm_steps, timed_steps, budget_s):
    """oracle/ timed on one host core over the same step window as GPU replica 0."""
    from oracle import sfo

    o = sfo.Model.cvrp(problem["capacity"], problem["depot"], problem["demands"], problem["matrix"],
                       problem["customers"], problem["routes"])
    o.configure(leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=20, random_seed=seed)
    o.phase_start()
    aligned = warm_steps <= 2000
    if aligned and warm_steps:
        o.steps(warm_steps)
    m0 = o.stats()["moves_evaluated"]
    done = 0
    t0 = time.perf_counter()
    while done < timed_steps and time.perf_counter() - t0 < budget_s:
        n = min(100, timed_steps - done)
        o.steps(n)
        done += n
    dt = time.perf_counter() - t0
    moves = o.stats()["moves_evaluated"] - m0
    first = warm_steps if aligned else 0
    return {
        "value": moves / dt,
        "unit": "moves/s",
        "cores": 1,
        "kind": "port",
        "sample": f"local-search steps [{first}, {first + done}) of the same CVRP workload, seed {seed} "
                  f"(= GPU replica 0's search): {moves} moves in {dt:.1f}s on 1 host core",
        "steps": done,
        "working_score": [int(v) for v in o.score()[:2]] if (aligned and done == timed_steps) else None,
        "best_score": [int(v) for v in o.best_score()[:2]],
    }


def cpu_solve(problem, seed, seconds, box, start="roundrobin", leaves=("nearby_change", "nearby_swap"), la_size=400, limit=256):
    """M2 on the host: the oracle searches for `seconds` of wall clock on one core (runs beside the GPU solve; the
    ctypes call releases the GIL).  A savings start (Clarke-Wright construction) is built inside the budget."""
    try:
        from oracle import sfo

        o = sfo.Model.cvrp(problem["capacity"], problem["depot"], problem["demands"], problem["matrix"],
                           problem["customers"], problem["routes"])
        o.configure(leaves=sum(LEAF_BITS[x] for x in leaves), max_nearby=20, random_seed=seed, la_size=la_size, limit=limit)
        o.set_ruin()
        t0 = time.perf_counter()
        if start != "roundrobin":
            o.construct_list_clarke_wright(problem["customers"], 1 if start == "savings_capacity" else 0)
            o.construct_list_k_opt(2, 1)  # the default construction's second step (ListKOpt with route_hooks::feasible)
        construct_s = time.perf_counter() - t0
        start_score = [int(v) for v in o.score()[:2]]
        o.phase_start()
        o.steps_timed(max(seconds - construct_s, 0.0))
        dt = time.perf_counter() - t0
        st = o.stats()
        box["result"] = {"best_score": [int(v) for v in o.best_score()[:2]], "steps": st["step_count"],
                         "moves_evaluated": st["moves_evaluated"], "seconds": dt, "cores": 1,
                         "start_score": start_score, "construction_seconds": construct_s}
    except Exception as e:  # the bench line still goes out; the gap is visible
        box["error"] = f"{type(e).__name__}: {e}"


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` outside a launcher: one process per GPU over torch.distributed.run."""
    from solverforge_amd import _lib

    n_dev = _lib.load().sf_device_count()
    if n_dev < n:
        sys.stderr.write(f"bench.py: --gpus {n} needs {n} HIP devices, this node has {n_dev}; refusing to run fewer "
                         "ranks than asked for (a 1-rank number must not be reported as an N-GPU one)\n")
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def pmc_collect(argv, warmup, steps, kernel_substr, timeout_s, passes=None, attempts=2, budget_s=None, need="SQ_INSTS_VALU"):
    """rocprofv3 --pmc passes of this same command (child mode: warm-up + timed launches only).  Returns
    ({counter: mean per timed launch}, kernel resource info) or (None, reason)."""
    passes = PMC_PASSES if passes is None else passes
    budget_s = PMC_BUDGET_S if budget_s is None else budget_s
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not on PATH"
    out = {}
    info = {}
    base = tempfile.mkdtemp(prefix="sfpmc_", dir="/tmp")
    env = dict(os.environ)
    env["TMPDIR"] = "/tmp"
    failed = []
    t_pmc = time.perf_counter()
    try:
        for i, grp in enumerate(passes):
            d = os.path.join(base, f"pmc_{i}")
            work_file = os.path.join(base, f"work_{i}.json")
            # counters only for the kernel that is priced (the set-up kernels -- presort, compress, radix sort -- run unprofiled)
            cmd = [exe, "--pmc"] + grp + ["--kernel-include-regex", kernel_substr.rstrip("<"), "-f", "csv", "-d", d, "-o", "b", "--", sys.executable,
                                            os.path.abspath(__file__)] + argv + ["--pmc-child", "--pmc-child-out", work_file]
            # own process group: a pass that hangs is killed together with the profiled grandchild.  rocprofv3 counter passes hang
            # now and then on this pool (a pass takes ~10 s when it works): one retry per pass before its counters are given up.
            ok = False
            why = f"{'+'.join(grp)}: the PMC time budget ({budget_s:.0f} s) was spent by earlier passes"
            for attempt in range(attempts):
                left = budget_s - (time.perf_counter() - t_pmc)
                if left < 5.0:
                    break
                deadline = min(timeout_s, left)
                shutil.rmtree(d, ignore_errors=True)
                pr = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                      start_new_session=True)
                try:
                    _, err = pr.communicate(timeout=deadline)
                except subprocess.TimeoutExpired:
                    try:
                        os.killpg(pr.pid, 9)
                    except OSError:
                        pass
                    try:
                        _, err = pr.communicate(timeout=5)
                    except Exception:
                        err = b""
                    # the child arms faulthandler: a pass that hangs says where its Python side was (the tail of its stderr)
                    why = f"{'+'.join(grp)}: timed out after {deadline:.0f}s (attempt {attempt + 1}); child stderr tail: {err.decode(errors='replace')[-240:]!r}"
                    continue
                if pr.returncode != 0:
                    why = f"{'+'.join(grp)}: rc={pr.returncode} {err.decode(errors='replace')[-160:]} (attempt {attempt + 1})"
                    continue
                ok = True
                break
            if not ok:
                failed.append(why)
                continue
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            per = {}
            for f in files:
                for row in csv.DictReader(open(f)):
                    if kernel_substr not in row["Kernel_Name"]:
                        continue
                    per.setdefault(row["Counter_Name"], []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"])))
                    info = {"kernel": row["Kernel_Name"], "rocprofv3_allocation": {"vgpr": int(row.get("VGPR_Count", 0) or 0), "sgpr": int(row.get("SGPR_Count", 0) or 0),
                                                                                   "scratch": int(row.get("Scratch_Size", 0) or 0)}}
            if not per:
                failed.append(f"{'+'.join(grp)}: no rows for {kernel_substr}")
            try:
                info["child_work"] = json.load(open(work_file))
            except Exception:
                pass
            for c, v in per.items():
                v.sort()
                vals = [x for _, x in v][warmup:warmup + steps]  # the timed launches, in dispatch order
                if len(vals) != steps:
                    failed.append(f"{c}: {len(v)} dispatches of {kernel_substr}, expected {warmup + steps}")
                    continue
                out[c] = sum(vals) / len(vals)
    finally:
        shutil.rmtree(base, ignore_errors=True)
    if info.get("kernel"):
        info.update(elf_kernel_resources(info["kernel"]))
    if failed:
        info = dict(info, failed_passes=failed)
    if need not in out:
        return None, "; ".join(failed) or f"no {need}"
    return out, info


def dump_outputs(d, out_dir, suffix=""):
    """--dump-outputs: what a caller of the timed path receives after its last launch, as float64 .npy files (int64 scores and
    counters of this size are exact in float64).  Scores of every replica; routes and counters of a fixed, seeded sample of
    DUMP_SAMPLE replicas (the routes of all 98,304 would be ~0.9 GB).  A route file holds one row per sampled replica: the
    element ids of each list followed by -1, padded with -2 to the longest row."""
    os.makedirs(out_dir, exist_ok=True)
    n = d.n_replicas
    sample = np.arange(n) if n <= DUMP_SAMPLE else np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_SAMPLE, replace=False))

    def routes(best):
        rows = [np.concatenate([np.append(np.asarray(r, dtype=np.float64), -1.0) for r in d.working_lists(0, int(i), best=best)]) for i in sample]
        w = max(len(r) for r in rows)
        return np.stack([np.pad(r, (0, w - len(r)), constant_values=-2.0) for r in rows])

    arrays = {
        "working_scores": d.calculate_score().astype(np.float64),  # [replicas, levels] committed (hard, soft)
        "best_scores": d.best_scores().astype(np.float64),
        "sample_replicas": sample.astype(np.float64),
        "sample_working_routes": routes(False),
        "sample_best_routes": routes(True),
        # [sample, 10] in the order of sf_stats: step_count, moves_generated, moves_evaluated, moves_accepted, moves_applied,
        # score_calculations, moves_not_doable, candidates_scored, sources_scanned, reserved
        "sample_stats": np.array([list(d.stats(int(i)).values()) for i in sample], dtype=np.float64),
    }
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a)


def seconds_to_reach(curve, target):
    """First time of `curve` [(seconds, score tuple)] at which the score is >= target (lexicographic), or None."""
    if not curve or not target:
        return None
    tgt = tuple(int(v) for v in target)
    for t, b in curve:
        if tuple(b) >= tgt:
            return round(t, 3)
    return None


def elf_kernel_resources(kernel_name):
    """Registers / spills / scratch of one kernel from the shipped library's gfx950 code objects (the kernel descriptor notes, scripts/elf_resources.py):
    what the hardware allocates from.  rocprofv3's VGPR_Count / SGPR_Count columns are allocation figures of the dispatch, not the descriptor's counts."""
    try:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scripts"))
        import elf_resources

        hit = [k for k in elf_resources.kernels() if k["kernel"] == kernel_name]
        if not hit:
            return {"source": "code-object notes: kernel not found"}
        k = hit[0]
        return {"vgpr": k.get("vgpr"), "agpr": k.get("agpr"), "sgpr": k.get("sgpr"), "scratch": k.get("scratch"), "sgpr_spills": k.get("sgpr_spills"),
                "vgpr_spills": k.get("vgpr_spills"), "lds_static": k.get("lds_static"), "source": "code-object notes of libsolverforge_amd.so (llvm-readelf --notes)"}
    except Exception as e:  # the line is still worth having
        return {"source": f"code-object notes unavailable: {e!r}"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--replicas", type=int, default=M1_REPLICAS,
                    help="independent searches per GPU and launch (98304 = 16 x 24 per CU: the COMPACT wave kernel runs 6 waves per SIMD at CVRP-1000, "
                         "and a launch of many residencies keeps every CU busy while the slower replicas of the earlier ones finish -- one residency "
                         "alone leaves a quarter of the slot time idle, profiles/r04c_wave_replica_sweep.txt, profiles/r06g_launch_shapes.txt)")
    ap.add_argument("--ls-steps", type=int, default=200, help="local-search steps per launch")
    ap.add_argument("--customers", type=int, default=1000)
    ap.add_argument("--vehicles", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=55)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-nearby", type=int, default=20, help="diagnostics (scripts/salu_fit.py): max_nearby of the two nearby leaves (the metric is quoted at 20)")
    ap.add_argument("--accepted-limit", type=int, default=256, help="diagnostics: AcceptedCount limit (the metric is quoted at 256)")
    ap.add_argument("--engine", choices=["auto", "block", "wave"], default="auto")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--solve-seconds", type=float, default=60.0, help="M2: wall-clock budget of the solve leg (0 = skip)")
    ap.add_argument("--solve-start", choices=["roundrobin", "savings", "savings_capacity"], default=SOLVE_START_DEFAULT,
                    help="M2 start state: the round-robin fill M1 is timed on, or the device's Clarke-Wright savings construction "
                         "from empty routes (built inside the budget, on both sides): savings = the reference's stock savings hooks "
                         "(structural feasibility only), savings_capacity = EXTENSION, a capacity-checking feasible hook")
    ap.add_argument("--solve-replicas", type=int, default=0, help="M2: replicas per GPU of the solve leg (0 = M2_REPLICAS of the policy)")
    ap.add_argument("--solve-budget", type=int, default=100_000, help="M2: candidates per replica per launch (sf_solve_moves)")
    ap.add_argument("--solve-policy", choices=sorted(M2_POLICIES), default="default",
                    help="M2 leaves on both sides: default = the reference's seven-leaf default list policy, default6 = without ruin, "
                         "nearby2 = the two-leaf nearby union M1 is timed on")
    ap.add_argument("--tuned-seconds", type=float, default=30.0,
                    help="M2 extension leg: wall-clock budget of the tuned configuration (0 = skip); see TUNED below")
    ap.add_argument("--c5-seconds", type=float, default=5.0,
                    help="side leg: seconds of the same 2-leaf search on BASELINE config 5 (CVRP-5000 / 500, 2,816 replicas per GPU; 0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline M1 figure, run the rocprofv3 counter passes (roofline), the CPU baseline, the M2 solve legs and the "
                         "CVRP-5000 side leg; a plain run does none of them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed launches, write what the last one computed (scores, best scores, a fixed sample of replicas' routes "
                         "and counters) as DIR/<name>.npy in float64")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 --pmc child passes (roofline fields stay null)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pmc-child-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--pmc-child-m2", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    m2_replicas = args.solve_replicas or M2_REPLICAS[args.solve_policy]

    if args.pmc_child or args.pmc_child_m2:  # a counter pass that hangs (rocprofv3 does now and then on this pool) leaves a Python stack in its stderr
        import faulthandler

        faulthandler.dump_traceback_later(30, exit=False)
    # the host driver only supports dmabuf IPC: RCCL's cross-process buffer sharing needs this before HIP initialises
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import __graft_entry__ as entry

    launched = "WORLD_SIZE" in os.environ
    if not launched and args.gpus > 1:
        entry.build()
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); refusing to report one as the other\n")
        sys.exit(2)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod  # plumbing only: rendezvous + barrier (gloo, CPU tensors)

        dist = dist_mod
        dist.init_process_group("gloo", rank=rank, world_size=world)

    # one builder per node: the other ranks wait, then only load the finished library
    if dist is None or local_rank == 0:
        entry.build()
    if dist is not None:
        dist.barrier()
        if local_rank != 0:
            entry.build()  # no-op when the library is current
    import solverforge_amd as sfa
    from solverforge_amd import _lib, datasets, portfolio

    problem = datasets.make_cvrp(args.customers, args.vehicles, args.capacity, seed=args.seed)
    n_dev = _lib.load().sf_device_count()
    if n_dev < 1:
        raise sfa.SolverForgeError("SF_ERR_NO_DEVICE: bench.py measures the HIP path; there is no CPU fallback")
    if world > n_dev:
        sys.stderr.write(f"bench.py: {world} ranks but {n_dev} HIP device(s) on this node\n")
        sys.exit(2)
    seed_base = portfolio.rank_seed_base(args.seed, rank, args.replicas)

    def new_director(prob=None, leaves=("nearby_change", "nearby_swap"), replicas=None, la_size=400, limit=256):
        nrep = replicas or args.replicas
        d = sfa.build_cvrp(prob if prob is not None else problem, n_replicas=nrep, device_id=local_rank, leaves=leaves, max_nearby=args.max_nearby)
        if limit == 256:
            limit = args.accepted_limit
        if len(leaves) == 2:
            d.set_engine({"auto": 0, "block": 1, "wave": 2}[args.engine])
        # replica r of rank q searches with seed base + q*replicas + r  (independent portfolio members)
        d.configure(sfa.SolverConfig(random_seed=portfolio.rank_seed_base(args.seed, rank, nrep), late_acceptance_size=la_size,
                                     accepted_count_limit=limit))
        return d

    if args.pmc_child_m2:  # counter pass of the M2 leg's kernel: the leg's first launches again, nothing else
        prob2 = problem if args.solve_start == "roundrobin" else dict(problem, routes=[[] for _ in problem["routes"]])
        d2 = new_director(prob2, M2_POLICIES[args.solve_policy], m2_replicas)
        d2.calculate_score()
        if args.solve_start != "roundrobin":
            d2.construct_list_clarke_wright(0, prob2["customers"], 1 if args.solve_start == "savings_capacity" else 0)
            d2.construct_list_k_opt(0, 2, 1)
        d2.phase_start()
        for _ in range(M2_PMC_WARM):
            d2.solve_moves(1 << 20, args.solve_budget, sync=True)
        b2 = d2.total_stats()
        for _ in range(M2_PMC_TIMED):
            d2.solve_moves(1 << 20, args.solve_budget, sync=True)
        a2 = d2.total_stats()
        if args.pmc_child_out:
            with open(args.pmc_child_out, "w") as f:
                json.dump({"moves_evaluated": a2["moves_evaluated"] - b2["moves_evaluated"], "candidates_scored": a2["candidates_scored"] - b2["candidates_scored"],
                           "launches": M2_PMC_TIMED, "ls_steps": a2["step_count"] - b2["step_count"], "replicas": m2_replicas}, f)
        d2.close()
        return
    d = new_director()
    start_score = d.calculate_score()[0].tolist()
    engine = {1: "block", 2: "wave"}[d.engine()]
    d.phase_start()

    def barrier(dd):
        dd.sync()
        if dist is not None:
            dist.barrier()
        dd.sync()

    for _ in range(args.warmup):
        d.solve_steps(args.ls_steps, sync=False)
    barrier(d)
    d.profile_solve()  # drop warmup events
    before = d.total_stats()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        d.solve_steps(args.ls_steps, sync=False)
    barrier(d)
    elapsed = time.perf_counter() - t0
    if args.pmc_child:  # counters are read by the parent from rocprofv3's CSV; the child says how much work its timed launches did
        after_c = d.total_stats()
        if args.pmc_child_out:
            with open(args.pmc_child_out, "w") as f:
                json.dump({"moves_evaluated": after_c["moves_evaluated"] - before["moves_evaluated"],
                           "candidates_scored": after_c["candidates_scored"] - before["candidates_scored"], "launches": args.steps,
                           "ls_steps": after_c["step_count"] - before["step_count"], "sources_scanned": after_c["sources_scanned"] - before["sources_scanned"],
                           "replicas": args.replicas}, f)
        d.close()
        return
    if dist is not None:
        elapsed = portfolio.max_over_ranks(dist, elapsed)
    kernel_ms, launches = d.profile_solve()  # HIP events on the context stream (the launch stream)
    after = d.total_stats()
    delta = {k: after[k] - before[k] for k in after}
    replica0_score = [int(v) for v in d.calculate_score()[0]]
    m1_best = list(max(tuple(int(v) for v in s) for s in d.best_scores()))
    if args.dump_outputs:
        dump_outputs(d, args.dump_outputs, "" if world == 1 else f"_rank{rank}")

    moves_local = delta["moves_evaluated"]
    scored_local = delta["candidates_scored"]
    moves_total = moves_local
    if dist is not None:
        moves_total = portfolio.sum_over_ranks(dist, moves_local)

    # ---- M2: a fresh portfolio solves for --solve-seconds of wall clock; the CPU oracle beside it on a host core ----
    solve = None
    dx = d  # the context whose best score goes into the portfolio exchange
    if args.full and args.solve_seconds > 0:
        d.close()
        prob2 = problem if args.solve_start == "roundrobin" else dict(problem, routes=[[] for _ in problem["routes"]])
        m2_leaves = M2_POLICIES[args.solve_policy]
        d2 = new_director(prob2, m2_leaves, m2_replicas)
        m2_start = d2.calculate_score()[0].tolist()
        cpu_box = {}
        cpu_thread = None
        if rank == 0 and not args.no_cpu_baseline:
            cpu_thread = threading.Thread(target=cpu_solve, args=(prob2, args.seed, args.solve_seconds, cpu_box, args.solve_start, m2_leaves),
                                          daemon=True)
        barrier(d2)
        if cpu_thread:
            cpu_thread.start()
        t1 = time.perf_counter()
        construct_s = 0.0
        if args.solve_start != "roundrobin":  # ListClarkeWrightPhase on every replica, inside the budget
            sc2, _ = d2.construct_list_clarke_wright(0, prob2["customers"], 1 if args.solve_start == "savings_capacity" else 0)
            m2_start = d2.construct_list_k_opt(0, 2, 1)[0].tolist()  # ListKOptPhase (route_hooks::feasible): the default's second step
            construct_s = time.perf_counter() - t1
        d2.phase_start()
        n_launch = 0
        curve = []  # (seconds since the leg started, best score over this rank's replicas) at every improvement: `seconds_to_cpu_best` reads it
        m2_window = None  # kernel time and work of launches [M2_PMC_WARM, M2_PMC_WARM + M2_PMC_TIMED): the window the counter passes replay
        while time.perf_counter() - t1 < args.solve_seconds:
            if n_launch == M2_PMC_WARM:
                d2.profile_solve()
                m2_wb = d2.total_stats()
            d2.solve_moves(1 << 20, args.solve_budget, sync=True)  # work-balanced launches (sf_solve_moves)
            n_launch += 1
            if n_launch == M2_PMC_WARM + M2_PMC_TIMED:
                wms, wn = d2.profile_solve()
                m2_wa = d2.total_stats()
                m2_window = {"kernel_ms": wms, "launches": wn, "moves_evaluated": m2_wa["moves_evaluated"] - m2_wb["moves_evaluated"],
                             "candidates_scored": m2_wa["candidates_scored"] - m2_wb["candidates_scored"], "ls_steps": m2_wa["step_count"] - m2_wb["step_count"]}
            bnow = max(tuple(int(v) for v in s) for s in d2.best_scores())  # (a 200 KB copy per ~40 ms launch)
            if not curve or bnow > curve[-1][1]:
                curve.append((time.perf_counter() - t1, bnow))
        gpu_s = time.perf_counter() - t1
        st2 = d2.total_stats()
        solve = {
            "seconds": gpu_s, "launches": n_launch, "moves_evaluated": st2["moves_evaluated"], "ls_steps": st2["step_count"],
            "best_score_local": list(max(tuple(int(v) for v in s) for s in d2.best_scores())),
            "moves_per_s": st2["moves_evaluated"] / gpu_s,
            "start": args.solve_start, "start_score": m2_start, "construction_seconds": construct_s,
            "leaves": list(m2_leaves), "replicas": m2_replicas or args.replicas, "curve": curve, "window": m2_window,
        }
        if cpu_thread:
            cpu_thread.join(timeout=args.solve_seconds + 30)
            solve["cpu_oracle"] = cpu_box.get("result", {"error": cpu_box.get("error", "did not finish")})
        if dist is not None:
            solve["moves_evaluated_all_ranks"] = portfolio.sum_over_ranks(dist, st2["moves_evaluated"])
        dx = d2

    # ---- M2 extension leg: the tuned configuration (TUNED), elite migration on; the CPU oracle with the same configuration beside it ----
    tuned = None
    if args.full and args.tuned_seconds > 0 and args.solve_seconds > 0:
        prob3 = problem if args.solve_start == "roundrobin" else dict(problem, routes=[[] for _ in problem["routes"]])
        d3 = new_director(prob3, TUNED["leaves"], TUNED["replicas"], TUNED["late_acceptance_size"], TUNED["accepted_count_limit"])
        d3.calculate_score()
        cpu_box3 = {}
        cpu_thread3 = None
        if rank == 0 and not args.no_cpu_baseline:
            cpu_thread3 = threading.Thread(target=cpu_solve, args=(prob3, args.seed, args.tuned_seconds, cpu_box3, args.solve_start, TUNED["leaves"],
                                                                   TUNED["late_acceptance_size"], TUNED["accepted_count_limit"]), daemon=True)
        barrier(d3)
        if cpu_thread3:
            cpu_thread3.start()
        t3 = time.perf_counter()
        t3_start = None
        if args.solve_start != "roundrobin":
            d3.construct_list_clarke_wright(0, prob3["customers"], 1 if args.solve_start == "savings_capacity" else 0)
            t3_start = d3.construct_list_k_opt(0, 2, 1)[0].tolist()
        d3.phase_start()
        n3, migrations, adopted, next_m = 0, 0, 0, TUNED["migration_period_s"]
        while time.perf_counter() - t3 < args.tuned_seconds:
            d3.solve_moves(1 << 20, TUNED["launch_move_budget"], sync=True)
            n3 += 1
            now = time.perf_counter() - t3
            if now >= next_m and now < args.tuned_seconds - 0.5 * TUNED["migration_period_s"]:
                adopted += d3.migrate_local(TUNED["migration_elite"], int(TUNED["replicas"] * TUNED["migration_replace_fraction"]))
                migrations += 1
                next_m += TUNED["migration_period_s"]
        s3 = time.perf_counter() - t3
        st3 = d3.total_stats()
        best3 = max(tuple(int(v) for v in s_) for s_ in d3.best_scores())
        if dist is not None:  # best over the ranks (host-side gather: the parity leg's exchange below is the RCCL one)
            best3 = tuple(portfolio.gloo_allgather_best(dist, best3, rank, world)[1])
        tuned = {"seconds": s3, "gpu": list(best3), "gpu_moves_per_s_rank0": st3["moves_evaluated"] / s3, "gpu_ls_steps_per_replica": st3["step_count"] / TUNED["replicas"],
                 "gpu_launches": n3, "migrations": migrations, "replicas_that_adopted": adopted, "start_score": t3_start,
                 "config": dict(TUNED, leaves=list(TUNED["leaves"])),
                 "note": "EXTENSION beside the parity leg: a configuration of the same facade (LateAcceptance size, AcceptedCount limit) chosen for the "
                         "device's step rate, plus elite migration (sf_portfolio_migrate_local, no reference counterpart); the replicas are no "
                         "longer the reference's single-chain trajectories after the first migration"}
        if cpu_thread3:
            cpu_thread3.join(timeout=args.tuned_seconds + 30)
            tuned["cpu_oracle_same_config"] = cpu_box3.get("result", {"error": cpu_box3.get("error", "did not finish")})
        d3.close()

    # ---- side leg: BASELINE config 5 (CVRP-5000 / 500 vehicles, the size an 8-GPU portfolio runs), the same 2-leaf search for a few seconds ----
    c5 = None
    if args.full and args.c5_seconds > 0 and args.solve_seconds > 0 and args.customers != 5000 and not args.pmc_child:
        try:
            prob5 = datasets.make_cvrp(5000, 500, 55, seed=args.seed)
            d5 = sfa.build_cvrp(prob5, n_replicas=C5_REPLICAS, device_id=local_rank, leaves=("nearby_change", "nearby_swap"))
            d5.configure(sfa.SolverConfig(random_seed=portfolio.rank_seed_base(args.seed, rank, C5_REPLICAS)))
            d5.calculate_score()
            d5.phase_start()
            d5.solve_steps(100)  # warm-up launch
            d5.sync()  # (no collective inside this leg: a rank whose side leg fails must not strand the others)
            b5 = d5.total_stats()
            t5 = time.perf_counter()
            n5 = 0
            while time.perf_counter() - t5 < args.c5_seconds:
                d5.solve_steps(100, sync=True)
                n5 += 1
            s5 = time.perf_counter() - t5
            a5 = d5.total_stats()
            mv5 = a5["moves_evaluated"] - b5["moves_evaluated"]
            mode5, renum5 = d5.wave_layout()
            c5 = {"workload": "solverforge-cvrp 5000 customers / 500 vehicles, 2-leaf nearby union, LateAcceptance(400)+AcceptedCount(256), 2,816 replicas per GPU (11 per CU: launch mode 6)",
                  "seconds": s5, "launches": n5, "moves_per_s_rank0": mv5 / s5, "wave_launch_mode": mode5, "internal_node_numbering": renum5,
                  "best_score_rank0": list(max(tuple(int(v) for v in s_) for s_ in d5.best_scores()))}
            d5.close()
        except Exception as e:  # a side leg never costs the headline line
            c5 = {"error": f"{type(e).__name__}: {e}"}
        if dist is not None:  # every rank, whatever happened above
            tot5 = portfolio.sum_over_ranks(dist, c5.get("moves_per_s_rank0", 0.0))
            c5["moves_per_s_all_ranks"] = tot5

    # ---- portfolio exchange: RCCL all-gather of best scores (correctness: identical winner everywhere) -------------
    exchange = "single-rank"
    best_local = max(tuple(int(v) for v in s) for s in dx.best_scores())
    winner = {"score": list(best_local), "rank": 0}
    ctx_abandoned = False
    if dist is not None:
        import torch

        # The RCCL communicator is set up in a worker thread with a deadline: a rank that cannot bring the xGMI
        # communicator up (driver / IPC configuration) must not hang the bench; every rank then takes the same
        # fallback and the JSON line says so.  A context whose worker thread was abandoned mid-call is never touched
        # again (calls on one context are not re-entrant): the process leaves through os._exit.
        box = {}

        def rccl_exchange():
            try:
                uid = dx.portfolio_unique_id() if rank == 0 else np.zeros(128, dtype=np.uint8)
                tu = torch.from_numpy(uid.copy())
                dist.broadcast(tu, src=0)
                dx.portfolio_init(tu.numpy(), rank, world)
                box["result"] = dx.portfolio_allgather_best()
                try:  # the winner's routes on every rank: ncclBroadcast of the route CSR from the winning rank
                    routes = dx.portfolio_broadcast_best(int(box["result"][1]), int(box["result"][2]))
                    box["winner_customers"] = sum(len(r) for r in routes)
                except Exception as e:
                    box["broadcast_error"] = f"{type(e).__name__}: {e}"
                dx.portfolio_destroy()
            except Exception as e:  # keep the bench alive; report the fallback honestly
                box["error"] = f"{type(e).__name__}: {e}"
            box["finished"] = True

        th = threading.Thread(target=rccl_exchange, daemon=True)
        th.start()
        th.join(timeout=float(os.environ.get("SF_RCCL_TIMEOUT_S", "120")))
        ctx_abandoned = not box.get("finished", False)

        def all_ranks_ok(flag):
            return -portfolio.max_over_ranks(dist, -(1.0 if flag else 0.0)) > 0.5  # min over ranks: everyone or no one

        if all_ranks_ok("result" in box):
            bs, wr, wrep = box["result"]
            winner = {"score": [int(v) for v in bs], "rank": int(wr), "replica": int(wrep)}
            if "winner_customers" in box:
                winner["routes_broadcast_customers"] = int(box["winner_customers"])
            elif "broadcast_error" in box:
                winner["routes_broadcast_error"] = box["broadcast_error"]
            exchange = "rccl-allgather (C ABI sf_portfolio_allgather_best)"
        else:
            why = box.get("error", "RCCL communicator not up before the deadline")
            # second choice: the same all-gather through torch.distributed's "nccl" backend (RCCL over xGMI)
            box2 = {}

            def torch_exchange():
                try:
                    box2["result"] = portfolio.torch_rccl_allgather_best(dist, best_local, rank, world, local_rank)
                except Exception as e:
                    box2["error"] = f"{type(e).__name__}: {e}"

            th2 = threading.Thread(target=torch_exchange, daemon=True)
            th2.start()
            th2.join(timeout=float(os.environ.get("SF_RCCL_TIMEOUT_S", "120")))
            if all_ranks_ok("result" in box2):
                wr, ws = box2["result"]
                winner = {"score": ws, "rank": wr}
                exchange = f"rccl-allgather (torch.distributed nccl backend; C ABI path: {why})"
            else:
                wr, ws = portfolio.gloo_allgather_best(dist, best_local, rank, world)
                winner = {"score": ws, "rank": wr}
                exchange = f"gloo-fallback ({why}; torch nccl: " + box2.get("error", "deadline") + ")"

    if rank == 0:
        gen_bytes_per_source = (args.customers + args.vehicles) * 12
        alg_bytes = scored_local * B_ALG_CANDIDATE + delta["sources_scanned"] * gen_bytes_per_source
        avg_launch_ms = kernel_ms / max(launches, 1)
        launch_s = avg_launch_ms * 1e-3
        kernel = "k_list_search_wave" if engine == "wave" else "k_list_search"
        # ---- PMC: rocprofv3 child passes of this command (N = 1 only: one GPU, one process) ----
        pmc, pmc_info, pmc_source, pmc_full, pmc_child_raw = None, {}, None, None, None
        if not args.full:
            pmc_source = "not collected: the counter passes run with --full"
        child_argv = ["--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--replicas", str(min(args.replicas, PMC_CHILD_MAX_REPLICAS)),
                      "--ls-steps", str(args.ls_steps), "--customers", str(args.customers), "--vehicles", str(args.vehicles),
                      "--capacity", str(args.capacity), "--seed", str(args.seed), "--engine", args.engine]
        # the CPU baseline leg (one host core, ~20 s) runs on a QUIET host, before the counter passes start their own processes (round 5 ran it
        # beside them: contention could only lower the baseline and inflate gpu_over_cpu); an exception becomes a field of the line, not its loss
        cb_box = {}
        cpu_leg = args.full and not args.no_cpu_baseline
        if cpu_leg:
            try:
                cb_box["result"] = cpu_baseline(problem, args.seed, args.warmup * args.ls_steps, args.steps * args.ls_steps, args.cpu_seconds)
            except Exception as e:
                cb_box["result"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_pmc:
            pmc, pmc_info = pmc_collect(child_argv, args.warmup, args.steps, kernel + "<", timeout_s=40, attempts=3)
            if pmc is not None and args.replicas > PMC_CHILD_MAX_REPLICAS:
                # the per-candidate counts the scaling below assumes, checked on the parent's own launch shape: a two-counter pass survives
                # there now and then (profiles/r04f_pmc_crash_notes.txt: 3 of 5), so three short tries; absent = the tool crashed every time
                full_argv = list(child_argv)
                full_argv[full_argv.index("--replicas") + 1] = str(args.replicas)
                full_argv[full_argv.index("--steps") + 1] = "4"
                full, full_info = pmc_collect(full_argv, args.warmup, 4, kernel + "<", timeout_s=40, passes=[["SQ_INSTS_VALU", "SQ_INSTS_SALU"]],
                                              attempts=3, budget_s=100.0)
                if full is not None and (full_info or {}).get("child_work", {}).get("moves_evaluated"):
                    fw = full_info["child_work"]
                    per = fw["moves_evaluated"] / fw["launches"]
                    pmc_full = {"replicas": fw["replicas"], "salu_per_candidate": full["SQ_INSTS_SALU"] / per, "valu_per_candidate": full["SQ_INSTS_VALU"] / per,
                                "launches": fw["launches"]}
                else:
                    pmc_full = {"replicas": args.replicas, "failed": str(full_info)[-300:]}
            if pmc is None:  # no counters, no roofline: the line says so instead of quoting an older profile
                pmc_source = f"none (live rocprofv3 passes failed: {pmc_info})"
                pmc_info = {}
            else:
                pmc_source = "rocprofv3 --pmc child passes of this command, mean over the timed launches"
                cw = (pmc_info or {}).get("child_work")
                if cw and cw.get("replicas") != args.replicas and cw.get("moves_evaluated"):
                    scale = (moves_local / max(launches, 1)) / (cw["moves_evaluated"] / max(cw["launches"], 1))
                    cyc = {"SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"}
                    pmc_child_raw = dict(pmc)
                    # instruction and byte counters scale with the work; the cycle counters are kept as measured (only their ratios are used)
                    pmc = {k: (v if k in cyc else v * scale) for k, v in pmc.items()}
                    pmc_source += (f"; the passes ran at {cw['replicas']} replicas per launch (rocprofv3 crashes on larger launches of this kernel on this pool) and the "
                                   f"instruction / byte counters are scaled by the work ratio {scale:.4f} (consumed candidates per launch, parent / child)")
        roof = {"bound": "valu-issue", "achieved": None, "peak": VALU_PEAK / 1e9, "unit": "G wave-instr/s", "frac": None,
                "traffic": None}
        if pmc and launch_s > 0:
            valu = pmc.get("SQ_INSTS_VALU", 0.0) / launch_s
            salu = pmc.get("SQ_INSTS_SALU", 0.0) / launch_s
            lds = pmc.get("SQ_INSTS_LDS", 0.0) / launch_s
            # issue rooflines of the three pipes the kernel lives on; `bound` names the tightest one (the kernel's HBM use is
            # ~2 % of peak, see hbm_frac).  Peaks: VALU 1024 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction; SALU one scalar
            # unit per CU issuing 1 instruction per clock; LDS 1 wave-instruction per 2 clocks per CU (ds_read_b32 rate).
            fr = {"valu-issue": (valu, VALU_PEAK), "salu-issue": (salu, SALU_PEAK), "lds-issue": (lds, LDS_PEAK)}
            roof["valu_frac"] = valu / VALU_PEAK
            roof["salu_frac"] = salu / SALU_PEAK
            roof["lds_issue_frac"] = lds / LDS_PEAK
            # memory-side traffic per launch (MI355X_MICROARCH.md "HBM"): rocprofv3 reports FETCH_SIZE / WRITE_SIZE in KiB; on gfx950 FETCH_SIZE
            # tallies the L2's 128-byte fabric read requests at 64 B (FETCH_SIZE = TCC_EA0_RDREQ x 64 B) -> the read side is doubled.  When the
            # derived-counter passes did not complete the same figures come from the raw request counters of the one-pass route
            # (reads: TCC_EA0_RDREQ x 64 B, doubled the same way; writes: TCC_EA0_WRREQ x 64 B, an upper bound -- some are 32-byte requests).
            rd = pmc["FETCH_SIZE"] * 1024.0 if "FETCH_SIZE" in pmc else (pmc["TCC_EA0_RDREQ_sum"] * 64.0 if "TCC_EA0_RDREQ_sum" in pmc else None)
            wr = pmc["WRITE_SIZE"] * 1024.0 if "WRITE_SIZE" in pmc else (pmc["TCC_EA0_WRREQ_sum"] * 64.0 if "TCC_EA0_WRREQ_sum" in pmc else None)
            if rd is not None and wr is not None:
                traffic = 2.0 * rd + wr
                roof["traffic"] = traffic
                roof["traffic_source"] = {"read": "FETCH_SIZE x 2" if "FETCH_SIZE" in pmc else "TCC_EA0_RDREQ_sum x 64 B x 2",
                                          "write": "WRITE_SIZE" if "WRITE_SIZE" in pmc else "TCC_EA0_WRREQ_sum x 64 B"}
                if "FETCH_SIZE" in pmc and "TCC_EA0_RDREQ_sum" in pmc:  # both routes completed: they should name the same bytes
                    roof["traffic_source"]["fetch_size_over_rdreq_x64"] = pmc["FETCH_SIZE"] * 1024.0 / max(pmc["TCC_EA0_RDREQ_sum"] * 64.0, 1.0)
                roof["hbm_frac"] = traffic / launch_s / 1e9 / HBM_PEAK_GBS
                roof["traffic_bytes_per_candidate"] = traffic / max(scored_local / max(launches, 1), 1)
                # the measured memory-side traffic competes with the issue rooflines for `bound`: at CVRP-5000 the facts (50 MB matrix,
                # 50 MB neighbour index) no longer fit the L2s and HBM is the tightest one
                fr["hbm"] = (traffic / launch_s, HBM_PEAK_GBS * 1e9)
            bound = max(fr, key=lambda k: fr[k][0] / fr[k][1])
            roof["bound"] = bound
            roof["achieved"] = fr[bound][0] / 1e9
            roof["peak"] = fr[bound][1] / 1e9
            roof["unit"] = "GB/s" if bound == "hbm" else "G wave-instr/s"
            roof["frac"] = fr[bound][0] / fr[bound][1]
            if pmc.get("SQ_WAVE_CYCLES"):
                wc = pmc["SQ_WAVE_CYCLES"]
                roof["wave_cycle_shares"] = {"active": pmc.get("SQ_ACTIVE_INST_ANY", 0) / wc, "wait_mem": pmc.get("SQ_WAIT_ANY", 0) / wc,
                                             "wait_issue": pmc.get("SQ_WAIT_INST_ANY", 0) / wc}
                cwr = ((pmc_info or {}).get("child_work") or {}).get("replicas", args.replicas)
                roof["wave_cycle_shares_shape"] = ("the timed launch shape" if cwr == args.replicas else
                                                   f"one-residency shape: measured on launches of {cwr} replicas (rocprofv3 --pmc crashes on larger launches of this "
                                                   f"kernel, profiles/r05_pmc_probe.txt), where ~1/4 of the slot time idles behind the slowest replicas; the timed "
                                                   f"{args.replicas}-replica launches refill a CU as workgroups retire (profiles/r04c_wave_replica_sweep.txt)")
            cw_ = (pmc_info or {}).get("child_work")
            if cw_ and cw_.get("moves_evaluated") and pmc_child_raw is not None:
                per_c = cw_["moves_evaluated"] / max(cw_["launches"], 1)
                roof["per_candidate"] = {"replicas": cw_["replicas"], "salu": pmc_child_raw.get("SQ_INSTS_SALU", 0.0) / per_c,
                                         "valu": pmc_child_raw.get("SQ_INSTS_VALU", 0.0) / per_c, "lds": pmc_child_raw.get("SQ_INSTS_LDS", 0.0) / per_c}
            elif pmc.get("SQ_INSTS_SALU"):
                per_c = moves_local / max(launches, 1)
                roof["per_candidate"] = {"replicas": args.replicas, "salu": pmc["SQ_INSTS_SALU"] / per_c, "valu": pmc["SQ_INSTS_VALU"] / per_c,
                                         "lds": pmc.get("SQ_INSTS_LDS", 0.0) / per_c}
            if pmc_full is not None:  # the same two counters on the parent's own launch shape, per consumed candidate, side by side
                roof["per_candidate_full_launch"] = pmc_full
            if pmc.get("SQ_BUSY_CYCLES") and not ((pmc_info or {}).get("child_work") or {}).get("replicas", args.replicas) != args.replicas:
                # per-SE busy cycles summed over the 32 shader engines (only when the passes ran the parent's own launch shape)
                roof["effective_clock_ghz"] = pmc["SQ_BUSY_CYCLES"] / 32.0 / launch_s / 1e9
            roof["counters_per_launch"] = {k: pmc[k] for k in sorted(pmc)}
        roof.update({
            "salu_peak_note": "SALU peak = 256 CUs x 2.4 GHz x 1 instruction per clock = 614.4 G/s; scripts/salu_microbench.hip measures what the chip "
                              "issues when every CU's scalar unit is saturated (profiles/r05_salu_microbench.jsonl)",
            "pmc_source": pmc_source, "kernel": (pmc_info or {}).get("kernel") or kernel,
            "kernel_resources": pmc_info or None, "avg_launch_ms": avg_launch_ms, "launches": launches,
            "candidates_scored_per_launch": scored_local / max(launches, 1),
            "sources_scanned_per_launch": delta["sources_scanned"] / max(launches, 1),
            # SURVEY.md §8(d) side number: bytes the REFERENCE algorithm would move for the same candidates / sources;
            # not a bandwidth this kernel uses (its replica state is LDS-resident, the neighbour index is presorted)
            "algorithmic_reference_bytes_per_launch": alg_bytes / max(launches, 1),
            "algorithmic_reference_gbps": alg_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0,
        })
        out = {
            "metric": f"moves-evaluated/sec, CVRP-{args.customers} (nearby-list selector, LateAcceptance(400)+AcceptedCount(256))",
            "value": moves_total / elapsed,
            "unit": "moves/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            # int64 score levels at the boundary and in the committed state; the timed instantiation prices a trial as int32 level deltas
            # gathered from a u16 copy of the matrix under host-checked bounds (exact strength reduction: DESIGN 2.1, csrc/sf_api.hip lm_small)
            "dtype": "int64 score / int32 trial deltas (u16 matrix copy)" if engine == "wave" else "int64",
            "data": "synthetic",
            "config": {
                # (short facts first: the driver's parser keeps 120 characters)
                "workload": f"cvrp {args.customers}/{args.vehicles} nearby-change+nearby-swap max_nearby=20 LA(400) AcceptedCount(256) order=Random; "
                            f"solverforge-cvrp {args.customers} customers / {args.vehicles} vehicles, capacity {args.capacity}, the two nearby list leaves of the default list policy",
                "replicas_per_gpu": args.replicas,
                "ls_steps_per_launch": args.ls_steps,
                "engine": engine,
                "parallelism": f"portfolio x{world} (independent seeds, {exchange})",
                "seed": args.seed,
            },
            "roofline": roof,
            "extra": {
                "candidates_scored_per_s": scored_local * world / elapsed,
                "moves_accepted": delta["moves_accepted"],
                "ls_steps": delta["step_count"],
                "moves_per_ls_step": moves_local / max(delta["step_count"], 1),
                "start_score": start_score,
                "replica0_working_score": replica0_score,
                "best_score_after_timed_region": m1_best,
                "winner": winner,
            },
        }
        if solve is not None:
            out["extra"]["best_score_at_60s"] = {
                "seconds": args.solve_seconds,
                "gpu": winner["score"],  # best over every replica of every rank (the portfolio exchange above)
                "gpu_moves_evaluated": solve.get("moves_evaluated_all_ranks", solve["moves_evaluated"]),
                "gpu_moves_per_s_rank0": solve["moves_per_s"],
                "gpu_ls_steps_rank0": solve["ls_steps"],
                "gpu_launches": solve["launches"],
                "start": solve["start"],
                "start_score": solve["start_score"],
                "gpu_construction_seconds": solve["construction_seconds"],
                "cpu_oracle": solve.get("cpu_oracle"),
                # how long this rank's portfolio needed to reach what the CPU oracle holds after the whole leg (null: never reached / no CPU leg)
                "seconds_to_cpu_best": seconds_to_reach(solve.get("curve"), (solve.get("cpu_oracle") or {}).get("best_score")),
                "gpu_best_curve_rank0": [[round(t, 2), list(b)] for t, b in (solve.get("curve") or [])][:40],
                "start_note": {"savings_capacity": "extension: Clarke-Wright + ListKOpt with a capacity-checking feasible hook (the reference's "
                                                   "stock savings_hooks::feasible is structural only)",
                               "savings": "the reference's stock CVRP construction wiring (structural feasibility)",
                               "roundrobin": "round-robin fill (the M1 start state)"}[solve["start"]],
                "policy": f"start = {solve['start']}; leaves = {'+'.join(solve['leaves'])} ({args.solve_policy}: "
                          + ("the reference's default list policy" if args.solve_policy == "default" else "a subset of the default list policy")
                          + f") on both sides, LateAcceptance(400)+AcceptedCount(256), {solve['replicas']} replicas per GPU; work-balanced launches "
                          f"(sf_solve_moves, {args.solve_budget} candidates per replica per launch)",
            }
        if solve is not None and tuned is not None:
            out["extra"]["best_score_at_60s"]["tuned"] = tuned
        # the numbers a reader compares with other configurations, at the top level of `extra`
        side = {}
        if solve is not None:
            side["cvrp1000_default_list_policy"] = {
                "what": f"the reference's out-of-the-box CVRP solve: {'+'.join(solve['leaves'])} ({args.solve_policy}), LateAcceptance(400)+AcceptedCount(256), "
                        f"{solve['replicas']} replicas per GPU, sustained over the {args.solve_seconds:.0f} s M2 leg (generic N-leaf engine)",
                "moves_per_s_rank0": solve["moves_per_s"], "moves_per_ls_step": solve["moves_evaluated"] / max(solve["ls_steps"], 1)}
            # the same three issue rooflines + memory-side traffic for THIS kernel, over launches [M2_PMC_WARM, +M2_PMC_TIMED) of the leg: time from the
            # leg's own HIP events, counters from rocprofv3 passes over a replay of the same launches (same seeds -> the same work)
            win = solve.get("window")
            roof2 = {"bound": None, "frac": None, "window": win, "kernel": "k_mixed_search_wave"}
            if world == 1 and not args.no_pmc and win and win["launches"] == M2_PMC_TIMED and win["kernel_ms"] > 0:
                m2_argv = ["--gpus", "1", "--customers", str(args.customers), "--vehicles", str(args.vehicles), "--capacity", str(args.capacity), "--seed", str(args.seed),
                           "--solve-start", args.solve_start, "--solve-policy", args.solve_policy, "--solve-budget", str(args.solve_budget), "--solve-replicas", str(m2_replicas),
                           "--pmc-child-m2"]
                pm2, info2 = pmc_collect(m2_argv, M2_PMC_WARM, M2_PMC_TIMED, "k_mixed_search_wave<", timeout_s=60, passes=M2_PMC_PASSES, attempts=2, budget_s=100.0)
                if pm2 is None:
                    roof2["pmc_source"] = f"none (live rocprofv3 passes failed: {info2})"
                else:
                    ls2 = win["kernel_ms"] * 1e-3 / win["launches"]
                    cw2 = (info2 or {}).get("child_work") or {}
                    fr2 = {"valu-issue": (pm2.get("SQ_INSTS_VALU", 0.0) / ls2, VALU_PEAK), "salu-issue": (pm2.get("SQ_INSTS_SALU", 0.0) / ls2, SALU_PEAK),
                           "lds-issue": (pm2.get("SQ_INSTS_LDS", 0.0) / ls2, LDS_PEAK)}
                    roof2.update({"valu_frac": fr2["valu-issue"][0] / VALU_PEAK, "salu_frac": fr2["salu-issue"][0] / SALU_PEAK, "lds_issue_frac": fr2["lds-issue"][0] / LDS_PEAK,
                                  "avg_launch_ms": ls2 * 1e3, "counters_per_launch": pm2,
                                  "replay_matches_leg": cw2.get("moves_evaluated") == win["moves_evaluated"],
                                  "pmc_source": f"rocprofv3 --pmc passes over a replay of launches {M2_PMC_WARM}..{M2_PMC_WARM + M2_PMC_TIMED - 1} of this leg "
                                                "(bench.py --pmc-child-m2), kernel time from the leg's own HIP events"})
                    per2 = win["moves_evaluated"] / win["launches"]
                    roof2["per_candidate"] = {"salu": pm2.get("SQ_INSTS_SALU", 0.0) / per2, "valu": pm2.get("SQ_INSTS_VALU", 0.0) / per2,
                                              "lds": pm2.get("SQ_INSTS_LDS", 0.0) / per2}
                    if "TCC_EA0_RDREQ_sum" in pm2 and "TCC_EA0_WRREQ_sum" in pm2:
                        tr2 = 2.0 * pm2["TCC_EA0_RDREQ_sum"] * 64.0 + pm2["TCC_EA0_WRREQ_sum"] * 64.0
                        roof2["traffic"] = tr2
                        roof2["hbm_frac"] = tr2 / ls2 / 1e9 / HBM_PEAK_GBS
                        roof2["traffic_bytes_per_candidate"] = tr2 / per2
                        fr2["hbm"] = (tr2 / ls2, HBM_PEAK_GBS * 1e9)
                    b2 = max(fr2, key=lambda k: fr2[k][0] / fr2[k][1])
                    roof2.update({"bound": b2, "achieved": fr2[b2][0] / 1e9, "peak": fr2[b2][1] / 1e9, "unit": "GB/s" if b2 == "hbm" else "G wave-instr/s",
                                  "frac": fr2[b2][0] / fr2[b2][1]})
                    if pm2.get("SQ_WAVE_CYCLES"):
                        wc2 = pm2["SQ_WAVE_CYCLES"]
                        roof2["wave_cycle_shares"] = {"active": pm2.get("SQ_ACTIVE_INST_ANY", 0) / wc2, "wait_mem": pm2.get("SQ_WAIT_ANY", 0) / wc2,
                                                      "wait_issue": pm2.get("SQ_WAIT_INST_ANY", 0) / wc2}
                    roof2["kernel"] = (info2 or {}).get("kernel", roof2["kernel"])
                    roof2["kernel_resources"] = {k: v for k, v in (info2 or {}).items() if k not in ("child_work",)}
            side["cvrp1000_default_list_policy"]["roofline"] = roof2
        if c5 is not None:
            side["cvrp5000_nearby2"] = c5
        if side:
            out["extra"]["side_configs"] = side
        if cpu_leg:
            cb = cb_box["result"]
            out["cpu_baseline"] = cb
            if "error" not in cb:
                ws = cb.pop("working_score")
                out["extra"]["gpu_over_cpu"] = out["value"] / cb["value"]
                out["extra"]["replica0_matches_cpu_oracle"] = None if ws is None else bool(ws == replica0_score)
        print(json.dumps(out))
        sys.stdout.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    # torch bundles its own HIP runtime next to the ROCm one this library links: skip the interpreter's exit-time
    # destructors of the two copies; a context abandoned inside a hung RCCL call is not closed either
    sys.stdout.flush()
    sys.stderr.flush()
    if not ctx_abandoned:
        dx.close()
    if dist is not None or ctx_abandoned:
        os._exit(0)


if __name__ == "__main__":
    main()
