"""CPU tests of bench.py's launcher contract: `--gpus N` must never silently run fewer ranks than asked for, and the
product path must refuse to run without a HIP device (no CPU fallback)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _device_count():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    return _lib.load().sf_device_count()


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_gpus_n_refuses_to_run_with_fewer_devices():
    n = _device_count()
    r = _run(["--gpus", str(n + 2), "--steps", "1", "--warmup", "0", "--solve-seconds", "0", "--no-pmc"])
    assert r.returncode == 2
    assert b"refusing to run fewer ranks" in r.stderr
    assert r.stdout.strip() == b""  # no JSON line: nothing to mistake for an N-GPU result


def test_c5_portfolio_refuses_to_run_with_fewer_devices():
    """BASELINE config 5 (CVRP-5000, the 8-GPU portfolio): the same refusal, before any problem data is built."""
    n = _device_count()
    r = _run(["--customers", "5000", "--vehicles", "500", "--replicas", "1280", "--gpus", str(max(n, 0) + 2), "--steps", "1", "--warmup", "0",
              "--solve-seconds", "0", "--no-pmc"])
    assert r.returncode == 2
    assert b"refusing to run fewer ranks" in r.stderr
    assert r.stdout.strip() == b""


def test_gpus_flag_must_match_the_launcher():
    r = _run(["--gpus", "1", "--steps", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2
    assert b"refusing to report one as the other" in r.stderr


def test_no_device_no_number():
    if _device_count() > 0:
        pytest.skip("a HIP device is present")
    r = _run(["--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert b"SF_ERR_NO_DEVICE" in r.stderr
    assert r.stdout.strip() == b""


def test_launch_shapes_are_whole_residencies():
    """The replica counts bench.py launches by default fill the 256 CUs evenly (round 6: the legs run many residencies per launch; a count that is not a
    multiple of one residency would leave CUs idle at the end of every launch), and the counter window of the M2 leg lies inside a short leg."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.M1_REPLICAS % (24 * 256) == 0  # wave engine, COMPACT slice at CVRP-1000: 24 replicas per CU
    assert b.M2_REPLICAS["default"] % (12 * 256) == 0  # generic engine, FAST + RUIN: 12 per CU
    assert b.M2_REPLICAS["default6"] % (16 * 256) == 0  # six-leaf FAST: 16 per CU
    assert b.C5_REPLICAS % (11 * 256) == 0  # wave engine, launch mode 6 at CVRP-5000: 11 per CU
    assert b.PMC_CHILD_MAX_REPLICAS % (24 * 256) == 0
    assert 0 < b.M2_PMC_TIMED <= b.M2_PMC_WARM  # the window [WARM, WARM + TIMED) of launches: past the construction, a few launches long
    assert [c for p in b.M2_PMC_PASSES for c in p].count("SQ_INSTS_SALU") == 1


def test_full_and_dump_outputs_are_options():
    """The side legs sit behind --full (off by default); --dump-outputs DIR is accepted."""
    r = _run(["--help"])
    assert r.returncode == 0
    assert b"--full" in r.stdout and b"--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_identical_outputs(tmp_path):
    """A plain run times only the M1 launches (no CPU baseline, no M2 legs) and, with --dump-outputs, writes the last launch's
    outputs as float64 .npy files; two runs with the same arguments write the same arrays."""
    import json

    import numpy as np

    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--replicas", "512", "--ls-steps", "50"]
    lines = []
    for k in range(2):
        r = _run(args + ["--dump-outputs", str(tmp_path / f"run{k}")])
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "cpu_baseline" not in line and "best_score_at_60s" not in line["extra"] and "side_configs" not in line["extra"]
    names = sorted(os.listdir(tmp_path / "run0"))
    assert names == sorted(os.listdir(tmp_path / "run1")) and "working_scores.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "run0" / n), np.load(tmp_path / "run1" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    scores = np.load(tmp_path / "run0" / "working_scores.npy")
    assert scores.shape == (512, 2) and scores[0].tolist() == lines[0]["extra"]["replica0_working_score"]
