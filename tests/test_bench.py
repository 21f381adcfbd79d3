"""bench.py command line: the result line, --steps, --dump-outputs, --full.

The benchmark is a host-side workload, so these run anywhere. Two runs with
the same arguments are started side by side (each hosts its own ensemble on
ephemeral ports) and must dump identical outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import registrar_amd as ra

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZNODES = 37
STEPS = 3


def _start(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.Popen(
        [sys.executable, os.path.join(REPO_ROOT, "bench.py"), "--gpus", "1",
         "--steps", str(STEPS), "--warmup", "1", "--znodes", str(ZNODES),
         "--dump-outputs", str(out_dir)] + list(extra),
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=REPO_ROOT)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two identical runs (the second with --full), finished: [(dir, result)]."""
    dirs = [tmp_path_factory.mktemp("dump%d" % i) / "out" for i in range(2)]
    procs = [_start(dirs[0]), _start(dirs[1], "--full")]
    done = []
    for d, p in zip(dirs, procs):
        out, err = p.communicate(timeout=240)
        assert p.returncode == 0, err.decode(errors="replace")[-2000:]
        lines = out.decode().splitlines()
        assert len(lines) == 1, "exactly one result line on stdout: %r" % lines
        done.append((d, json.loads(lines[0])))
    return done


def test_result_line(runs):
    for _, res in runs:
        assert res["metric"] == "ephemeral registrations/sec"
        assert res["unit"] == "registrations/s"
        assert res["higher_is_better"] is True
        assert res["dtype"] == "n/a"
        assert res["steps"] == STEPS
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed region
        per_step = ZNODES / res["value"] * 1000.0
        assert per_step == pytest.approx(res["ms_per_step"], rel=1e-2, abs=2e-3)


def test_dump_outputs_content(runs):
    d, _ = runs[0]
    assert sorted(os.listdir(d)) == ["heartbeat_rc.npy", "register_rc.npy", "znodes.npy"]
    arrays = {n[:-4]: np.load(d / n) for n in os.listdir(d)}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for a in arrays.values():
        assert a.dtype in (np.float32, np.float64)
    assert arrays["register_rc"].tolist() == [0.0]
    assert arrays["heartbeat_rc"].tolist() == [0.0]
    table = arrays["znodes"]
    assert table.shape[0] == ZNODES
    got = sorted(bytes(row[row != 0].astype(np.uint8)).decode() for row in table)
    base = ra.domain_to_path("rank0.bench.mi355x")
    want = [base + "/bench-r0"] + [ra.domain_to_path("a%04d.rank0.bench.mi355x" % i)
                                   for i in range(ZNODES - 1)]
    assert got == sorted(want)


def test_dump_outputs_repeatable(runs):
    (d0, _), (d1, _) = runs
    assert sorted(os.listdir(d0)) == sorted(os.listdir(d1))
    for n in os.listdir(d0):
        a, b = np.load(d0 / n), np.load(d1 / n)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), n
