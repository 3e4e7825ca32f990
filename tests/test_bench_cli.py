"""bench.py's command line and step schedule (CPU only but for the one test
marked gpu): the driver's fixed command `bench.py --gpus 1 --steps 20
--warmup 5` must parse and time exactly --steps leapfrog steps whatever Nt the
thermalisation ends with; --full and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench


def test_driver_argv_parses():
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (a.gpus, a.steps, a.warmup, a.Nt) == (1, 20, 5, 10)


def test_plain_run_is_lean_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_float64_arrays(tmp_path):
    class Ctx:
        def get_state(self):
            z = (np.arange(12.0) + 1j * np.arange(12.0)[::-1]).reshape(1, 6, 2)
            return z, -z

    acc = np.array([[True], [False]])
    dH = np.array([[0.25], [-0.5]])
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), Ctx(), acc, dH, 0, 1)
    got = {f.name: np.load(f) for f in out.iterdir()}
    assert sorted(got) == ["Delta.npy", "accepted.npy", "dH.npy", "pi.npy"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["Delta.npy"].shape == (1, 6, 2, 2)
    assert np.array_equal(got["Delta.npy"][..., 0], np.arange(12.0).reshape(1, 6, 2))
    assert np.array_equal(got["pi.npy"][..., 1], -np.arange(12.0)[::-1].reshape(1, 6, 2))
    assert np.array_equal(got["accepted.npy"], [[1.0], [0.0]]) and np.array_equal(got["dH.npy"], dH)


def _run_bench(args):
    root = os.path.dirname(os.path.abspath(bench.__file__))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, cwd=root, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    """A plain run prints the headline record without the side measurements;
    --full adds them; both time the same seeded sweeps, so their dumps are
    equal bit for bit (the HIP path is deterministic)."""
    args = ["--gpus", "1", "--steps", "8", "--warmup", "2", "--L", "8", "--beta", "4", "--therm", "10"]
    plain = _run_bench(args + ["--dump-outputs", str(tmp_path / "plain")])
    full = _run_bench(args + ["--full", "--dump-outputs", str(tmp_path / "full")])
    for rec in (plain, full):
        assert rec["steps"] == 8 and rec["ms_per_step"] > 0 and rec["dtype"] == "f64"
        assert rec["value"] == pytest.approx(1000.0 / rec["ms_per_step"])      # one chain, one GPU
    moved = {"roofline", "assembly", "cpu_baseline"}
    assert not moved & set(plain) and moved <= set(full)
    names = sorted(f.name for f in (tmp_path / "plain").iterdir())
    assert names == ["Delta.npy", "accepted.npy", "dH.npy", "pi.npy"]
    for n in names:
        x, y = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert x.dtype == np.float64 and np.all(np.isfinite(x)) and np.array_equal(x, y), n
    sweeps = sum(t["sweeps"] for t in plain["timed_trajectories"])
    assert np.load(tmp_path / "plain" / "dH.npy").shape == (sweeps, 1)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--Nt", "0"]])
def test_bad_counts_rejected(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


@pytest.mark.parametrize("steps", [1, 5, 9, 10, 20, 23, 50, 101])
@pytest.mark.parametrize("Nt", [1, 4, 10, 12, 17, 40])
def test_schedule_is_exact(steps, Nt):
    pieces = bench.schedule(3, steps, Nt)
    assert sum(n * nt for _, n, nt in pieces) == steps
    # draw indices are consecutive from `first`, every trajectory but the last has Nt steps
    first = 3
    for f, n, nt in pieces:
        assert f == first
        first += n
    assert all(nt == Nt for _, _, nt in pieces[:-1])
    assert bench.n_draws(pieces) == -(-steps // Nt)


def test_warmup_rounds_up_to_sweeps():
    Nt = 10
    warm = bench.schedule(0, -(-5 // Nt) * Nt, Nt)
    assert warm == [(0, 1, 10)]
