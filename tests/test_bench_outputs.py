"""bench.py's plain run and --dump-outputs: the plain result line carries the
headline figure only (what takes runs of its own sits behind --full), and
--dump-outputs writes the last timed step's solution as float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("cold_first_solve", "fsolver_end_to_end", "fsolver_cold_process", "secondary", "cpu_baseline",
             "sharded_diagnosis")


def test_dump_output_is_float64_and_samples_above_the_budget(tmp_path, monkeypatch):
    a = np.arange(1000, dtype=np.float32) * 0.5
    bench.dump_output(str(tmp_path), "small", a)
    got = np.load(tmp_path / "small.npy")
    assert got.dtype == np.float64 and np.array_equal(got, a.astype(np.float64))
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 100)
    bench.dump_output(str(tmp_path), "s1", a)
    bench.dump_output(str(tmp_path / "again"), "s1", a)
    s1, s2 = np.load(tmp_path / "s1.npy"), np.load(tmp_path / "again" / "s1.npy")
    assert s1.shape == (100,) and np.array_equal(s1, s2)          # the same sample every time
    assert np.all(np.diff(s1) > 0) and np.isin(s1, a).all()       # distinct entries of a, in order
    bench.dump_output(str(tmp_path), "shared", a, n_files=4)      # four files share the budget
    assert np.load(tmp_path / "shared.npy").shape == (25,)
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10 ** 6


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_solution(tmp_path, monkeypatch, capsys):
    """In this process (it has the GPU up already): a 120 x 120-cell plain run.
    The dumped A is the solution of the same problem: both are PCG answers to
    Precision 1e-8, each within the suite's 1e-5 of max |A| of the converged
    answer (tests/util.py), so within 2e-5 of each other."""
    from xfemm_amd import kernels, synth
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--cells", "120",
                                      "--dump-outputs", str(tmp_path)])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "DoF/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - 121 * 121 / (1e-3 * line["ms_per_step"])) <= 1e-9 * line["value"]
    assert not [k for k in FULL_ONLY if k in line] and "phases" not in line["roofline"]
    assert sorted(os.listdir(tmp_path)) == ["A.npy"]
    A = np.load(tmp_path / "A.npy")
    assert A.dtype == np.float64 and A.shape == (121 * 121,) and np.isfinite(A).all()
    P = kernels.Static2DProblem(device=0, **synth.magnetostatic(120))
    P.solve()
    A1 = P.solution()
    P.close()
    assert np.abs(A - A1).max() <= 2e-5 * np.abs(A1).max()
