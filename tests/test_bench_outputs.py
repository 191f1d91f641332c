"""bench.py command-line contract: ``--steps`` sets the timed step count,
the result line carries ``ms_per_step``, ``--dump-outputs`` writes the
last step's outputs reproducibly, and the secondary mm/staging GPU runs
happen with ``--full`` only."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def _run_bench(*extra):
    proc = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "5",
         "--warmup", "2", *extra],
        cwd=str(REPO),
        capture_output=True,
        text=True,
        timeout=240,
    )
    assert proc.returncode == 0, proc.stderr[-3000:]
    (line,) = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    return json.loads(line)


def _load_dump(path):
    files = sorted(path.glob("*.npy"))
    return {f.stem: np.load(f) for f in files}


def test_dump_outputs_reproducible_and_full_flag(tmp_path):
    a = _run_bench("--dump-outputs", str(tmp_path / "a"))
    # --no-secondary: the GB-sized secondary runs are not this test's matter
    b = _run_bench("--full", "--no-secondary",
                   "--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert line["steps"] == 5 and line["warmup"] == 2
        assert line["metric"] == "electrons_per_sec"
        assert line["ms_per_step"] > 0
        assert line["secondary"] == []

    da, db = _load_dump(tmp_path / "a"), _load_dump(tmp_path / "b")
    # worker_gpu is written only where the worker has a GPU to probe
    assert set(da) == set(db)
    assert {"result", "worker_served"} <= set(da) <= {
        "result", "worker_served", "worker_gpu"}
    for name, arr in da.items():
        assert arr.dtype in (np.float32, np.float64)
        assert np.array_equal(arr, db[name])
    # the noop electron returns 0 to its caller; one warm worker served
    # every electron of the run, warmup included
    assert da["result"].shape == () and da["result"] == 0
    assert da["worker_served"] == 2 + 5
    if "worker_gpu" in da:
        assert da["worker_gpu"].shape == (4,) and np.all(da["worker_gpu"] > 0)
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= 64 * 10**6


def test_dump_outputs_samples_large_results(tmp_path):
    """An output over the 64 MB budget is cut to a fixed seeded sample."""
    sys.path.insert(0, str(REPO))
    try:
        import bench
    finally:
        sys.path.remove(str(REPO))
    import torch

    n = bench.DUMP_LIMIT_BYTES // 4 + 1000
    big = torch.arange(n, dtype=torch.int32)  # exact in float32 (n < 2**24)
    result = {"t": big, "half": torch.ones(3, dtype=torch.bfloat16),
              "stats": [1, 2.5], "note": "text is left out"}
    meta = {"gpu": None, "served": None}
    for sub in ("x", "y"):
        bench.dump_outputs(str(tmp_path / sub), bench.caller_view(result, meta))
    dx, dy = _load_dump(tmp_path / "x"), _load_dump(tmp_path / "y")
    assert set(dx) == {"result_t", "result_half", "result_stats"}
    assert dx["result_t"].dtype == np.float32
    assert dx["result_half"].dtype == np.float32
    assert dx["result_half"].tolist() == [1.0, 1.0, 1.0]
    assert dx["result_stats"].dtype == np.float64
    assert dx["result_stats"].tolist() == [1.0, 2.5]
    assert dx["result_t"].size == bench.DUMP_LIMIT_BYTES // 3 // 4
    # the values are their own indices: ascending and without repeats,
    # from the first stratum to the last
    assert np.all(np.diff(dx["result_t"]) > 0)
    assert dx["result_t"][0] < n / dx["result_t"].size
    assert dx["result_t"][-1] >= n - n / dx["result_t"].size - 1
    assert np.array_equal(dx["result_t"], dy["result_t"])

    gpu = {"name": "x", "cu_count": 256, "max_clock_mhz": 2400,
           "lds_per_cu_kb": 160, "wavefront_size": 64, "hbm_bw_gbps": 5000.0}
    view = bench.caller_view(0, {"gpu": gpu, "served": 9})
    assert view == {"result": 0, "worker_gpu": [256, 2400, 160, 64],
                    "worker_served": 9}
    total = sum(f.stat().st_size for f in (tmp_path / "x").iterdir())
    assert total <= 64 * 10**6


@pytest.mark.gpu
def test_secondary_runs_only_with_full():
    """On a GPU a plain run stops at its headline figure; ``--full`` adds
    the mm and staging secondary runs (fixed step counts, ten 1 GB
    returns among them, hence about ten seconds)."""
    plain = _run_bench()
    assert plain["secondary"] == []
    full = _run_bench("--full")
    assert [s["config"] for s in full["secondary"]] == ["mm", "staging"]
    for sec in full["secondary"]:
        assert sec["electrons_per_sec"] > 0 and sec["p50_ms"] > 0
        assert sec["steps"] > 0
