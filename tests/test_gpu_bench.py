"""bench.py's multi-shard line proves itself:
`--gpus N` on this one-GPU box drives N logical shards with the LOCAL
transport -- the same layouts, halo plan, pack/unpack kernels and
ring / interior / exchange streams as the RCCL path -- and the JSON line must
carry parity_vs_1gpu (the same grid and generations as one shard on GPU 0,
census checksum + live count) and the per-phase timings."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, full=True):
    # more shards than this box has GPUs: an explicit rehearsal
    extra = ["--rehearse-shards"] if "--gpus" in args else []
    # --full: parity_vs_1gpu, the phases and the copy ceiling are not part of a plain run
    extra += ["--full", "--no-cpu-baseline"] if full else []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra, *args],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("kernel", ["bit", "byte"])
def test_strong_scaling_4_shards_full_size(kernel):
    """configs[3] at N = 4: 65536^2 split 2x2 (MPI_Dims_create), LOCAL shards."""
    out = run_bench("--gpus", "4", "--scaling", "strong", "--kernel", kernel, "--steps", "40", "--warmup", "8")
    assert out["scaling"] == "strong"
    # a rehearsal says what it ran on: one GPU, four shards, no RCCL communicator (LOCAL copies)
    c = out["config"]
    assert out["n_gpus"] == 1 and c["shards"] == 4 and c["devices"] == 1 and c["rehearsal"] is True, c
    assert c["rccl_nranks"] == 0 and len(c["pci_bus_ids"]) == 1, c
    assert out["config"]["dims"] == [2, 2] and out["config"]["nx"] == out["config"]["ny"] == 65536
    p = out["parity_vs_1gpu"]
    assert p["ok"] is True and p["live"] > 0, p
    ph = out["phases"]
    assert ph["blocks"] > 0 and ph["block_ms"] > 0 and ph["interior_ms"] > 0 and ph["halo_ms"] > 0


@pytest.mark.parametrize("args", [("--gpus", "2", "--size", "8192", "--steps", "45", "--warmup", "4"),
                                  ("--gpus", "2", "--size", "8192", "--partition", "rows", "--steps", "45",
                                   "--warmup", "4"),
                                  ("--gpus", "3", "--size", "4096", "--partition", "cols", "--steps", "33",
                                   "--warmup", "0"),
                                  ("--gpus", "8", "--scaling", "strong", "--size", "8192", "--steps", "20",
                                   "--warmup", "5", "--parity-seconds", "0")])
def test_multi_shard_bench_parity(args):
    """Weak scaling 2-D (default) / row strips / column strips, and strong 4x2 blocks whose
    parity leg is a fresh 3K+1-generation run (--parity-seconds 0)."""
    out = run_bench(*args)
    p = out["parity_vs_1gpu"]
    assert p["ok"] is True, p
    if "--parity-seconds" in args:
        assert p["same_run"] is False and p["generations"] == 3 * out["config"]["generations_per_exchange"] + 1
    else:
        assert p["same_run"] is True
    assert out["phases"]["blocks"] > 0


def test_weak_scaling_default_is_cartesian_8():
    """configs[4] at N = 8: the weak line's
    default partition is life_cart's MPI_Dims_create {4, 2} -- a 262144 x
    131072 global grid of 65536^2 blocks, four halo peers per block -- and it
    proves itself against the same grid run as one shard."""
    out = run_bench("--gpus", "8", "--scaling", "weak", "--steps", "40", "--warmup", "8")
    assert out["scaling"] == "weak" and out["config"]["dims"] == [4, 2]
    assert (out["config"]["nx"], out["config"]["ny"]) == (262144, 131072)
    assert out["config"]["partition"] == "cart"
    assert out["parity_vs_1gpu"]["ok"] is True, out["parity_vs_1gpu"]
    c = out["call"]  # the host enqueue cost of the 8-shard pass is in the line
    assert c["passes"] == 4 and c["host_enqueue_ms"] >= c["pass_enqueue_max_ms"] > 0, c
    assert 0 < c["device_span_ms"] <= c["elapsed_ms"], c


def test_single_gpu_line_is_valu_roofline():
    """N = 1, temporal bit kernel: the roofline names the binding resource
    (VALU issue) and keeps the HBM figures beside it."""
    out = run_bench("--steps", "32", "--warmup", "16", "--size", "16384")
    r = out["roofline"]
    assert r["bound"] == "valu" and 0 < r["frac"] < 1 and r["unit"] == "Tlane-op/s"
    # achieved = the algorithmic ops of the owned cells (22 per 64-cell pair row and generation); the issued
    # ops (ghost rows, edge lanes) are larger
    updates = r["algorithmic_ops_per_launch"] * 64.0 / 22.0
    assert updates == pytest.approx(16384 * 16384 * r["generations_per_launch"], rel=1e-3)  # rounded to 3 digits
    assert r["issued"]["ops_per_launch"] > r["algorithmic_ops_per_launch"] and r["issued"]["frac"] > r["frac"]
    assert r["hbm"]["achieved"] > 0 and r["hbm"]["peak"] == 8000.0
    assert r["hbm"]["copy_ceiling_GBps"] > 0  # --full measures the stream-copy ceiling
    assert "parity_vs_1gpu" not in out and out["scaling"] == "weak"
    assert out["n_gpus"] == 1 and out["config"]["shards"] == 1 and out["config"]["rehearsal"] is False
    c = out["call"]  # one event pair around the call's launches: span <= the bench clock
    assert c["passes"] == 3 and 0 < c["device_span_ms"] <= c["elapsed_ms"] and c["host_enqueue_ms"] > 0, c


PLAIN_CASES = {  # args, (nx, ny), generations = warmup + steps
    # 4096 rows of 16 KiB as float32 are 64 MiB: cells.npy is the seeded row sample
    "sampled": (("--size", "4096", "--steps", "40", "--warmup", "8"), (4096, 4096), 48),
    # a width that is no multiple of 8 (the last packed byte is partial), the byte kernel, every row
    "odd_byte": (("--shape", "1001x777", "--kernel", "byte", "--steps", "33", "--warmup", "5"), (1001, 777), 38),
    # two 2048^2 blocks side by side (a multi-stream call): the plain line has no statistics run, the dump is
    # the gathered grid
    "two_shards": (("--gpus", "2", "--size", "2048", "--steps", "45", "--warmup", "4"), (4096, 2048), 49),
}


@pytest.mark.parametrize("case", sorted(PLAIN_CASES))
def test_plain_run_is_lean_and_dumps_outputs(case, tmp_path):
    """Without --full the line is the headline only (no cpu_baseline, copy
    ceiling, parity or statistics run), ms_per_step is the timed call over
    --steps, and --dump-outputs writes the grid after warmup + steps
    generations: bit-exact against the oracle, in float arrays of bounded size."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    args, (nx, ny), gens = PLAIN_CASES[case]
    out = run_bench(*args, "--dump-outputs", str(tmp_path / "dump"), full=False)
    steps = int(args[args.index("--steps") + 1])
    assert out["steps"] == steps and out["value"] > 0 and out["higher_is_better"] is True
    assert out["ms_per_step"] == pytest.approx(out["call"]["elapsed_ms"] / steps, abs=1e-4)
    # value and elapsed_ms are rounded to 3 and 4 decimals
    ms = out["call"]["elapsed_ms"]
    assert out["value"] == pytest.approx(nx * ny * steps / (ms * 1e-3) / 1e9, rel=5e-5 / ms + 5e-4 / out["value"] + 1e-9)
    assert (out["config"]["nx"], out["config"]["ny"]) == (nx, ny)
    for key in ("cpu_baseline", "parity_vs_1gpu", "phases"):
        assert key not in out
    if case == "two_shards":
        assert "roofline" not in out
    else:
        hbm = out["roofline"].get("hbm", out["roofline"])
        assert hbm["copy_ceiling_GBps"] is None and hbm["frac_of_copy_ceiling"] is None

    want = O.life_run(O.fill_random(nx, ny, 1, 0.5), gens, 8)
    files = {f[:-4]: np.load(tmp_path / "dump" / f) for f in sorted(os.listdir(tmp_path / "dump"))}
    assert sorted(files) == ["cells", "cells_rows", "checksum", "live_count", "row_population"]
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())
    assert sum(os.path.getsize(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")) <= 64 << 20
    rows = files["cells_rows"].astype(np.int64)
    assert len(rows) == (2048 if case == "sampled" else ny) and np.all(np.diff(rows) > 0) and rows[-1] < ny
    np.testing.assert_array_equal(files["cells"], want[rows].astype(np.float32))
    np.testing.assert_array_equal(files["row_population"], want.sum(axis=1, dtype=np.int64))
    assert int(files["live_count"]) == int(want.sum()) == out["config"]["live_cells_end"]
    census = O.checksum(want)
    assert [int(v) for v in files["checksum"]] == [census >> 32, census & 0xFFFFFFFF]
