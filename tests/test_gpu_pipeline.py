"""Pipelined passes (LIFE_OPT_PIPELINE, life_step.hip pipelined_pass): a pass
of the per-launch tiles cut into R row regions, one launch each, alternating
between the shard's two compute streams and ordered by events.  Forced here
(the automatic rule wants several rounds of tiles per region), with the
dataflow form and the small-grid kernels off, and compared cell by cell with
the oracle.

Shapes: the smallest tile grids that still have a plan (at least 2 tile rows
per region) and hold the edges of the schedule:

* 4160 x 1400 bit: two tile columns, the last one banded with 3 owned pairs
  (8 tile rows per banded item); 9 tile rows, regions of 3, 2, 2, 2 at R = 4.
  61 generations are passes of 11, 10, 10, 10, 10, 10: the pass length, and
  with it the tile grid, changes inside the call (both streams joined, the
  rotation restarted), and the run of equal passes rotates once round and past.
* 3968 x 1349 bit: one tile column.  48 generations are 4 passes of 12: the
  last of 9 tile rows has 5 rows, fewer than the 12 ghost rows, so tile row
  0's window reaches two tile rows up.  37 generations are passes of 10, 9, 9,
  9 over 8 tile rows.
* 2048 x 1984 byte, R = 3: 7 tile rows of 320 owned rows, two passes of 20.
* 4096 x 1000: 6 tile rows, no plan at R = 4: whole launches, same result.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}


def reference(oracle, nx, ny, seed, gens):
    """oracle.life_run of fill_random(seed) after `gens` generations, computed once per module run."""
    key = (nx, ny, seed)
    if key not in _CACHE:
        _CACHE[key] = {0: oracle.fill_random(nx, ny, seed, 0.5)}
    have = _CACHE[key]
    if gens not in have:
        base = max(g for g in have if g <= gens)
        have[gens] = oracle.life_run(have[base], gens - base, threads=8)
        have[gens].setflags(write=False)
    return have[gens]


def pipelined(gpu, nx, ny, kernel, R):
    life = gpu.Life(nx, ny, kernel=kernel, small_grid=False, flow=0)
    life.configure(gpu.OPT_PIPELINE, R)
    return life


def pass_sizes(gens, bmax):
    sizes = []
    while gens:
        n = -(-gens // bmax)
        sizes.append(-(-gens // n))
        gens -= sizes[-1]
    return sizes


@pytest.mark.parametrize("R", [3, 4])
@pytest.mark.parametrize("nx,ny,gens", [(4160, 1400, 61), (3968, 1349, 37), (3968, 1349, 48)])
def test_bit_regions_match_oracle(gpu, oracle, nx, ny, gens, R):
    with pipelined(gpu, nx, ny, "bit", R) as life:
        life.upload(reference(oracle, nx, ny, 3, 0))
        life.step(gens)
        assert life.last_path() == "tiles"
        want = reference(oracle, nx, ny, 3, gens)
        np.testing.assert_array_equal(life.gather(), want)
        assert life.live_count() == int(want.sum())


def test_bit_regions_on_poisoned_buffers(gpu, oracle, monkeypatch):
    """LIFE_POISON is read at every creation (tests/test_gpu_poison.py sets it the same way): a row no
    region launch wrote, or one read before its writer finished, comes back as 0xA5 cells."""
    monkeypatch.setenv("LIFE_POISON", "1")
    nx, ny, gens = 4160, 1400, 61
    for R in (3, 4):
        with pipelined(gpu, nx, ny, "bit", R) as life:
            life.upload(reference(oracle, nx, ny, 3, 0))
            life.step(gens)
            np.testing.assert_array_equal(life.gather(), reference(oracle, nx, ny, 3, gens))


def test_byte_regions_match_oracle(gpu, oracle):
    nx, ny, gens = 2048, 1984, 40
    with pipelined(gpu, nx, ny, "byte", 3) as life:
        life.upload(reference(oracle, nx, ny, 5, 0))
        life.step(gens)
        assert life.last_path() == "tiles"
        np.testing.assert_array_equal(life.gather(), reference(oracle, nx, ny, 5, gens))


def test_ordering_around_a_pipelined_call(gpu, oracle):
    """What precedes and follows the call on the compute stream stays ordered with the launches on the
    second stream: the fill before it, the census behind it, the next call."""
    nx, ny = 4160, 1400
    with pipelined(gpu, nx, ny, "bit", 4) as life:
        life.fill_random(3, 0.5)  # asynchronous: no sync before the step
        life.step(25)
        want = reference(oracle, nx, ny, 3, 25)
        assert life.live_count() == int(want.sum())  # the census right behind the call
        assert life.checksum() == oracle.checksum(want)
        np.testing.assert_array_equal(life.gather(), want)
        life.step(25)
        life.step(25)  # two calls back to back
        want = reference(oracle, nx, ny, 3, 75)
        assert life.checksum() == oracle.checksum(want)
        np.testing.assert_array_equal(life.gather(), want)


def test_no_plan_runs_whole_launches(gpu, oracle):
    """6 tile rows cannot hold 4 regions of 2: one launch per pass, as with the option off -- the same
    cells and the same booked work (two tile columns, the second banded: 6 + 1 items)."""
    nx, ny, gens = 4096, 1000, 36
    got = {}
    for R in (0, 4):
        with pipelined(gpu, nx, ny, "bit", R) as life:
            life.upload(reference(oracle, nx, ny, 9, 0))
            life.set_timing(True)
            life.step(gens)
            got[R] = (life.kernel_stats()[1:], life.kernel_work(), life.call_stats()["passes"])
            np.testing.assert_array_equal(life.gather(), reference(oracle, nx, ny, 9, gens))
    assert got[0] == got[4] and got[4][2] == 3


def test_call_pair_books_one_launch_per_pass(gpu, oracle):
    """Under the one event pair per call a pipelined pass counts as ONE launch of the whole grid: its
    compulsory bytes and cell-updates, and the VALU work as tiled -- 9 full tiles and, in regions of 3, 2,
    2, 2 tile rows, 4 banded items per pass (a whole launch has ceil(9 / 8) = 2: the regions are there).
    (The suite's A/B runs: without bands 18 tiles either way; LIFE_TIMING_MODE 1 / 2 run whole launches,
    3 books nothing.)"""
    mode = os.environ.get("LIFE_TIMING_MODE", "0")
    items = 18 if os.environ.get("LIFE_BANDS", "1") == "0" else 9 + (4 if mode in ("0", "3") else 2)
    nx, ny, gens = 4160, 1400, 61
    sizes = pass_sizes(gens, gpu.BLOCK_GENS["bit"])
    assert sizes == [11, 10, 10, 10, 10, 10]
    with pipelined(gpu, nx, ny, "bit", 4) as life:
        life.upload(reference(oracle, nx, ny, 3, 0))
        life.set_timing(True)
        life.step(gens)
        ms, n, b = life.kernel_stats()
        upd, valu = life.kernel_work()
        assert life.call_stats()["passes"] == len(sizes)
        if mode == "3":
            assert (n, b, upd, valu) == (0, 0.0, 0.0, 0.0)
        else:
            assert n == len(sizes) and ms > 0
            assert b == pytest.approx(nx * ny * 0.25)
            assert n * upd == pytest.approx(nx * ny * gens)
            R, NW = gpu.TEMPORAL_ROWS["bit"], gpu.TILE_WAVES["bit"]
            assert n * valu == pytest.approx(sum(items * 64 * NW * R * 22 * m for m in sizes))
        np.testing.assert_array_equal(life.gather(), reference(oracle, nx, ny, 3, gens))


def test_automatic_rule_engages_on_a_large_grid(gpu):
    """32768 x 65536 bit with the dataflow form off: 4.3 rounds of resident workgroups per pass and 5
    passes, so the automatic rule (4 regions, each at least one round, at least 4 passes) pipelines.  The
    same census as with the option off; the booked VALU work differs, since region launches split no
    half-height tail (with LIFE_TIMING_MODE 1 / 2 both run whole launches; with 3 nothing is booked)."""
    nx, ny, gens = 32768, 65536, 50
    got = {}
    for value in (0, 1):
        with pipelined(gpu, nx, ny, "bit", value) as life:
            life.fill_random(11, 0.5)
            life.set_timing(True)
            life.step(gens)
            got[value] = (life.checksum(), life.live_count(), life.kernel_stats()[1], life.kernel_work()[1])
    assert got[0][:3] == got[1][:3] and got[0][1] > 0
    if os.environ.get("LIFE_TIMING_MODE", "0") == "0":
        assert got[0][2] == 5 and got[0][3] != got[1][3]


_PER_LAUNCH = r"""
import sys
sys.path.insert(0, {pkg!r})
import life_mi355x as lm
with lm.Life(4160, 1400, kernel="bit", small_grid=False, flow=0) as life:
    life.configure(lm.OPT_PIPELINE, 4)
    life.fill_random(3, 0.5)
    life.set_timing(True)
    life.step(61)
    ms, n, b = life.kernel_stats()
    assert n == 6 and ms > 0 and abs(b - 4160 * 1400 * 0.25) < 1, (n, ms, b)
    print("PER_LAUNCH", life.checksum(), life.live_count(), flush=True)
"""


@pytest.mark.parametrize("mode", ["1", "2"])
def test_per_launch_timing_runs_whole_launches(gpu, oracle, mode):
    """LIFE_TIMING_MODE 1 / 2 (read when the library loads: a child process) give every launch its own
    event pair or dispatch stamps; overlapping kernels have no time of their own, so each pass runs as
    one timed launch, with the same result."""
    from conftest import ROOT

    env = dict(os.environ, LIFE_TIMING_MODE=mode)
    out = subprocess.run([sys.executable, "-c", _PER_LAUNCH.format(pkg=os.path.join(ROOT, "mpi-and-open-mp_amd"))],
                         env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0 and "PER_LAUNCH" in out.stdout, out.stdout + out.stderr
    want = reference(oracle, 4160, 1400, 3, 61)
    assert out.stdout.split()[-2:] == [str(oracle.checksum(want)), str(int(want.sum()))]
