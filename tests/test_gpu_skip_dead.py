"""Skip-dead passes (LIFE_OPT_SKIP_DEAD, life_step.hip step_skip): a pass runs
only the tiles whose input window may hold a live cell, clears the blocks the
destination buffer may still hold alive, and skips the rest.  Compared with
the oracle over the WHOLE grid (a stale or garbage block anywhere shows), with
the live count, and with last_path() == "skip".

The grid is 8192 x 700 bit with the small-grid kernels off: three tile
columns of 62, 62 and 4 pairs; at 12 generations per pass five tile rows of
168 rows, the last partial -- the smallest grid with an interior tile, a
narrow last column and both wraps.  61 generations run as passes of 11, 10,
10, 10, 10, 10 (tile rows of 170 and 172 rows): the tile grid changes inside
the call, the map's granularity does not.
"""
import os
import subprocess

import numpy as np
import pytest

import rule_ref
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NX, NY = 8192, 700
DRIVER = os.path.join(ROOT, "mpi-and-open-mp_amd", "driver", "life_mi355x")
GLIDER = np.array([(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)], np.int64)  # heading south-east, +1, +1 per 4 generations
BLINKER = np.array([(0, 0), (1, 0), (2, 0)], np.int64)


def grid_of(cells, nx=NX, ny=NY):
    g = np.zeros((ny, nx), np.uint8)
    c = np.asarray(cells, np.int64)
    g[c[:, 1] % ny, c[:, 0] % nx] = 1
    return g


def skipping(gpu, nx=NX, ny=NY, **kw):
    return gpu.Life(nx, ny, kernel="bit", small_grid=False, skip_dead=True, **kw)


def check(life, want):
    """The whole grid, the live count and the path."""
    assert life.last_path() == "skip"
    np.testing.assert_array_equal(life.gather(), want)
    assert life.live_count() == int(want.sum())


# ------------------------------------------------------------ 1. a glider across the tile corners
@pytest.mark.parametrize("x0,y0", [(3960, 160), (8184, 696)], ids=["tile-corner", "periodic-corner"])
def test_glider_across_the_corners(gpu, oracle, x0, y0):
    """North-west of the tile corner (3968, 168), then of the periodic corner (8191, 699); 61
    generations move it 15 cells south-east, across the corner.  Its window belongs to two tile rows
    and two tile columns at most: the third tile column reads one edge pair of each of the other
    two, the tile row above the 20-row (m = 11) or 12-row last one stops short of it."""
    cells = GLIDER + (x0, y0)
    want = oracle.life_run(grid_of(cells), 61, threads=8)
    assert want.sum() == 5
    with skipping(gpu) as life:
        life.clear()
        life.set_cells(cells)
        life.step(61)
        passes, run, cleared, total = life.activity()
        print(f"glider at ({x0}, {y0}): passes {passes} run {run} cleared {cleared} total {total}")
        check(life, want)
        assert passes == 6 and total == 3 * 5 + 5 * 3 * 5
        assert 0 < run <= 4 * passes and run < total


# ------------------------------------------------------------ 2. a pattern that dies
def test_domino_dies_and_does_not_come_back(gpu):
    """Two cells in an interior tile die at generation 1.  The second pass of step(24) writes into the
    buffer that still holds them and runs no tile: without the clear class they would be back."""
    with skipping(gpu) as life:
        life.clear()
        life.set_cells([(5000, 300), (5001, 300)])
        life.step(24)
        passes, run, cleared, total = life.activity()
        print(f"domino: passes {passes} run {run} cleared {cleared} total {total}")
        check(life, np.zeros((NY, NX), np.uint8))
        assert life.live_count() == 0
        assert passes == 2 and cleared >= 1 and run <= 4


# ------------------------------------------------------------ 3. a fresh device whose buffers hold 0xA5
def test_fresh_device_under_poison(gpu, oracle, monkeypatch):
    """LIFE_POISON is read at creation (tests/test_gpu_pipeline.py sets it the same way).  After one
    pass the result lies in the buffer that was never written: every block of it is run or cleared."""
    monkeypatch.setenv("LIFE_POISON", "1")
    soup = oracle.fill_random(512, 300, 11, 0.5)
    g0 = np.zeros((NY, NX), np.uint8)
    g0[168 - 150:168 + 150, 3968 - 256:3968 + 256] = soup  # straddles the tile corner (3968, 168)
    with skipping(gpu) as life:
        life.clear()
        life.set_rect(3968 - 256, 168 - 150, soup)
        life.step(12)
        want = oracle.life_run(g0, 12, threads=8)
        check(life, want)
        life.step(49)
        check(life, oracle.life_run(want, 49, threads=8))


# ------------------------------------------------------------ 4. edits between step calls
def test_edits_between_step_calls(gpu, oracle):
    """After step(24) of a glider in tile (0, 0) the map holds every other block as dead; each edit puts
    live cells into such a block, and the next step(24) must see them."""
    with skipping(gpu) as life:
        life.clear()
        life.set_cells(GLIDER + (100, 40))
        g = grid_of(GLIDER + (100, 40))

        def advance():
            nonlocal g
            life.step(24)
            g = oracle.life_run(g, 24, threads=8)
            check(life, g)

        advance()
        far = BLINKER + (6000, 500)  # tile (1, 2)
        life.set_cells(far)
        g[far[:, 1], far[:, 0]] = 1
        advance()
        patch = oracle.fill_random(40, 30, 5, 0.4)
        life.set_rect(7000, 350, patch)
        g[350:380, 7000:7040] = patch
        advance()
        g = grid_of(np.concatenate([GLIDER + (8150, 650), BLINKER + (4100, 20)]))
        life.upload_bits(np.packbits(g, axis=1, bitorder="little"))
        advance()
        life.clear()
        life.set_cells(GLIDER + (2000, 400))
        g = grid_of(GLIDER + (2000, 400))
        advance()
        life.fill_random(9, 0.02)
        g = oracle.fill_random(NX, NY, 9, 0.02)
        advance()


# ------------------------------------------------------------ 5. the option toggled
def test_toggle(gpu, oracle):
    g = grid_of(np.concatenate([GLIDER + (3960, 160), BLINKER + (7000, 600)]))
    with skipping(gpu) as life:
        life.upload(g)
        life.step(24)
        g = oracle.life_run(g, 24, threads=8)
        check(life, g)
        life.configure(gpu.OPT_SKIP_DEAD, 0)
        life.step(24)
        g = oracle.life_run(g, 24, threads=8)
        assert life.last_path() != "skip"
        assert life.activity() == (0, 0, 0, 0)
        np.testing.assert_array_equal(life.gather(), g)
        life.configure(gpu.OPT_SKIP_DEAD, 1)
        life.step(24)
        g = oracle.life_run(g, 24, threads=8)
        check(life, g)


# ------------------------------------------------------------ 6. nothing to skip
def test_dense_soup_runs_every_tile(gpu, oracle):
    g = oracle.fill_random(NX, NY, 3, 0.5)
    with skipping(gpu) as life:
        life.configure(gpu.OPT_BLOCK_GENS, 5)
        life.fill_random(3, 0.5)
        for gens in (61, 7, 1):
            life.step(gens)
            g = oracle.life_run(g, gens, threads=8)
            passes, run, cleared, total = life.activity()
            print(f"soup step({gens}): passes {passes} run {run} cleared {cleared} total {total}")
            check(life, g)
            assert passes == -(-gens // 5) and run == total and cleared == 0


# ------------------------------------------------------------ 7. a last tile row shorter than m
def test_short_last_tile_row(gpu, oracle):
    """3968 x 1349: one tile column, nine tile rows at 12 generations per pass, the last 5 rows tall: tile
    row 0's window reaches two tile rows up.  Cells in tile row 0, in the last tile row, and in the
    rows of the tile row before it that only tile row 0's window wrap reaches."""
    nx, ny = 3968, 1349
    cells = np.concatenate([GLIDER + (30, 2), GLIDER + (2000, 1345), BLINKER + (3000, 1339), GLIDER + (3950, 1330),
                            GLIDER + (500, 700)])
    g = grid_of(cells, nx, ny)
    with skipping(gpu, nx, ny) as life:
        life.clear()
        life.set_cells(cells)
        life.step(48)
        want = oracle.life_run(g, 48, threads=8)
        check(life, want)
        passes, run, cleared, total = life.activity()
        assert passes == 4 and total == 4 * 9 and run < total


# ------------------------------------------------------------ 8. another rule
def test_highlife(gpu):
    """B36/S23 runs the table-rule instance: a soup window and a replicator."""
    rule = rule_ref.NAMED["B36/S23"]
    g = np.zeros((NY, NX), np.uint8)
    g[100:260, 3900:4100] = rule_ref.soup(200, 160, 4, 0.4)
    rep = np.array([[0, 0, 1, 1, 1], [0, 1, 0, 0, 1], [1, 0, 0, 0, 1], [1, 0, 0, 1, 0], [1, 1, 1, 0, 0]], np.uint8)
    g[600:605, 8000:8005] = rep
    with skipping(gpu, rule="B36/S23") as life:
        life.upload(g)
        life.step(37)
        want = rule_ref.rule_run(g, 37, rule)
        check(life, want)
        assert want[550:, 7900:].any()
        passes, run, cleared, total = life.activity()
        assert passes == 4 and 0 < run < total


# ------------------------------------------------------------ 9. devices that do not qualify
@pytest.mark.parametrize("nx,ny,kw", [(512, 300, dict(kernel="byte", small_grid=False)),
                                      (512, 300, dict(kernel="bit", small_grid=False, shards=2)),
                                      (8200, 300, dict(kernel="bit", small_grid=False)),
                                      (500, 500, dict(kernel="bit", small_grid=True))],
                         ids=["byte", "two-shards", "width-8200", "small-grid"])
def test_devices_that_do_not_qualify(gpu, oracle, nx, ny, kw):
    """The option is accepted and has no effect: the oracle's result on today's path."""
    if kw.get("shards", 1) > 1:
        kw = dict(kw, transport=gpu.XPORT_LOCAL)
    g = oracle.fill_random(nx, ny, 7, 0.3)
    want = oracle.life_run(g, 13, threads=4)
    paths = []
    for on in (False, True):
        with gpu.Life(nx, ny, skip_dead=on, **kw) as life:
            life.upload(g)
            life.step(13)
            np.testing.assert_array_equal(life.gather(), want)
            assert life.live_count() == int(want.sum())
            assert life.activity() == (0, 0, 0, 0)
            paths.append(life.last_path())
            if on:
                with pytest.raises(gpu.LifeError):
                    life.configure(gpu.OPT_SKIP_DEAD, 2)
    assert paths[0] == paths[1] != "skip"


def test_bad_value_on_a_device_that_qualifies(gpu):
    with skipping(gpu) as life:
        for v in (2, -1):
            with pytest.raises(gpu.LifeError):
                life.configure(gpu.OPT_SKIP_DEAD, v)


def test_timing_books_one_launch_per_pass(gpu, oracle):
    """Timing on: a pass is one timed launch, the whole grid's cell-updates, no bytes and no VALU ops (the
    host does not know how many tiles ran); the results do not change, nor does a rule change between
    calls drop the maps' validity (the second call still skips)."""
    g = grid_of(GLIDER + (100, 40))
    with skipping(gpu) as life:
        life.clear()
        life.set_cells(GLIDER + (100, 40))
        life.set_timing(True)
        life.step(24)
        ms, launches, nbytes = life.kernel_stats()
        updates, valu = life.kernel_work()
        assert launches == 2 and ms > 0 and nbytes == 0 and valu == 0
        assert updates == NX * NY * 12
        life.set_timing(False)
        life.set_rule("B3/S23")
        life.step(24)
        passes, run, cleared, total = life.activity()
        assert passes == 2 and run <= 2 * passes and cleared == 0
        check(life, oracle.life_run(g, 48, threads=8))


# ------------------------------------------------------------ 10. full scale, no oracle
def test_full_scale_glider_crosses_the_periodic_corner(gpu):
    """65536^2: 17 x 391 tiles per pass.  The glider starts 60 cells north-west of the periodic corner
    and ends 60 cells south-east of it after 480 generations (120 cells, the same phase)."""
    n = 65536
    with skipping(gpu, n, n) as life:
        life.clear()
        life.set_cells(GLIDER + (n - 60, n - 60))
        life.step(480)
        assert life.last_path() == "skip"
        passes, run, cleared, total = life.activity()
        print(f"65536^2 glider: passes {passes} run {run} cleared {cleared} total {total}")
        assert life.live_count() == 5
        want = np.zeros((12, 12), np.uint8)
        want[GLIDER[:, 1] + 4, GLIDER[:, 0] + 4] = 1
        np.testing.assert_array_equal(life.gather_rect(56, 56, 12, 12), want)
        assert passes == 40 and total == 40 * 17 * 391
        assert 0 < run <= 4 * passes


# ------------------------------------------------------------ 11. the driver
def test_driver_flag_writes_the_same_frames(gpu, tmp_path):
    def run(cwd, *extra):
        os.makedirs(cwd)
        r = subprocess.run([DRIVER, os.path.join(GOLDEN, "cfg", "p46gun_big.cfg"), "--nx", str(NX), "--ny", str(NY),
                            "--steps", "92", "--save-steps", "46", "--format", "bits", "--live", *extra], cwd=cwd,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        vtk = os.path.join(cwd, "vtk")
        return {f: open(os.path.join(vtk, f), "rb").read() for f in sorted(os.listdir(vtk))}, r.stderr

    plain, live0 = run(str(tmp_path / "plain"))
    skip, live1 = run(str(tmp_path / "skip"), "--skip-dead")
    assert len(plain) == 2 and skip == plain and live0 == live1
    assert any(b for b in plain[sorted(plain)[-1]][64:])
