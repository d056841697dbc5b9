"""The second tile shape on every launch form: bit tiles of 16 register rows
per wave (windows of 8 x 16 = 128 rows, T = 128 - 2m owned rows) and byte
tiles of 32 (256-row windows), selected by life_tune_temporal /
LIFE_TEMPORAL_ROWS.  Every tile kernel family is compiled for both shapes
(life_kernels.hip LIFE_BIT_SHAPES); the rest of the suite runs the default one
(24 / 48 rows) everywhere but in test_temporal_tile_heights_agree.

The shape is no cosmetic parameter.  With 16-row waves the ghost depth exceeds
a wave's rows from m = 17 on, so whole waves of a window are ghost (tile_body_bit
r0 / r1), as they already are at m = 12 in a half-height tile (8 rows per
wave); at m = 32 a tile owns 64 rows and a half tile none, so no tail may be
planned; T = 104, 106, 108 ... is another alignment against the activity map's
32-row words, and a wave of a skip-dead tile stores 16 rows into its two map
rows.

Every case is compared cell by cell over the whole grid with oracle.life_run
(B3/S23) or rule_ref.rule_run (other rules), with live_count(), and shows the
launch form that ran through last_path(), activity() or the booked VALU work
(items x 64 lanes x 8 waves x R rows x 22 m: R and T = 8R - 2m enter it, so it
tells the shapes apart).  The one exception is the half-height tail, which
needs a launch of more than one round of workgroups: it is pinned on a band
around the x = 0 seam, as test_gpu_band_split.py does at the default shape.

The setting is process-wide: the `tile_rows` fixture restores the default
after each test, also on failure, and the module's last test checks through
the booked work that the default shape is back.

Two more cases at the default shape belong to the same work: a dataflow call
whose last tile row is shorter than m (tflow_kernel's wait on tile rows ty - 2
and ty + 2), and skip-dead maps whose last column holds one pair, that are one
pair wide in all, or lower than one 32-row map row.
"""
import os
import subprocess

import numpy as np
import pytest

import rule_ref
import test_gpu_band_split as bs
import test_gpu_rule as tr
from conftest import ROOT

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")
GLIDER = np.array([(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)], np.int64)  # heading south-east, +1, +1 per 4 generations
BLINKER = np.array([(0, 0), (1, 0), (2, 0)], np.int64)
HIGHLIFE, DAYNIGHT = rule_ref.NAMED["B36/S23"], rule_ref.NAMED["B3678/S34678"]


@pytest.fixture
def tile_rows(gpu, request):
    """(kernel, rows): that encoding's tiles at `rows` register rows per wave for one test."""
    kernel, rows = request.param
    gpu.tune_temporal(rows, kernel)
    try:
        yield rows
    finally:
        gpu.tune_temporal(gpu.TEMPORAL_ROWS[kernel], kernel)


def shape(*shapes):
    return pytest.mark.parametrize("tile_rows", shapes, indirect=True, ids=[f"{k}{r}" for k, r in shapes])


BIT16, BYTE32, BIT24_16 = shape(("bit", 16)), shape(("byte", 32)), shape(("bit", 24), ("bit", 16))


def lane_ops(items, m, rows=16, per_pair_row=22):
    return items * 64 * 8 * rows * per_pair_row * m


def tile_rows_of(ny, m, rows=16):
    return -(-ny // (8 * rows - 2 * m))


def check(life, want, path):
    """The whole grid, the live count and the path."""
    assert life.last_path() == path
    np.testing.assert_array_equal(life.gather(), want)
    assert life.live_count() == int(want.sum())


def grid_of(cells, nx, ny):
    g = np.zeros((ny, nx), np.uint8)
    c = np.asarray(cells, np.int64)
    g[c[:, 1] % ny, c[:, 0] % nx] = 1
    return g


_rule_refs = {}


def rule_reference(nx, ny, seed, rule, gens):
    """rule_ref.rule_run of rule_ref.soup(seed) after `gens` generations, computed once per module run."""
    have = _rule_refs.setdefault((nx, ny, seed, rule), {0: rule_ref.soup(nx, ny, seed)})
    if gens not in have:
        base = max(g for g in have if g <= gens)
        have[gens] = rule_ref.rule_run(have[base], gens - base, rule)
        have[gens].setflags(write=False)
    return have[gens]


# ------------------------------------------------------------ whole launches, banded and split last columns
NY = 1765  # 17 tile rows at m = 12 (T 104, the last 101 rows) and at m = 11 (T 106, the last 69): a G = 4 item of
#            16 tile rows once full, once partial


def run_whole(gpu, oracle, nx, ny, calls, bmax=None):
    """bs.run_whole at 16 rows: per-launch tiles, the booked work of ceil(ny / (128 - 2m)) tile rows of
    16-row waves per pass; `calls`: the generations of each step call."""
    done, want_ops = 0, 0.0
    with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=0) as life:
        if bmax:
            life.configure(gpu.OPT_BLOCK_GENS, bmax)
        life.upload(bs.reference(oracle, nx, ny, 5, 0))
        life.set_timing(True)
        for gens in calls:
            life.step(gens)
            done += gens
            check(life, bs.reference(oracle, nx, ny, 5, done), "tiles")
            sizes = bs.pass_sizes(gens, bmax or 12)
            want_ops += sum(lane_ops(bs.items_of(nx, tile_rows_of(ny, m)), m) for m in sizes)
            # (a width of whole pairs runs one timed launch per pass; any other wraps through its own apron)
            if bs.MODE != "3" and nx % 64 == 0:
                print(f"{nx} x {ny}: passes {sizes}, booked {bs.booked(life):.0f}, want {want_ops:.0f}")
                assert bs.booked(life) == pytest.approx(want_ops)


@BIT16
@pytest.mark.parametrize("nx", bs.WIDTHS)
def test_whole_launches_match_oracle(gpu, oracle, tile_rows, nx):
    """23 generations: passes of 12 and 11, 17 tile rows each."""
    assert (tile_rows_of(NY, 12), tile_rows_of(NY, 11)) == (17, 17) and NY - 16 * 104 == 101 and NY - 16 * 106 == 69
    run_whole(gpu, oracle, nx, NY, [23])


@BIT16
def test_whole_launches_on_poisoned_buffers(gpu, oracle, tile_rows, monkeypatch):
    """a pair or a row no item stored comes back as 0xA5 cells"""
    monkeypatch.setenv("LIFE_POISON", "1")
    run_whole(gpu, oracle, 6016, NY, [23])


# ------------------------------------------------------------ ghost rows deeper than a wave
@BIT16
@pytest.mark.parametrize("bmax", [16, 17, 32])
def test_ghost_deeper_than_a_wave(gpu, oracle, tile_rows, bmax):
    """4160 x 700 (a full tile column and a banded one of 3 pairs), bmax + 1 generations as a call of bmax and a
    call of 1: two passes of different m, the first with bmax ghost rows at each end of a 128-row window --
    one whole wave at 16, one and a row at 17, two at 32 (T = 64) -- the second with one.  Then one call of
    bmax + 1 generations, which is cut into two passes of about half of it each (9 + 8, 9 + 9, 17 + 16: at
    17 still more ghost rows than a wave has)."""
    assert bs.pass_sizes(bmax, bmax) == [bmax]
    assert bs.pass_sizes(bmax + 1, bmax) == [bmax // 2 + 1, bmax + 1 - (bmax // 2 + 1)]
    run_whole(gpu, oracle, 4160, 700, [bmax, 1, bmax + 1], bmax)


# ------------------------------------------------------------ the half-height tail: 8 rows per wave
TAIL_HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include "life_host.h"
// argv: W m R slots hmax: the smallest height h <= hmax of a W-pair-wide shard whose whole launch of R-row
// tiles at m generations per pass gets a half-height tail from life::tail_plan: "h nty F n2" (zeros: none)
int main(int argc, char **argv) {
    const long long W = atoll(argv[1]), m = atoll(argv[2]), R = atoll(argv[3]), slots = atoll(argv[4]),
                    hmax = atoll(argv[5]);
    const long long ntx = (W + 61) / 62, o = W - 62 * (ntx - 1), T = 8 * R - 2 * m, T2 = 8 * (R / 2) - 2 * m;
    const life::BandSplit sp = life::band_split(o);
    life::BandRows b;
    for (b.n = 0; b.n < sp.n; b.n++) b.B[b.n] = 64 >> sp.b[b.n].gsh;
    const long long nfull = ntx - (b.n > 0 ? 1 : 0);
    for (long long h = 1; h <= hmax; h++) {
        const long long nty = (h + T - 1) / T;
        if (life::tail_row_items(nfull, b, nty) <= slots) {  // one round or less is left whole: the next tile row
            h = nty * T;
            continue;
        }
        const life::TailPlan p = life::tail_plan(nfull, b, 0, nty, h, T, T2, slots, 2, 0.06);
        if (p.F < nty) {
            printf("%lld %lld %lld %lld\n", h, nty, (long long)p.F, (long long)p.n2);
            return 0;
        }
    }
    printf("0 0 0 0\n");
    return 0;
}
"""
# resident workgroups of the 16-row B3/S23 tiles on an MI355X: 256 CUs x 4 (60 VGPRs: 8 waves per SIMD; 40 KiB
# of LDS each); the 24-row tiles have 3 per CU.  (A wrong figure here fails the booked-work assertion below.)
SLOTS16 = 1024


@pytest.fixture(scope="module")
def tail_shape(tmp_path_factory):
    """(h, nty, F, n2): the smallest height of a 6016-wide shard (94 pairs: one full tile column, sub-columns
    of 30 and 2 pairs) with a half-height tail at m = 12 and 16-row tiles, from life::tail_plan itself (the
    g++ harness of tests/test_tail_plan.py)."""
    d = tmp_path_factory.mktemp("tailshape")
    (d / "h.cpp").write_text(TAIL_HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    str(d / "h.cpp"), os.path.join(CSRC, "life_plan.cpp"), "-o", str(exe)], check=True)

    def ask(m):
        return tuple(map(int, subprocess.run([str(exe), "94", str(m), "16", str(SLOTS16), "200000"], check=True,
                                             capture_output=True, text=True).stdout.split()))

    assert ask(32) == (0, 0, 0, 0)  # T2 = 0: no half tile at m = 32, whatever the height
    return ask(12)


@BIT16
def test_half_height_tail_band_vs_oracle(gpu, oracle, tile_rows, tail_shape):
    """6016 x the smallest height with a tail: more than one round of the 1024 resident workgroups, so the
    bottom tile row runs as half-height tiles, 8 rows per wave under 12 ghost rows: the first and the last
    wave of each are all ghost, the second and the seventh hold 4 owned rows.  Pinned to the oracle on a
    full-height band around the x = 0 seam that holds the whole last tile column (pairs 62..93: both
    sub-columns, their seam and the tile column left of them) and the wrap; the band's cut edges are wrong
    by at most a cell per generation.  Then the same grid in one pass of 32 generations: T2 = 0, whole tiles
    only."""
    nx, left, right, margin = 6016, 2048 + 64, 64, 32
    ny, nty, F, n2 = tail_shape
    print(f"tail shape: height {ny}, {nty} tile rows, {F} full, {n2} half-height tile rows")
    assert ny > 0 and F < nty == tile_rows_of(ny, 12) and n2 == -(-(ny - 104 * F) // 40)
    band = oracle.fill_random_window(nx, nx - left - margin, 0, left + right + 2 * margin, ny, seed=7, density=0.5)
    done = 0
    for bmax, gens in ((12, 24), (32, 32)):
        with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=0) as life:
            life.configure(gpu.OPT_BLOCK_GENS, bmax)
            life.fill_random(7, 0.5)
            life.set_timing(True)
            life.step(gens)
            assert life.last_path() == "tiles"
            got = life.gather_rect(nx - left, 0, left + right, ny)
            work = bs.booked(life)
        band = oracle.life_run(band, gens - done, threads=16)  # (the band after 24, then after 32 generations)
        done = gens
        np.testing.assert_array_equal(got, band[:, margin:margin + left + right])
        if bs.MODE == "3" or not (bs._flag("LIFE_BANDS") and bs._flag("LIFE_BAND_SPLIT")):
            continue
        per_pass = work / lane_ops(1, bmax) / (gens // bmax)
        print(f"m = {bmax}: {per_pass} items per pass booked, {bs.items_of(nx, tile_rows_of(ny, bmax))} whole")
        if bmax == 32:
            assert per_pass == pytest.approx(bs.items_of(nx, tile_rows_of(ny, 32)))
        elif os.environ.get("LIFE_TAIL_SPLIT", "2") == "2":
            # F full tile rows and n2 half rows at half a tile each, every row with both sub-columns
            assert per_pass == pytest.approx(bs.items_of(nx, F) + 0.5 * bs.items_of(nx, n2))
            assert per_pass != pytest.approx(bs.items_of(nx, nty))


# ------------------------------------------------------------ table rules
B3_OFF, S2_OFF = (0x00, 0x0C), (0x08, 0x08)  # rule_ref.conway_flips(): B3/S23 with B3, with S2 flipped


@BIT16
@pytest.mark.parametrize("rule", [B3_OFF, S2_OFF] + [rule_ref.NAMED[k] for k in (
    "B36/S23", "B3678/S34678", "B2/S", "B1357/S1357", "B3/S012345678")], ids=lambda r: f"B{r[0]:03x}S{r[1]:03x}")
def test_table_coverage(gpu, tile_rows, rule):
    """test_gpu_rule.check_table's tile half: step(1), then step(12) from the soup on 200 x 70 that holds
    every (alive, neighbours) pair."""
    assert B3_OFF in rule_ref.conway_flips() and S2_OFF in rule_ref.conway_flips()
    soup = rule_ref.soup(200, 70, tr.SOUP_SEED)
    assert rule_ref.coverage(soup) == rule_ref.ALL_PAIRS
    want = tr.ref(200, 70, tr.SOUP_SEED, rule, (1, 13))
    with gpu.Life(200, 70, kernel="bit", rule=rule) as life:
        assert life.rule == gpu.format_rule(*rule)
        life.upload(soup)
        life.step(1)
        check(life, want[0], "tiles")
        life.step(12)
        check(life, want[1], "tiles")


@BIT16
def test_tile_geometry_under_a_rule(gpu, tile_rows):
    """Day & Night on 4160 x 1400, 25 generations (passes of 9 + 8 + 8): 13 tile rows, banded items."""
    want = tr.ref(*tr.BIG, 5, DAYNIGHT, (25,))[0]
    with gpu.Life(*tr.BIG, kernel="bit", rule="B3678/S34678") as life:
        life.upload(rule_ref.soup(*tr.BIG, 5))
        life.set_timing(True)
        life.step(25)
        check(life, want, "tiles")
        if bs.MODE != "3":
            ops = sum(lane_ops(bs.items_of(4160, tile_rows_of(1400, m)), m, 16, gpu.RULE_VALU_PER_PAIR_ROW)
                      for m in (9, 8, 8))
            assert bs.booked(life) == pytest.approx(ops)


@BIT16
def test_pipelined_passes_under_a_rule(gpu, tile_rows):
    """HighLife, OPT_PIPELINE 4, 48 generations: 4 passes over 14 tile rows in regions of 4, 4, 3, 3."""
    want = tr.ref(*tr.BIG, 5, HIGHLIFE, (48,))[0]
    with gpu.Life(*tr.BIG, kernel="bit", rule=HIGHLIFE) as life:
        life.configure(gpu.OPT_PIPELINE, 4)
        life.upload(rule_ref.soup(*tr.BIG, 5))
        life.set_timing(True)
        life.step(48)
        check(life, want, "tiles")
        if bs.MODE == "0":  # (modes 1 / 2 run whole launches)
            ops = 4 * lane_ops(sum(bs.items_of(4160, r) for r in (4, 4, 3, 3)), 12, 16, gpu.RULE_VALU_PER_PAIR_ROW)
            assert bs.booked(life) == pytest.approx(ops)


# ------------------------------------------------------------ pipelined regions, B3/S23
@BIT16
@pytest.mark.parametrize("ny,rows,regions", [(1400, 14, (4, 4, 3, 3)), (1253, 13, (4, 3, 3, 3))])
def test_pipelined_regions(gpu, oracle, tile_rows, ny, rows, regions):
    """6016 wide, OPT_PIPELINE 4, 48 generations = 4 passes of 12 (T 104).  1400: 14 tile rows; 1253: 12 of
    104 rows and a last one of 5, fewer than m, so tile row 0's window reaches two tile rows up, across a
    region boundary.  The booked items are those of the regions (each lists its own banded items)."""
    nx, gens = 6016, 48
    assert tile_rows_of(ny, 12) == rows == sum(regions)
    with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=0) as life:
        life.configure(gpu.OPT_PIPELINE, 4)
        life.upload(bs.reference(oracle, nx, ny, 5, 0))
        life.set_timing(True)
        life.step(gens)
        check(life, bs.reference(oracle, nx, ny, 5, gens), "tiles")
        if bs.MODE == "0":  # (modes 1 / 2 run whole launches)
            assert sum(bs.items_of(nx, r) for r in regions) != bs.items_of(nx, rows)
            assert bs.booked(life) == pytest.approx(4 * lane_ops(sum(bs.items_of(nx, r) for r in regions), 12))


# ------------------------------------------------------------ the dataflow form
# nx, ny, generations, m (tests/test_gpu_flow.py); the last: T 88, 7 tile rows of 88 and a last one of 9 rows,
# fewer than m: tile row 0 reads the rows of tile row 6 (ty - 2), tile row 6 those of tile row 0 (ty + 2)
FLOW16 = [(2048, 1000, 87, 20), (4032, 600, 90, 21), (1984, 700, 135, 32), (64, 900, 37, 8), (8192, 1500, 61, 12),
          (2048, 625, 87, 20)]


def run_flow(gpu, oracle, nx, ny, gens, m, flow):
    g0 = oracle.fill_random(nx, ny, seed=21, density=0.45)
    want = oracle.life_run(g0, gens, threads=8)
    with gpu.Life(nx, ny, kernel="bit", small_grid=False) as life:
        life.configure(gpu.OPT_FLOW, flow)
        life.configure(gpu.OPT_BLOCK_GENS, m)
        life.upload(g0)
        life.set_timing(True)
        life.step(gens)
        check(life, want, "flow")
        _, launches, _ = life.kernel_stats()
        assert launches >= gens // m  # the passes were timed as one launch each


@BIT16
@pytest.mark.parametrize("flow", [1, 2])
@pytest.mark.parametrize("nx,ny,gens,m", FLOW16)
def test_flow_parity(gpu, oracle, tile_rows, nx, ny, gens, m, flow):
    assert 128 - 2 * m >= m and gens // m >= 4  # the form's conditions (flow_ok, kFlowMinPasses)
    run_flow(gpu, oracle, nx, ny, gens, m, flow)


@BIT24_16
@pytest.mark.parametrize("flow", [1, 2])
def test_flow_short_last_tile_row(gpu, oracle, tile_rows, flow):
    """A last tile row shorter than m under the dataflow form, at either shape: 2048 x 919 at 24 rows (T 152:
    6 tile rows and one of 7 rows), 2048 x 625 at 16 (T 88: 7 and one of 9), m = 20."""
    ny = {24: 919, 16: 625}[tile_rows]
    T = 8 * tile_rows - 40
    assert 0 < ny - (ny // T) * T < 20 and ny // T >= 4
    run_flow(gpu, oracle, 2048, ny, 87, 20, flow)


# ------------------------------------------------------------ skip-dead passes
NX, SY = 8192, 700  # three tile columns of 62, 62 and 4 pairs; 7 tile rows at m = 12: tile corner (3968, 104)


def skipping(gpu, nx=NX, ny=SY, **kw):
    return gpu.Life(nx, ny, kernel="bit", small_grid=False, skip_dead=True, **kw)


@BIT16
@pytest.mark.parametrize("x0,y0", [(3960, 96), (8184, 696)], ids=["tile-corner", "periodic-corner"])
def test_skip_glider_across_the_corners(gpu, oracle, tile_rows, x0, y0):
    """61 generations (passes of 11, 10, 10, 10, 10, 10: T 106 and 108, 7 tile rows each) carry the glider 15
    cells south-east, across the tile corner (3968, 104) or the periodic corner."""
    cells = GLIDER + (x0, y0)
    want = oracle.life_run(grid_of(cells, NX, SY), 61, threads=8)
    assert want.sum() == 5
    with skipping(gpu) as life:
        life.clear()
        life.set_cells(cells)
        life.step(61)
        passes, run, cleared, total = life.activity()
        print(f"glider at ({x0}, {y0}): passes {passes} run {run} cleared {cleared} total {total}")
        check(life, want, "skip")
        assert passes == 6 and total == 6 * 3 * 7
        assert 0 < run <= 4 * passes


@BIT16
def test_skip_fresh_device_under_poison(gpu, oracle, tile_rows, monkeypatch):
    """A 512 x 300 soup over the tile corner (3968, 104) and the y wrap, on buffers that hold 0xA5: after one
    pass the result lies in the buffer that was never written, every block of it run or cleared."""
    monkeypatch.setenv("LIFE_POISON", "1")
    soup = oracle.fill_random(512, 300, 11, 0.5)
    x0, y0 = 3968 - 256, (104 - 150) % SY
    g0 = np.zeros((SY, NX), np.uint8)
    g0[np.ix_((y0 + np.arange(300)) % SY, x0 + np.arange(512))] = soup
    with skipping(gpu) as life:
        life.clear()
        life.set_rect(x0, y0, soup)
        np.testing.assert_array_equal(life.gather(), g0)
        life.step(12)
        want = oracle.life_run(g0, 12, threads=8)
        check(life, want, "skip")
        assert life.activity()[0] == 1
        life.step(49)
        check(life, oracle.life_run(want, 49, threads=8), "skip")


@BIT16
def test_skip_dense_soup_runs_every_tile(gpu, oracle, tile_rows):
    g = oracle.fill_random(NX, SY, 3, 0.5)
    with skipping(gpu) as life:
        life.configure(gpu.OPT_BLOCK_GENS, 5)
        life.fill_random(3, 0.5)
        for gens in (61, 7, 1):
            life.step(gens)
            g = oracle.life_run(g, gens, threads=8)
            passes, run, cleared, total = life.activity()
            check(life, g, "skip")
            assert passes == -(-gens // 5) and run == total and cleared == 0
            assert total == sum(3 * tile_rows_of(SY, m) for m in bs.pass_sizes(gens, 5))


@BIT16
def test_skip_domino_dies_and_does_not_come_back(gpu, tile_rows):
    """Two cells die at generation 1; the second pass of step(24) writes into the buffer that still holds
    them and runs no tile: without the clear class they would be back."""
    with skipping(gpu) as life:
        life.clear()
        life.set_cells([(5000, 300), (5001, 300)])
        life.step(24)
        passes, run, cleared, total = life.activity()
        check(life, np.zeros((SY, NX), np.uint8), "skip")
        assert passes == 2 and total == 2 * 3 * 7 and cleared >= 1 and run <= 4


@BIT16
def test_skip_highlife(gpu, tile_rows):
    """B36/S23 runs the table-rule instance: a soup window over the tile corner and a replicator."""
    g = np.zeros((SY, NX), np.uint8)
    g[100:260, 3900:4100] = rule_ref.soup(200, 160, 4, 0.4)
    rep = np.array([[0, 0, 1, 1, 1], [0, 1, 0, 0, 1], [1, 0, 0, 0, 1], [1, 0, 0, 1, 0], [1, 1, 1, 0, 0]], np.uint8)
    g[600:605, 8000:8005] = rep
    with skipping(gpu, rule="B36/S23") as life:
        life.upload(g)
        life.step(37)
        want = rule_ref.rule_run(g, 37, HIGHLIFE)
        check(life, want, "skip")
        assert want[550:, 7900:].any()
        passes, run, cleared, total = life.activity()
        assert passes == 4 and 0 < run < total


@BIT16
@pytest.mark.parametrize("bmax", [17, 32])
def test_skip_ghost_deeper_than_a_wave(gpu, oracle, tile_rows, bmax):
    """A glider 20 cells north-west of the tile corner (3968, 128 - 2 bmax), 3 bmax + 1 generations: as a call
    of three passes of bmax (whole waves of ghost rows; T = 94: 8 tile rows, T = 64: 11) and a call of one
    generation, and, on a fresh device, as one call, which runs four passes of about 3 bmax / 4 (13: T 102;
    25 and 24: T 78 and 80, still more ghost rows than a wave has)."""
    T = 128 - 2 * bmax
    cells = GLIDER + (3968 - 20, T - 20)
    for calls in ((3 * bmax, 1), (3 * bmax + 1,)):
        g = grid_of(cells, NX, SY)
        with skipping(gpu) as life:
            life.configure(gpu.OPT_BLOCK_GENS, bmax)
            life.clear()
            life.set_cells(cells)
            for gens in calls:
                life.step(gens)
                g = oracle.life_run(g, gens, threads=8)
                assert g.sum() == 5
                passes, run, cleared, total = life.activity()
                print(f"bmax {bmax} step({gens}): passes {passes} run {run} cleared {cleared} total {total}")
                check(life, g, "skip")
                sizes = bs.pass_sizes(gens, bmax)
                assert sizes == [bmax] * 3 or len(sizes) == (1 if gens == 1 else 4)
                assert passes == len(sizes) and total == sum(3 * tile_rows_of(SY, m) for m in sizes)
                assert 0 < run <= 4 * passes


# A glider at the periodic corner and a blinker in the middle; after 24 generations a second blinker at the
# listed place, whose three rows the map then holds as dead -- except on 3968 x 5, whose one map cell has no
# dead row (the edit still has to invalidate the map).  The oracle was run on each shape beforehand: at
# every generation to 49 the patterns are apart and whole (5 + 3, then 5 + 3 + 3 cells), as asserted below.
EDGE_SHAPES = [(4032, 200, (1000, 150)),  # 63 pairs: the last map column holds one pair, its first and its last
               # (... and is both neighbours of column 0, so either of its two edge masks serves there.  125 pairs:
               # three map columns, the last of one pair; the glider leaves it for column 0 through its LAST-pair
               # mask alone: test_skip_glider_alone_on_the_edge_shapes.)
               (8000, 200, (1000, 150)),
               (64, 40, (16, 35)),        # one pair in all: the column is its own left and right neighbour
               (128, 33, (32, 26)),       # a second map row of one row
               (3968, 5, (1000, 2))]      # lower than one map row, and than m


@BIT24_16
@pytest.mark.parametrize("nx,ny,second", EDGE_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in EDGE_SHAPES])
def test_skip_map_edge_shapes(gpu, oracle, tile_rows, nx, ny, second):
    first = np.concatenate([GLIDER + (nx - 8, ny - 4), BLINKER + (nx // 2, ny // 2)])
    more = BLINKER + second
    g = grid_of(first, nx, ny)
    with skipping(gpu, nx, ny) as life:
        life.clear()
        life.set_cells(first)
        life.step(24)
        g = oracle.life_run(g, 24)
        assert g.sum() == 8
        check(life, g, "skip")
        assert life.activity()[0] == 2
        rows = sorted({(y + d) % ny for y in more[:, 1] for d in (-1, 0, 1)})
        assert g[rows].any() == (ny == 5)
        life.set_cells(more)
        g[more[:, 1], more[:, 0]] = 1
        life.step(25)
        g = oracle.life_run(g, 25)
        assert g.sum() == 11
        check(life, g, "skip")
        passes, run, cleared, total = life.activity()
        assert passes == 3 and 0 < run <= total


@BIT24_16
@pytest.mark.parametrize("nx,ny", [s[:2] for s in EDGE_SHAPES], ids=[f"{s[0]}x{s[1]}" for s in EDGE_SHAPES])
def test_skip_glider_alone_on_the_edge_shapes(gpu, oracle, tile_rows, nx, ny):
    """The glider of the state above without the blinker, which on 4032 and 8000 x 200 lies in a pair that
    keeps the tiles of map column 0 running whatever the last column's masks say.  Alone, the glider reaches
    x = 0 at generation 24 only if the last-pair mask of the narrow last column made column 0's tile run in
    the second pass (a build without that mask fails this on 8000 x 200, and passes the state above)."""
    cells = GLIDER + (nx - 8, ny - 4)
    g = grid_of(cells, nx, ny)
    with skipping(gpu, nx, ny) as life:
        life.clear()
        life.set_cells(cells)
        for gens in (24, 25):
            life.step(gens)
            g = oracle.life_run(g, gens)
            assert g.sum() == 5
            check(life, g, "skip")
            passes, run, cleared, total = life.activity()
            assert passes == len(bs.pass_sizes(gens, 12)) and 0 < run <= total
        assert g[:, :8].sum() == 5  # it has crossed the seam


# ------------------------------------------------------------ partitioned shards: ring, interior, deep halo
SHARDED = [(4, (2, 2), 260, 260), (8, (1, 8), 64, 320), (2, (1, 2), 2048, 1100), (8, (4, 2), 8192, 200)]
GENS = (1, 4, 10, 45)  # cumulative


def sharded_reference(oracle, nx, ny, rule, gens):
    if rule == rule_ref.CONWAY:  # (test_rule_host.py pins rule_run to the oracle at B3/S23)
        have = _rule_refs.setdefault((nx, ny, 9, rule), {0: rule_ref.soup(nx, ny, 9)})
        if gens not in have:
            base = max(g for g in have if g <= gens)
            have[gens] = oracle.life_run(have[base], gens - base, threads=8)
            have[gens].setflags(write=False)
        return have[gens]
    return rule_reference(nx, ny, 9, rule, gens)


def run_sharded(gpu, oracle, life, nx, ny, rule, gens=GENS, option=None):
    with life:
        assert life.layout().generations_per_exchange == gpu.TEMPORAL_DEPTH["bit" if life.kernel else "byte"]
        life.upload(sharded_reference(oracle, nx, ny, rule, 0))
        if option:
            life.configure(*option)
        done = 0
        for n in gens:
            life.step(n - done)
            done = n
            want = sharded_reference(oracle, nx, ny, rule, n)
            np.testing.assert_array_equal(life.gather(), want, err_msg=f"generation {n}")
            assert life.last_path() == "tiles"
        assert life.live_count() == int(want.sum())


@BIT16
@pytest.mark.parametrize("rule", [rule_ref.CONWAY, HIGHLIFE], ids=["B3S23", "B36S23"])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("shards,dims,nx,ny", SHARDED)
def test_shards_local(gpu, oracle, tile_rows, shards, dims, nx, ny, overlap, rule):
    """K-deep aprons through the LOCAL transport: ring tiles first, the interior beside the exchange
    (overlap) or all tiles in one launch (serial), and the deep-halo passes between exchanges (1 + 3 + 6 +
    35 generations: up to three passes on one exchange)."""
    run_sharded(gpu, oracle, gpu.Life(nx, ny, shards=shards, kernel="bit", dims=dims, transport=gpu.XPORT_LOCAL,
                                      overlap=overlap, small_grid=False, rule=rule), nx, ny, rule)


@BIT16
def test_shards_without_deep_halo(gpu, oracle, tile_rows):
    life = gpu.Life(2048, 1100, shards=2, kernel="bit", dims=(1, 2), transport=gpu.XPORT_LOCAL, small_grid=False)
    run_sharded(gpu, oracle, life, 2048, 1100, rule_ref.CONWAY, option=(gpu.OPT_DEEP_HALO, 0))


@BIT16
def test_loopback(gpu, oracle, tile_rows):
    """The shard as a periodic partition of itself: both axes' aprons from halo messages to itself."""
    life = gpu.Life(2048, 300, kernel="bit", small_grid=False)
    run_sharded(gpu, oracle, life, 2048, 300, rule_ref.CONWAY, option=(gpu.OPT_LOOPBACK, 1))


# ------------------------------------------------------------ a device that outlives a shape change
@shape(("bit", 24))
@pytest.mark.parametrize("skip_dead", [False, True], ids=["flow", "skip"])
def test_device_outlives_a_shape_change(gpu, oracle, tile_rows, skip_dead):
    """50 generations at 24 rows, then 50 at 16 on the same device: the dataflow scratch (a pass counter per
    tile) and the skip-dead classes (a byte per tile) are sized per call from the shape of that call; 6 tile
    rows become 10 (flow, 2048 x 1000) and 5 become 7 (skip, 8192 x 700)."""
    nx, ny = (NX, SY) if skip_dead else (2048, 1000)
    if skip_dead:
        g = np.zeros((ny, nx), np.uint8)
        g[20:320, 3800:4312] = oracle.fill_random(512, 300, 13, 0.4)
        g[GLIDER[:, 1] + 690, GLIDER[:, 0] + 8180] = 1
    else:
        g = oracle.fill_random(nx, ny, seed=29, density=0.45)
    path = "skip" if skip_dead else "flow"
    with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=1, skip_dead=skip_dead) as life:
        life.upload(g)
        tiles = []
        for rows in (24, 16):
            gpu.tune_temporal(rows, "bit")
            life.step(50)
            g = oracle.life_run(g, 50, threads=8)
            check(life, g, path)
            tiles.append(life.activity()[3])
        if skip_dead:  # passes of 10: T 172, then 108
            assert tiles == [5 * 3 * 5, 5 * 3 * 7]


# ------------------------------------------------------------ byte tiles of 32 rows
def byte_ops(tiles, m, rows=32):
    return tiles * 64 * 8 * rows * (12 * m + 35)  # (test_gpu_parity.test_timing_stats)


@BYTE32
def test_byte_pipelined_regions(gpu, oracle, tile_rows):
    """2048 x 1600, OPT_PIPELINE 4, 40 generations = 2 passes of 20: 256-row windows under 32 ghost rows, 9
    tile rows of 192 (48-row waves: 5 of 320), two tile columns of 62 and 2 words."""
    nx, ny, gens = 2048, 1600, 40
    with gpu.Life(nx, ny, kernel="byte", small_grid=False, flow=0) as life:
        life.configure(gpu.OPT_PIPELINE, 4)
        life.upload(bs.reference(oracle, nx, ny, 5, 0))
        life.set_timing(True)
        life.step(gens)
        check(life, bs.reference(oracle, nx, ny, 5, gens), "tiles")
        if bs.MODE != "3":
            assert -(-ny // 192) == 9
            assert bs.booked(life) == pytest.approx(2 * byte_ops(2 * 9, 20))


@BYTE32
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("shards,dims,nx,ny", [(8, (4, 2), 512, 80), (2, (1, 2), 2048, 1100)])
def test_byte_shards_local(gpu, oracle, tile_rows, shards, dims, nx, ny, overlap):
    run_sharded(gpu, oracle, gpu.Life(nx, ny, shards=shards, kernel="byte", dims=dims, transport=gpu.XPORT_LOCAL,
                                      overlap=overlap, small_grid=False), nx, ny, rule_ref.CONWAY, (1, 8, 13, 40))


@BYTE32
def test_byte_own_apron_wrap(gpu, oracle, tile_rows):
    """4016 wide: not a multiple of 32, so x wraps through the shard's own apron (ring, exchange, interior)."""
    run_sharded(gpu, oracle, gpu.Life(4016, 130, kernel="byte", small_grid=False, flow=0), 4016, 130,
                rule_ref.CONWAY, (1, 8, 13, 40))


# ------------------------------------------------------------ afterwards
def test_default_shapes_are_back(gpu, oracle):
    """After everything above the process runs 24-row bit tiles and 48-row byte tiles again: the booked work
    of a pass over 2048 x 1000 is that of 6 tile rows of T 168 (16 rows: 10 of 104) and of 4 of T 320."""
    for kernel, ops in (("bit", lane_ops(bs.items_of(2048, 6), 12, 24)), ("byte", byte_ops(2 * 4, 12, 48))):
        with gpu.Life(2048, 1000, kernel=kernel, small_grid=False, flow=0) as life:
            life.upload(bs.reference(oracle, 2048, 1000, 5, 0))
            life.set_timing(True)
            life.step(12)
            check(life, bs.reference(oracle, 2048, 1000, 5, 12), "tiles")
            if bs.MODE != "3":
                assert bs.booked(life) == pytest.approx(ops)
