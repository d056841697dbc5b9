"""The population trace (LIFE_OPT_POPULATION, life_dev_population): the live
cells of the whole grid after every generation of a step call, counted inside
the bit tiles (census instances, life_kernels.hip tile_body_bit POP) or, on
every other device, by the census kernel behind one-generation launches.

Expected counts come from the oracle stepped ONE generation at a time
(oracle.life_run(grid, 1); tests/rule_ref.py under a rule); every case also
compares the final gather() with it and checks last_path().

The base shape is the one tests/test_gpu_skip_dead.py argues for: 8192 x 700
bit, small-grid kernels off -- three tile columns of 62, 62 and 4 pairs (the
last banded), a partial last tile row, both wraps; 61 generations run as
passes of 11, 10, 10, 10, 10, 10, so the tile grid changes inside the call.
A wrong ownership mask shows in the generation where it happens: a counted
ghost row or edge lane, a seam counted twice, the rows below `ylim` or the
apron cells a deep-halo pass advances.
"""
import os
import subprocess

import numpy as np
import pytest

import rule_ref
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NX, NY = 8192, 700
GENS = 61
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")
DRIVER = os.path.join(ROOT, "mpi-and-open-mp_amd", "driver", "life_mi355x")
GLIDER = np.array([(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)], np.int64)
BLINKER = np.array([(0, 0), (1, 0), (2, 0)], np.int64)
HIGHLIFE = rule_ref.NAMED["B36/S23"]
LIFE_EINVAL = -1
_CACHE = {}


def curve(oracle, grid, gens, rule=None):
    """(counts[gens], final grid): the population after each generation, stepping one at a time."""
    counts = np.empty(gens, np.int64)
    for g in range(gens):
        grid = oracle.life_run(grid, 1, threads=8) if rule is None else rule_ref.rule_step(grid, *rule)
        counts[g] = int(grid.sum())
    return counts, grid


def soup_ref(oracle, rule=None):
    """The base soup, its 61-generation curve and final grid: computed once per rule, read-only."""
    if rule not in _CACHE:
        g0 = oracle.fill_random(NX, NY, 7, 0.5)
        counts, end = curve(oracle, g0, GENS, rule)
        for a in (g0, counts, end):
            a.setflags(write=False)
        _CACHE[rule] = (g0, counts, end)
    return _CACHE[rule]


def soup_long(oracle):
    """The B3/S23 soup's curve over 84 generations (a call of 20, then one of 64) and its grid there."""
    if "long" not in _CACHE:
        _, counts, end = soup_ref(oracle)
        more, end = curve(oracle, end, 84 - GENS)
        counts = np.concatenate([counts, more])
        for a in (counts, end):
            a.setflags(write=False)
        _CACHE["long"] = (counts, end)
    return _CACHE["long"]


def recording(gpu, nx=NX, ny=NY, **kw):
    kw.setdefault("kernel", "bit")
    kw.setdefault("small_grid", False)
    return gpu.Life(nx, ny, population=True, **kw)


def check(life, counts, grid, path="tiles"):
    got = life.population()
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, counts)
    assert life.last_path() == path
    np.testing.assert_array_equal(life.gather(), grid)
    assert life.live_count() == int(counts[-1])


@pytest.fixture
def tile_rows(gpu, request):
    """The bit tiles at `rows` register rows per wave for one test (as tests/test_gpu_tile_shapes.py)."""
    gpu.tune_temporal(request.param, "bit")
    try:
        yield request.param
    finally:
        gpu.tune_temporal(gpu.TEMPORAL_ROWS["bit"], "bit")


HEIGHTS = pytest.mark.parametrize("tile_rows", [24, 16], indirect=True, ids=["bit24", "bit16"])


# ------------------------------------------------------------ 1. soup, both tile heights, poisoned buffers
@HEIGHTS
@pytest.mark.parametrize("poison", [False, True], ids=["zeroed", "poisoned"])
def test_soup(gpu, oracle, tile_rows, poison, monkeypatch):
    """Seams counted twice, the partial last tile row (ylim) and the narrow banded column (j2 < W) all show
    here; on buffers full of 0xA5 (LIFE_POISON, read at creation) a counted cell that was never written does."""
    if poison:
        monkeypatch.setenv("LIFE_POISON", "1")
    g0, counts, end = soup_ref(oracle)
    with recording(gpu) as life:
        life.upload(g0)
        life.step(GENS)
        check(life, counts, end)


# ------------------------------------------------------------ 2. ghost-zone discipline
# 33 generations run as passes of 11: tile rows of 170 rows, tile columns of 62 pairs = 3968 cells
CELLS = {"tile-corner": (3968, 170), "before-tile-corner": (3967, 169), "periodic-corner": (NX - 1, NY - 1),
         "origin": (0, 0), "last-partial-tile-row": (5000, 690), "banded-column": (8000, 340)}


@pytest.mark.parametrize("where", list(CELLS))
def test_single_cell_under_the_parity_rule(gpu, where):
    """B1357/S1357 (tests/test_gpu_light_cone.py): one cell spreads at light speed and the population changes
    every generation, so a counted ghost row or edge lane gives a wrong number in the generation where it
    happens.  The pattern stays inside a 67 x 67 window for 33 generations: the curve comes from that window
    stepped alone, the final grid is the window rolled into place."""
    x, y = CELLS[where]
    gens, half = 33, 40
    win = np.zeros((2 * half + 1, 2 * half + 1), np.uint8)
    win[half, half] = 1
    counts = np.empty(gens, np.int64)
    for g in range(gens):
        win = rule_ref.rule_step(win, *rule_ref.PARITY)
        counts[g] = int(win.sum())
    assert len(set(np.diff(counts))) > 1 and not win[0].any() and not win[:, 0].any()
    want = np.zeros((NY, NX), np.uint8)
    want[:2 * half + 1, :2 * half + 1] = win
    want = np.roll(want, (y - half, x - half), (0, 1))
    with recording(gpu, rule="B1357/S1357") as life:
        life.clear()
        life.set_cells([(x, y)])
        life.step(gens)
        check(life, counts, want)


# ------------------------------------------------------------ 3. the table-rule instance
def test_highlife_soup(gpu, oracle):
    g0, counts, end = soup_ref(oracle, HIGHLIFE)
    assert not np.array_equal(counts, soup_ref(oracle)[1])
    with recording(gpu, rule="B36/S23") as life:
        life.upload(g0)
        life.step(GENS)
        check(life, counts, end)


# ------------------------------------------------------------ 4. partitioned shards
SHARDED = pytest.mark.parametrize("dims", [(2, 2), (1, 4), (4, 1)], ids=["2x2", "rows", "cols"])


@SHARDED
@pytest.mark.parametrize("option", [None, "OPT_DEEP_HALO", "OPT_OVERLAP"], ids=["default", "no-deep-halo", "serial"])
def test_shards(gpu, oracle, dims, option):
    """LOCAL transport.  20 generations run as 10 + 10, the first a deep-halo pass that also advances apron
    rows and pairs (some other shard's cells: not counted), then one exchange; 64 more as ring + interior
    launches on two streams adding into the same counters.  The trace is the sum over the shards."""
    g0 = soup_ref(oracle)[0]
    counts, end = soup_long(oracle)
    with recording(gpu, shards=4, dims=dims, transport=gpu.XPORT_LOCAL) as life:
        if option:
            life.configure(getattr(gpu, option), 0)
        life.upload(g0)
        life.step(20)
        np.testing.assert_array_equal(life.population(), counts[:20])
        assert life.last_path() == "tiles"
        life.step(64)
        check(life, counts[20:], end)


def test_loopback(gpu, oracle):
    """One shard that exchanges both halos with itself (LIFE_OPT_LOOPBACK 1): ring, interior and deep-halo
    passes on a single device."""
    g0 = soup_ref(oracle)[0]
    counts, end = soup_long(oracle)
    with recording(gpu) as life:
        life.configure(gpu.OPT_LOOPBACK, 1)
        life.upload(g0)
        life.step(20)
        np.testing.assert_array_equal(life.population(), counts[:20])
        life.step(64)
        check(life, counts[20:], end)


# ------------------------------------------------------------ 5. half-height tail and both sub-columns
TAIL = (1984, 256433, 2)  # nx (31 pairs: sub-columns of 30 and 1), ny, generations per pass

_PLAN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "life_host.h"
int main(int, char **argv) {  // W h m slots -> sub-columns, full tile rows F, half rows n2, tile rows
    const long long W = atoll(argv[1]), h = atoll(argv[2]), m = atoll(argv[3]), slots = atoll(argv[4]);
    const long long ntx = (W + 61) / 62, T = 192 - 2 * m, T2 = 96 - 2 * m, nty = (h + T - 1) / T;
    const life::BandSplit sp = life::band_split(W - 62 * (ntx - 1));
    life::BandRows b;
    for (b.n = 0; b.n < sp.n; b.n++) b.B[b.n] = 64 >> sp.b[b.n].gsh;
    const life::TailPlan p = life::tail_plan(ntx - (b.n > 0 ? 1 : 0), b, 0, nty, h, T, T2, slots, 2, 0.06, 0);
    printf("%d %lld %lld %lld\n", sp.n, (long long)p.F, (long long)p.n2, nty);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    (d / "p.cpp").write_text(_PLAN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    str(d / "p.cpp"), os.path.join(CSRC, "life_plan.cpp"), "-o", str(d / "p")], check=True)
    return lambda *a: tuple(map(int, subprocess.run([str(d / "p"), *map(str, a)], check=True, capture_output=True,
                                                    text=True).stdout.split()))


def test_half_height_tail(gpu, oracle, plan):
    """The smallest shape whose whole-block launch takes a tail split and a two-sub-column band: one tile
    column of 31 pairs (0.5625 items per tile row) needs 1365 tile rows to pass the 768 slots of 256 CUs x 3
    tiles; one row fewer and the plan has no tail.  Two passes of 2 generations (an intermediate generation
    in each pass; the oracle steps half a billion cells per generation)."""
    nx, ny, m = TAIL
    slots = 768
    bands, F, n2, nty = plan(nx // 64, ny, m, slots)
    assert bands == 2 and 0 < F < nty and n2 > 0, (bands, F, n2, nty)
    assert plan(nx // 64, ny - 1, m, slots)[1] == nty - 1  # 1364 tile rows: no tail
    g = oracle.fill_random(nx, ny, 7, 0.5)
    counts, g = curve(oracle, g, 2 * m)
    with recording(gpu, nx, ny, flow=0) as life:
        life.configure(gpu.OPT_BLOCK_GENS, m)
        life.fill_random(7, 0.5)
        life.set_timing(True)
        life.step(2 * m)
        _, launches, _ = life.kernel_stats()
        _, valu = life.kernel_work()
        check(life, counts, g)
    # half tiles were booked at half a tile each: fewer lane-ops than nty rows of whole items
    if os.environ.get("LIFE_TIMING_MODE", "0") != "3" and os.environ.get("LIFE_TAIL_SPLIT", "2") == "2":
        assert launches == 2
        items = lambda rows: -(-rows // 2) + -(-rows // 16)  # noqa: E731  (G = 32 and G = 4: 2 and 16 rows an item)
        per_item = 64 * 8 * 24 * (gpu.CONWAY_VALU_PER_PAIR_ROW + gpu.POP_VALU_PER_PAIR_ROW) * m
        assert valu == pytest.approx((items(F) + 0.5 * items(n2)) * per_item)


# ------------------------------------------------------------ 6. skip-dead passes
def test_skip_dead_glider_and_blinker(gpu, oracle):
    cells = np.concatenate([GLIDER + (3960, 160), BLINKER + (6000, 500)])
    g = np.zeros((NY, NX), np.uint8)
    g[cells[:, 1], cells[:, 0]] = 1
    with recording(gpu, skip_dead=True) as life:
        life.clear()
        life.set_cells(cells)
        life.step(GENS)
        passes, run, cleared, total = life.activity()
        check(life, np.full(GENS, 8, np.int64), oracle.life_run(g, GENS, threads=8), path="skip")
        assert passes == 6 and 0 < run < total


def test_skip_dead_gun(gpu, oracle):
    _, _, _, _, cells = gpu.load_cfg_cells(os.path.join(GOLDEN, "cfg", "p46gun.cfg"))
    cells = cells + (3900, 100)  # across the tile corner (3968, 168)
    g = np.zeros((NY, NX), np.uint8)
    g[cells[:, 1], cells[:, 0]] = 1
    counts, end = curve(oracle, g, GENS)
    assert len(set(counts)) > 10
    with recording(gpu, skip_dead=True) as life:
        life.clear()
        life.set_cells(cells)
        life.step(GENS)
        check(life, counts, end, path="skip")
        passes, run, cleared, total = life.activity()
        assert run < total


# ------------------------------------------------------------ 7. the generic path
def generic(gpu, oracle, nx, ny, path, configure=(), **kw):
    g0 = oracle.fill_random(nx, ny, 3, 0.4)
    counts, end = curve(oracle, g0, 20)
    with gpu.Life(nx, ny, population=True, **kw) as life:
        for opt, v in configure:
            life.configure(opt, v)
        life.upload(g0)
        life.step(20)
        assert life.last_path() != "flow"
        check(life, counts, end, path=path)


def test_generic_byte(gpu, oracle):
    g0, counts, _ = soup_ref(oracle)
    with recording(gpu, kernel="byte") as life:
        life.upload(g0)
        life.step(20)
        check(life, counts[:20], oracle.life_run(g0, 20, threads=8))


@pytest.mark.parametrize("nx,ny", [(1000, 37), (100, 37)])
def test_generic_widths_of_partial_pairs(gpu, oracle, nx, ny):
    """A last pair that also holds apron cells: one generation per launch and the census kernel."""
    with gpu.Life(nx, ny, kernel="bit", small_grid=False) as life:
        life.step(1)
        path = life.last_path()
    generic(gpu, oracle, nx, ny, path, kernel="bit", small_grid=False)


def test_small_grid_is_bypassed(gpu, oracle):
    with gpu.Life(200, 96, kernel="bit") as life:
        life.step(20)
        assert life.last_path() == "small"
    generic(gpu, oracle, 200, 96, "tiles", kernel="bit")


def test_dataflow_form_is_bypassed(gpu, oracle):
    """2048 x 1000 at 20 generations per pass, LIFE_OPT_FLOW 1 (tests/test_gpu_flow.py CASES[0]): 87
    generations run as dataflow passes without the option; with it, as census tiles."""
    nx, ny, m = 2048, 1000, 20
    with gpu.Life(nx, ny, kernel="bit", small_grid=False) as life:
        life.configure(gpu.OPT_FLOW, 1)
        life.configure(gpu.OPT_BLOCK_GENS, m)
        life.step(87)
        assert life.last_path() == "flow"
    generic(gpu, oracle, nx, ny, "tiles", configure=[(gpu.OPT_FLOW, 1), (gpu.OPT_BLOCK_GENS, m)], kernel="bit",
            small_grid=False)


# ------------------------------------------------------------ 8. the contract
def test_option_off_records_nothing(gpu, oracle):
    g0, counts, _ = soup_ref(oracle)
    with gpu.Life(NX, NY, kernel="bit", small_grid=False) as life:
        assert life.population().size == 0  # before any call
        life.upload(g0)
        life.step(12)
        assert life.population().size == 0 and life.population().dtype == np.int64
        assert life.last_path() == "tiles"
        life.configure(gpu.OPT_POPULATION, 1)
        life.step(10)
        np.testing.assert_array_equal(life.population(), counts[12:22])
        life.configure(gpu.OPT_POPULATION, 0)
        life.step(3)
        assert life.population().size == 0
        for v in (2, -1):
            with pytest.raises(gpu.LifeError) as e:
                life.configure(gpu.OPT_POPULATION, v)
            assert e.value.rc == LIFE_EINVAL
    with gpu.Life(2048, 1000, kernel="bit", small_grid=False) as life:  # the paths of a device with the option off
        life.configure(gpu.OPT_FLOW, 1)
        life.configure(gpu.OPT_BLOCK_GENS, 20)
        life.step(87)
        assert life.last_path() == "flow" and life.population().size == 0


def test_trace_is_the_last_calls(gpu, oracle):
    import ctypes

    g0, counts, _ = soup_ref(oracle)
    with recording(gpu) as life:
        life.upload(g0)
        life.step(7)
        life.step(13)
        np.testing.assert_array_equal(life.population(), counts[7:20])
        assert life.live_count() == counts[19]
        # the C reader: length query, a short max, a long max
        lib, n = gpu._lib(), ctypes.c_int64(-1)
        assert lib.life_dev_population(life._h, None, 0, ctypes.byref(n)) == 0 and n.value == 13
        buf = np.full(20, -7, np.int64)
        p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        assert lib.life_dev_population(life._h, p, 5, ctypes.byref(n)) == 0 and n.value == 13
        np.testing.assert_array_equal(buf[:5], counts[7:12])
        assert (buf[5:] == -7).all()
        assert lib.life_dev_population(life._h, p, 20, None) == 0
        np.testing.assert_array_equal(buf[:13], counts[7:20])
        assert (buf[13:] == -7).all()
        assert lib.life_dev_population(life._h, None, 3, ctypes.byref(n)) == LIFE_EINVAL
        life.step(0)
        assert life.population().size == 0
        life.step(1)
        np.testing.assert_array_equal(life.population(), counts[20:21])


def test_one_timed_launch_per_pass(gpu, oracle):
    """Timing on: the fold behind a pass is not a timed launch; the census ops are booked."""
    g0, counts, _ = soup_ref(oracle)
    with recording(gpu, flow=0) as life:
        life.upload(g0)
        life.set_timing(True)
        life.step(24)
        _, launches, _ = life.kernel_stats()
        updates, valu = life.kernel_work()
        np.testing.assert_array_equal(life.population(), counts[:24])
    if os.environ.get("LIFE_TIMING_MODE", "0") != "3":
        assert launches == 2 and updates == NX * NY * 12
        items = 2 * 5 + 1  # 5 tile rows of 168 rows: two whole tile columns and one banded item (4 pairs, G = 8)
        if os.environ.get("LIFE_BANDS", "1") != "0":
            assert valu == pytest.approx(items * 64 * 8 * 24 * 12 *
                                         (gpu.CONWAY_VALU_PER_PAIR_ROW + gpu.POP_VALU_PER_PAIR_ROW))


def test_edits_between_calls(gpu, oracle):
    g0, counts, _ = soup_ref(oracle)
    g = np.array(oracle.life_run(g0, 12, threads=8))
    block = np.ones((40, 64), np.uint8)
    with recording(gpu) as life:
        life.upload(g0)
        life.step(12)
        np.testing.assert_array_equal(life.population(), counts[:12])
        cells = [(x, y) for y in range(330, 370) for x in range(3936, 4000)]  # across the tile column seam
        life.set_cells(cells)
        g[330:370, 3936:4000] = block
        more, end = curve(oracle, g, 12)
        assert not np.array_equal(more, counts[12:24])
        life.step(12)
        check(life, more, end)


# ------------------------------------------------------------ 9. the driver
def test_driver_population_file(gpu, oracle, tmp_path):
    cfg = os.path.join(GOLDEN, "cfg", "p46gun.cfg")  # 300 x 100, here in 512 x 300: census tiles
    nx, ny, steps = 512, 300, 100
    _, _, _, _, cells = gpu.load_cfg_cells(cfg)
    grid = np.zeros((ny, nx), np.uint8)
    grid[cells[:, 1], cells[:, 0]] = 1

    def run(cwd, *extra):
        os.makedirs(cwd)
        r = subprocess.run([DRIVER, cfg, "--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--save-steps", "40",
                            *extra], cwd=cwd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        float(r.stdout)  # the printed time: one "%f\n"
        assert r.stdout.count("\n") == 1
        vtk = os.path.join(cwd, "vtk")
        return {f: open(os.path.join(vtk, f), "rb").read() for f in sorted(os.listdir(vtk))}

    plain = run(str(tmp_path / "plain"))
    out = tmp_path / "pop.txt"
    traced = run(str(tmp_path / "traced"), "--population", str(out))
    assert len(plain) == 3 and traced == plain
    counts, _ = curve(oracle, grid, steps)
    want = "".join(f"{g} {n}\n" for g, n in enumerate([int(grid.sum()), *counts]))
    assert out.read_text() == want
