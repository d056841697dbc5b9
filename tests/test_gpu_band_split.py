"""The last tile column of the bit tiles as two banded sub-columns
(life::band_split, life_kernels.hip tile_geom / band_item): every path that
lists or runs banded items, compared cell by cell with the CPU oracle, on the
smallest shapes on which it can go wrong.  Per-launch tiles throughout
(small_grid=False, flow=0).

A row of W pairs is cut into tile columns of 62; the last one owns o = W - 62
(ntx - 1) pairs and runs as sub-columns of G lanes holding at most G - 2 of
them, 64 / G tile rows per workgroup: o = 32 as {30 in 32, 2 in 4}, 16 as
{14 in 16, 2 in 4}, 8 as {6 in 8, 2 in 4}, 31-44 in two parts, 30 and below
in one where no pair of parts takes fewer lanes, 45 and above as a whole
tile.  The booked VALU work (items x 64 lanes x 8 waves x 24 rows x 22 m)
shows which geometry ran.

The suite's A/B runs (LIFE_BANDS=0, LIFE_BAND_SPLIT=0, LIFE_TIMING_MODE) are
followed by the expected item counts; LIFE_TIMING_MODE=3 books nothing.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NY = 2851  # 17 tile rows at m = 12 (the last 163 rows short) and at m = 11: a G = 4 item once full, once partial
_CACHE = {}


def _flag(name):
    text = os.environ.get(name)
    if text is None:
        return True
    try:
        return int(text) != 0
    except ValueError:
        return False  # as atoi: text it cannot read is 0


MODE = os.environ.get("LIFE_TIMING_MODE", "0")


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


def group_of(own):
    return next((1 << g for g in range(2, 6) if own <= (1 << g) - 2), None)


def band_groups(o, split=None):
    """Group sizes G of the sub-columns the last tile column runs as ([]: a whole tile): brute force over
    every cut into two, fewest lanes, ties to one sub-column."""
    if not _flag("LIFE_BANDS"):
        return []
    if split is None:
        split = _flag("LIFE_BAND_SPLIT")
    best = [group_of(o)] if group_of(o) else []
    lanes = best[0] if best else 64
    for a in range(o - 1, 0, -1):
        if split and group_of(a) and group_of(o - a) and group_of(a) + group_of(o - a) < lanes:
            best, lanes = [group_of(a), group_of(o - a)], group_of(a) + group_of(o - a)
    return best


def items_of(nx, rows, split=None):
    """workgroups of a launch over `rows` tile rows of an nx-cell-wide shard"""
    W = -(-nx // 64)
    ntx = -(-W // 62)
    G = band_groups(W - 62 * (ntx - 1), split)
    return (ntx - (1 if G else 0)) * rows + sum(-(-rows // (64 // g)) for g in G)


def pass_sizes(gens, bmax=12):
    sizes = []
    while gens:
        n = -(-gens // bmax)
        sizes.append(-(-gens // n))
        gens -= sizes[-1]
    return sizes


def lane_ops(items, m):
    return items * 64 * 8 * 24 * 22 * m


def booked(life):
    _, n, _ = life.kernel_stats()
    return n * life.kernel_work()[1]


def run_whole(gpu, oracle, nx, ny, gens, bmax=None):
    with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=0) as life:
        if bmax:
            life.configure(gpu.OPT_BLOCK_GENS, bmax)
        life.upload(reference(oracle, nx, ny, 5, 0))
        life.set_timing(True)
        life.step(gens)
        assert life.last_path() == "tiles"
        np.testing.assert_array_equal(life.gather(), reference(oracle, nx, ny, 5, gens))
        # (a width of whole pairs wraps x inside the tiles and runs one timed launch per pass; any other wraps
        # through its own apron, as ring and interior launches with the exchange between: not booked per pass)
        if MODE != "3" and nx % 64 == 0:
            want = sum(lane_ops(items_of(nx, -(-ny // (192 - 2 * m))), m) for m in pass_sizes(gens, bmax or 12))
            assert booked(life) == pytest.approx(want)


# two tile columns, the last owning o pairs: split (31, 32, 36, 44, 16, 8) and not (30: one band, 45: a whole
# tile); one tile column of 32 / 31 pairs, whose sub-column 0 also holds the wrap at pair -1; a partial last pair
WIDTHS = [64 * (62 + o) for o in (31, 32, 36, 44, 16, 8, 30, 45)] + [64 * 32, 64 * 31, 64 * 94 - 27]


@pytest.mark.parametrize("nx", WIDTHS)
def test_whole_launches_match_oracle(gpu, oracle, nx):
    """23 generations: passes of 12 and 11, so the tile grid changes inside the call."""
    assert pass_sizes(23) == [12, 11]
    run_whole(gpu, oracle, nx, NY, 23)


def test_split_shapes_are_split():
    """the cases above do run two sub-columns where they should (lanes per tile row of the last column)"""
    want = {31: 36, 32: 36, 36: 40, 44: 48, 16: 20, 8: 12, 30: 32, 45: 64}
    for o, lanes in want.items():
        assert sum(band_groups(o, True) or [64]) == lanes
    assert band_groups(32, True) == [32, 4] and band_groups(32, False) == []


def test_passes_of_32_generations(gpu, oracle):
    """OPT_BLOCK_GENS 32: 64 ghost rows per window, 128 owned; the sub-columns' ghost lanes absorb 32 cells"""
    run_whole(gpu, oracle, 64 * 94, NY, 32, bmax=32)


def test_on_poisoned_buffers(gpu, oracle, monkeypatch):
    """a pair no sub-column stored comes back as 0xA5 cells"""
    monkeypatch.setenv("LIFE_POISON", "1")
    run_whole(gpu, oracle, 64 * 94, NY, 23)
    run_whole(gpu, oracle, 64 * 78, NY, 23)


@pytest.mark.parametrize("ny,rows,regions", [(1400, 9, (3, 2, 2, 2)), (11088, 66, (16, 16, 16, 18))])
def test_pipelined_regions(gpu, oracle, ny, rows, regions):
    """OPT_PIPELINE 4, 48 generations = 4 passes of 12.  9 tile rows: regions of 3, 2, 2, 2, not aligned on
    the bands (each region's banded items start at its first tile row); 66: regions aligned on the largest
    band, 16 tile rows, so a pass takes the items of a whole launch."""
    nx, gens = 6016, 48
    assert -(-ny // 168) == rows and sum(regions) == rows
    with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=0) as life:
        life.configure(gpu.OPT_PIPELINE, 4)
        life.upload(reference(oracle, nx, ny, 5, 0))
        life.set_timing(True)
        life.step(gens)
        assert life.last_path() == "tiles"
        np.testing.assert_array_equal(life.gather(), reference(oracle, nx, ny, 5, gens))
        if MODE == "0":  # (modes 1 / 2 run whole launches)
            assert booked(life) == pytest.approx(4 * lane_ops(sum(items_of(nx, r) for r in regions), 12))
    if rows == 66:
        assert sum(items_of(nx, r, True) for r in regions) == items_of(nx, rows, True) == 66 + 33 + 5


def test_half_height_tail_band_vs_oracle(gpu, oracle):
    """6016 x 84000: 500 tile rows, 782 items on 768 slots, so the bottom tile rows run as half-height tiles,
    both sub-columns banded there too.  Pinned to the oracle on a full-height band around the x = 0 seam that
    holds the whole last tile column (pairs 62..93: both sub-columns, their seam and the tile column left of
    them) and the wrap; the band's cut edges are wrong by at most 24 cells."""
    nx, ny, gens, left, right, margin = 6016, 84000, 24, 2048 + 64, 64, 32
    band = oracle.fill_random_window(nx, nx - left - margin, 0, left + right + 2 * margin, ny, seed=7, density=0.5)
    cols = np.r_[nx - left:nx, 0:right]
    with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=0) as life:
        life.configure(gpu.OPT_BLOCK_GENS, 12)
        life.fill_random(7, 0.5)
        life.set_timing(True)
        life.step(gens)
        assert life.last_path() == "tiles"
        got = life.gather()[:, cols]
        work = booked(life)
    band = oracle.life_run(band, gens, threads=8)
    np.testing.assert_array_equal(got, band[:, margin:margin + left + right])
    if MODE != "3" and os.environ.get("LIFE_TAIL_SPLIT", "2") != "0" and _flag("LIFE_BANDS") and \
            _flag("LIFE_BAND_SPLIT"):
        # half-height items were booked, at half a tile each: not the 782 whole items per pass but F full
        # tile rows and the ceil((84000 - 168 F) / 72) half rows below them, every row with both sub-columns
        assert items_of(nx, 500) == 782
        per_pass = work / (2 * lane_ops(1, 12))
        assert per_pass != pytest.approx(782)
        splits = [items_of(nx, F) + 0.5 * items_of(nx, -(-(ny - 168 * F) // 72)) for F in range(500)]
        assert any(per_pass == pytest.approx(s) for s in splits), per_pass


@pytest.mark.parametrize("ny,shards,dims", [(300, 2, (2, 1)), (600, 4, (2, 2))])
def test_partitioned_deep_halo(gpu, oracle, ny, shards, dims):
    """Blocks 94 pairs wide, LOCAL transport, deep halo on (the default): ring and interior regions list the
    sub-columns' items, and the passes between exchanges store the apron pairs -1 (left ghost lane of the
    first tile column) and W (right ghost lane of the LAST sub-column)."""
    nx, done = 12032, 0
    for r in range(shards):
        assert gpu.layout_query(nx, ny, dims, r, "bit").w == 6016
    with gpu.Life(nx, ny, shards=shards, kernel="bit", dims=dims, transport=gpu.XPORT_LOCAL, small_grid=False,
                  flow=0) as life:
        life.configure(gpu.OPT_DEEP_HALO, 1)
        life.upload(reference(oracle, nx, ny, 5, 0))
        for gens in (5, 20, 7):
            life.step(gens)
            done += gens
            np.testing.assert_array_equal(life.gather(), reference(oracle, nx, ny, 5, done),
                                          err_msg=f"after {done} generations")


_ONE_BAND = r"""
import json, sys
sys.path.insert(0, {pkg!r})
import life_mi355x as lm
with lm.Life({nx}, {ny}, kernel="bit", small_grid=False, flow=0) as life:
    life.fill_random(9, 0.5)
    life.set_timing(True)
    life.step({gens})
    _, n, _ = life.kernel_stats()
    print("ONE_BAND " + json.dumps([life.checksum(), life.live_count(), n * life.kernel_work()[1]]), flush=True)
"""


def test_one_band_knob_gives_the_same_grid_and_books_more(gpu, oracle):
    """LIFE_BAND_SPLIT=0 (read once per process: a child) runs the last column of 32 pairs as whole tiles:
    the same grid, and a booked VALU count higher by exactly the item difference x 64 lanes x 8 x 24 x 22 m."""
    from conftest import ROOT

    nx, ny, gens = 6016, NY, 24
    want = reference(oracle, nx, ny, 9, gens)
    with gpu.Life(nx, ny, kernel="bit", small_grid=False, flow=0) as life:
        life.fill_random(9, 0.5)
        life.set_timing(True)
        life.step(gens)
        np.testing.assert_array_equal(life.gather(), want)
        here = (life.checksum(), life.live_count(), booked(life))
    script = _ONE_BAND.format(pkg=os.path.join(ROOT, "mpi-and-open-mp_amd"), nx=nx, ny=ny, gens=gens)
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, LIFE_BAND_SPLIT="0"),
                         capture_output=True, text=True, timeout=110)
    assert out.returncode == 0 and "ONE_BAND" in out.stdout, out.stdout + out.stderr
    there = json.loads(out.stdout.split("ONE_BAND ", 1)[1])
    assert tuple(there[:2]) == here[:2] == (oracle.checksum(want), int(want.sum()))
    if MODE != "3":
        more = items_of(nx, 17, False) - items_of(nx, 17)
        if _flag("LIFE_BANDS") and _flag("LIFE_BAND_SPLIT"):
            assert (items_of(nx, 17, False), items_of(nx, 17)) == (34, 28)
        assert there[2] - here[2] == pytest.approx(2 * lane_ops(more, 12), abs=1.0)
