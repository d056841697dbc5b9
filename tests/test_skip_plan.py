"""The activity-map arithmetic of the skip-dead passes (LIFE_OPT_SKIP_DEAD,
csrc/life_act.h), checked on the CPU: the header the plan kernel includes is
compiled into a g++ harness, as tests/test_pipe_plan.py reaches life::pipe_plan.

A map cell covers 62 pair columns (one tile column) x 32 rows and holds three
row masks: any pair, the first pair, the last pair.  For every tile of a pass
the harness prints what the plan kernel works from -- the map rows and row
bits of the tile's window (owned rows + m ghost rows at each end, wrapped),
the map columns of the edge lane columns at either side (wrapped), the map
rows and bits of its owned rows -- and, given a map, what act_window_live
says.  Brute force over cells says what those must be:

* the read set is exactly the set of map cells holding a cell of the wrapped
  window: nothing missing (a live cell there would be skipped over), nothing
  more (the pass would run tiles it need not); and, finer than the map cells,
  the row bits are exactly the window's rows;
* the left / right map columns hold the pair before / after the owned pairs,
  as their last / first pair;
* the owned set is exactly the owned rows, in map column tx;
* a model pass over random sparse states, the map built in numpy: every tile
  act_window_live does not run is all dead in the oracle's result after m
  generations, and every tile whose cell window is dead is not run;
* a model pass at light speed: those states move a row per two generations
  at most, so under the parity rule (rule_ref.PARITY, one cell reaches
  (+-m, +-m) in m generations) a single cell on a tile's diagonal makes the
  tile run at distance m, and reaches its corner cell, and not at m + 1.

Geometries: 8192 x 700 (three tile columns of 62, 62 and 4 pairs; five tile
rows at m = 12, the last partial) at m = 12, 10, 5, 1; 3968 x 1349 at m = 12,
whose last tile row has 5 rows, fewer than m, so tile row 0's window reaches
two tile rows up; 4096 x 200 and 3968 x 160, where a tile is its own
neighbour (the latter one tile in all).

The window height is a parameter: 192 rows (8 waves x 24 register rows, the
default shape; also at m = 16, 17 and 32) and 128 rows (16 register rows):
T = 128 - 2m is 104 at m = 12, 64 at m = 32; 3968 x 1253 has a 5-row last tile
row there; 4032 wide leaves one pair to the last map column, 64 wide is one
pair in all, 3968 x 5 is lower than one map row.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "life_act.h"
// a row span as its (map row, row bits) pairs
static void put(const life::ActSpan &s) {
    int n = 0;
    for (int i = 0; i < 3; i++) n += (int)(s.b[i] - s.a[i]);
    printf(" %d", n);
    for (int i = 0; i < 3; i++)
        for (long long r = s.a[i]; r < s.b[i]; r++) printf(" %lld %u", r, life::act_row_bits(s, i, r));
}
// argv: W h T m [map file]; per tile one line:
// tx ty | read rows | left col, right col | map cols of the window | owned rows | window live (-1: no map)
int main(int argc, char **argv) {
    const long long W = atoll(argv[1]), h = atoll(argv[2]), T = atoll(argv[3]);
    const int m = atoi(argv[4]);
    const long long ncol = life::act_cols(W), nrow = life::act_rows(h);
    std::vector<uint32_t> map;
    if (argc > 5) {
        map.resize((size_t)(ncol * nrow * life::kActWords));
        FILE *f = fopen(argv[5], "rb");
        if (!f || fread(map.data(), 4, map.size(), f) != map.size()) return 2;
        fclose(f);
    }
    printf("G %d %d %d %lld %lld\n", life::kActRows, life::kActPairs, life::kActWords, ncol, nrow);
    for (long long ty = 0; ty * T < h; ty++)
        for (long long tx = 0; tx < ncol; tx++) {
            printf("%lld %lld", tx, ty);
            const life::ActSpan rr = life::act_read_rows(ty, T, m, h), rc = life::act_read_cols(tx, W);
            put(rr);
            printf(" %lld %lld", (long long)life::act_left_col(tx, W), (long long)life::act_right_col(tx, W));
            int n = 0;
            for (int i = 0; i < 3; i++) n += (int)(rc.b[i] - rc.a[i]);
            printf(" %d", n);
            for (int i = 0; i < 3; i++)
                for (long long c = rc.a[i]; c < rc.b[i]; c++) printf(" %lld", c);
            put(life::act_own_rows(ty, T, h));
            printf(" %d\n", map.empty() ? -1 : (int)life::act_window_live(map.data(), W, rr, tx));
        }
    return 0;
}
"""

WINDOW = 8 * 24  # rows of a tile's window: 8 waves x 24 register rows (the default shape)
WINDOW16 = 8 * 16  # ... x 16 register rows (life_tune_temporal / LIFE_TEMPORAL_ROWS 16)
GEOMS = [(8192, 700, 12), (8192, 700, 10), (8192, 700, 5), (8192, 700, 1), (3968, 1349, 12), (4096, 200, 12),
         (4096, 200, 1), (3968, 160, 12)]


def shaped(window, cases):
    """(nx, ny, m, window) parameters, ids 'w<window>-nx-ny-m'."""
    return [pytest.param(*c, window, id="w%d-%d-%d-%d" % ((window,) + c)) for c in cases]


def default_shape(cases):
    return [pytest.param(*c, WINDOW, id="%d-%d-%d" % c) for c in cases]


# m above 16: at 16-row waves whole waves of the window are ghost; at m = 32 a 128-row window owns 64 rows, two
# map rows; T = 128 - 2m is 104, 106, 94: another alignment against the map's 32-row words; 3968 x 1253 at
# T = 104: a last tile row of 5 rows, fewer than m; one pair in the last map column (4032), one pair in all (64:
# a column its own left and right neighbour), a height under one map row (3968 x 5); 8000: three map columns,
# the last of one pair (4032 has two, and its last is both neighbours of its first)
GEOMS_DEEP = [(8192, 700, 16), (8192, 700, 17), (8192, 700, 32)]
GEOMS16 = [(8192, 700, 12), (8192, 700, 11), (8192, 700, 17), (8192, 700, 32), (3968, 1253, 12), (4032, 200, 12),
           (64, 40, 12), (3968, 5, 12), (8000, 200, 12)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("skip")
    (d / "h.cpp").write_text(HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}", str(d / "h.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def row_set(tok, i):
    """(rows as a set of cell rows, map rows, next index) of a printed row span."""
    n = int(tok[i])
    rows, cells = set(), set()
    for k in range(n):
        r, bits = int(tok[i + 1 + 2 * k]), int(tok[i + 2 + 2 * k])
        cells.add(r)
        got = {32 * r + b for b in range(32) if bits >> b & 1}
        assert got and not (rows & got), (r, bits)  # no empty map row, no row twice
        rows |= got
    return rows, cells, i + 1 + 2 * n


def plan(exe, nx, ny, m, mapfile=None, window=WINDOW):
    """{(tx, ty): dict} and (ncol, nrow)."""
    W, T = nx // 64, window - 2 * m
    cmd = [exe, str(W), str(ny), str(T), str(m)] + ([mapfile] if mapfile else [])
    lines = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.splitlines()
    g = lines[0].split()
    assert g[:4] == ["G", "32", "62", "3"], g
    tiles = {}
    for ln in lines[1:]:
        tok = ln.split()
        rows, rcells, i = row_set(tok, 2)
        left, right, n = int(tok[i]), int(tok[i + 1]), int(tok[i + 2])
        cols = {int(t) for t in tok[i + 3:i + 3 + n]}
        own, ocells, i = row_set(tok, i + 3 + n)
        assert i == len(tok) - 1
        tiles[(int(tok[0]), int(tok[1]))] = dict(rows=rows, rcells=rcells, left=left, right=right, cols=cols, own=own,
                                                 ocells=ocells, live=int(tok[i]))
    return tiles, (int(g[4]), int(g[5]))


@pytest.mark.parametrize("nx,ny,m,window",
                         default_shape(GEOMS) + shaped(WINDOW, GEOMS_DEEP) + shaped(WINDOW16, GEOMS16))
def test_read_and_owned_sets_match_brute_force(harness, nx, ny, m, window):
    W, T = nx // 64, window - 2 * m
    assert T > 0
    tiles, (ncol, nrow) = plan(harness, nx, ny, m, window=window)
    ntx, nty = -(-W // 62), -(-ny // T)
    assert (ncol, nrow) == (ntx, -(-ny // 32))
    assert sorted(tiles) == sorted((tx, ty) for ty in range(nty) for tx in range(ntx))
    for (tx, ty), t in tiles.items():
        y0, y1 = ty * T, min(ty * T + T, ny)
        p0, p1 = 62 * tx, min(62 * tx + 62, W)
        rows = {y % ny for y in range(y0 - m, y1 + m)}
        pairs = [p % W for p in range(p0 - 1, p1 + 1)]
        # map cells: exactly those the window touches, rows and columns
        assert t["rcells"] == {y // 32 for y in rows}, (tx, ty)
        assert t["cols"] == {p // 62 for p in pairs}, (tx, ty)
        assert t["cols"] == {t["left"], tx, t["right"]}, (tx, ty)
        assert max(t["rcells"]) < nrow and max(t["cols"]) < ncol
        # finer: exactly the window's rows; the edge lane columns as the last / first pair of their map column
        assert t["rows"] == rows, (tx, ty)
        pl, pr = pairs[0], pairs[-1]
        assert t["left"] == pl // 62 and pl == min(62 * t["left"] + 61, W - 1), (tx, ty)
        assert t["right"] == pr // 62 and pr == 62 * t["right"], (tx, ty)
        assert t["own"] == set(range(y0, y1)) and t["ocells"] == {y // 32 for y in range(y0, y1)}, (tx, ty)


def test_short_last_tile_row_reaches_two_tile_rows_up(harness):
    """3968 x 1349 at m = 12: the last tile row holds rows [1344, 1349), fewer than m, so tile
    row 0's window starts at row 1337, inside the tile row before the last."""
    tiles, _ = plan(harness, 3968, 1349, 12)
    assert {1337, 1343, 1344, 1348, 0, 179} <= tiles[(0, 0)]["rows"] and 1336 not in tiles[(0, 0)]["rows"]
    assert tiles[(0, 8)]["own"] == set(range(1344, 1349))


def sparse_state(nx, ny, seed, corner_y=168):
    """A few 6 x 6 soups, some straddling the tile corner (3968, corner_y) and the periodic corner."""
    rng = np.random.default_rng(seed)
    g = np.zeros((ny, nx), np.uint8)
    spots = [(3968 % nx - 3, corner_y % ny - 3), (nx - 3, ny - 3), (int(rng.integers(nx)), int(rng.integers(ny))),
             (int(rng.integers(nx)), int(rng.integers(ny)))]
    for x, y in spots[seed % 2:]:
        blob = (rng.random((6, 6)) < 0.5).astype(np.uint8)
        for j in range(6):
            for i in range(6):
                g[(y + j) % ny, (x + i) % nx] |= blob[j, i]
    return g


def activity_map(g, ncol, nrow):
    """The map words of a state: [nrow][ncol][any, first, last] row masks."""
    ny, nx = g.shape
    W = nx // 64
    pairs = g.reshape(ny, W, 64).any(axis=2)
    words = np.zeros((nrow, ncol, 3), np.uint32)
    for c in range(ncol):
        p0, p1 = 62 * c, min(62 * c + 62, W)
        for k, rowlive in enumerate((pairs[:, p0:p1].any(axis=1), pairs[:, p0], pairs[:, p1 - 1])):
            for y in np.nonzero(rowlive)[0]:
                words[y // 32, c, k] |= np.uint32(1 << (y % 32))
    return words


@pytest.mark.parametrize("nx,ny,m,window",
                         default_shape([(8192, 700, 12), (8192, 700, 5), (3968, 1349, 12), (4096, 200, 12)]) +
                         shaped(WINDOW16, [(8192, 700, 12), (8192, 700, 32), (3968, 1253, 12)]))
def test_model_pass_skips_only_dead_blocks(harness, oracle, tmp_path, nx, ny, m, window):
    W, T = nx // 64, window - 2 * m
    skipped = ran = 0
    for seed in (1, 2, 3):
        # (the default shape's cases keep their corner spot at row 168, whatever their m)
        g = sparse_state(nx, ny, seed, 168 if window == WINDOW else T)
        ncol, nrow = -(-W // 62), -(-ny // 32)
        f = tmp_path / f"map{seed}.bin"
        activity_map(g, ncol, nrow).tofile(f)
        tiles, _ = plan(harness, nx, ny, m, str(f), window=window)
        want = oracle.life_run(g, m)
        for (tx, ty), t in tiles.items():
            y0, y1 = ty * T, min(ty * T + T, ny)
            x0, x1 = 64 * 62 * tx, min(64 * (62 * tx + 62), nx)
            ys = [y % ny for y in range(y0 - m, y1 + m)]
            xs = [x % nx for x in range(x0 - 64, x1 + 64)]
            window_live = bool(g[np.ix_(ys, xs)].any())
            assert t["live"] == int(window_live), (seed, tx, ty)  # exact to the row and the edge pair
            if t["live"]:
                ran += 1
            else:
                skipped += 1
                assert not want[y0:y1, x0:x1].any(), (seed, tx, ty)
    assert ran > 0
    assert skipped > 0 or len(tiles) <= 4


@pytest.mark.parametrize("nx,ny,m", [(8192, 700, 12), (8192, 700, 32), (3968, 1349, 12)])
def test_model_pass_at_light_speed(harness, tmp_path, nx, ny, m):
    """The window is tight from both sides at c.  Every pattern above moves at most a row per two generations,
    so a window of m / 2 ghost rows would pass.  Under the parity rule (rule_ref.PARITY) one cell is, m
    generations on, alive at (+-m, +-m) whatever else the grid holds: for each tile, a single cell on the
    exact diagonal north-west of its block's first cell and south-east of its last one, wraps included --
    at distance m the tile must run, and rule_ref.parity_run puts a live cell into its block, namely that
    corner; at distance m + 1 it must not run, and every tile that is not run is all dead after m
    generations."""
    import rule_ref

    W, T = nx // 64, WINDOW - 2 * m
    ncol, nrow = -(-W // 62), -(-ny // 32)
    f = tmp_path / "map.bin"
    g = np.zeros((ny, nx), np.uint8)
    blocks = {(tx, ty): (ty * T, min(ty * T + T, ny), 64 * 62 * tx, min(64 * (62 * tx + 62), nx))
              for ty in range(-(-ny // T)) for tx in range(ncol)}
    for (tx, ty), (y0, y1, x0, x1) in blocks.items():
        for cx, cy, sign in ((x0, y0, -1), (x1 - 1, y1 - 1, 1)):
            for d in (m, m + 1):
                x, y = (cx + sign * d) % nx, (cy + sign * d) % ny
                g[y, x] = 1
                activity_map(g, ncol, nrow).tofile(f)
                tiles, _ = plan(harness, nx, ny, m, str(f))
                want = rule_ref.parity_run(g, m)
                g[y, x] = 0
                where = (tx, ty, cx, cy, d)
                assert tiles[(tx, ty)]["live"] == int(d == m), where
                if d == m:
                    assert want[cy, cx] == 1, where
                for t, (b0, b1, a0, a1) in blocks.items():
                    if not tiles[t]["live"]:
                        assert not want[b0:b1, a0:a1].any(), (where, t)
