"""Every ghost zone of the bit path at light speed, under the parity rule.

B1357/S1357 (rule_ref.PARITY): the next state of a cell is the XOR of its eight
neighbours.  The rule is linear over GF(2), so one input cell changes, m
generations on, a pattern whose bounding box is exactly (2m + 1)^2 with all
four corners (+-m, +-m) and the four axis points alive, WHATEVER the other
cells hold (tests/test_light_cone_host.py): a single wrong, stale or missing
cell at the full depth m of a ghost zone always flips an owned cell.  B3/S23
and HighLife soups, which the rest of the suite runs, lose such a cell on the
way in almost every trial (the host module prints the rates).

The tile geometry, the halo plan, banded columns and the pipelined passes are
rule-independent bodies; what the parity rule pins on the
table-rule instances is the geometry B3/S23 runs on:

a. m ghost rows above and below a tile, m = 1..32, at both tile heights;
b. the K = 32 aprons and 64 x 32 corner blocks of partitioned shards, one
   exchange feeding up to three passes (deep halo), both schedules;
c. the same aprons through the loopback, per axis;
d. the one-cell aprons of the one-generation kernel;
e. the region waits of pipelined passes;
f. the window of a skip-dead tile, from both sides, at c.

Every comparison is over the whole grid, bit-exact, with live_count() and
last_path().  The reference is rule_ref.parity_run, a closed form that does no
stepping; tests/test_light_cone_host.py pins it to rule_ref.rule_run on the
states and generation counts of this module (STATES below is that list).
"""
import numpy as np
import pytest

import rule_ref as R

pytestmark = pytest.mark.gpu

RULE = "B1357/S1357"
SEED = 7
K = 32  # generations per halo exchange of the temporal bit layout (life_mi355x.TEMPORAL_DEPTH)

# ------------------------------------------------------------ shapes and call lists (the host module reads these)
WIDE = (4160, 300)  # 65 pairs: one full tile column and a banded one of 3 pairs; 2 to 5 tile rows, the last partial
DEPTHS = range(1, 33)
# shards, dims, nx, ny: 2-D partitions (corner blocks), a block of one pair, x-only
PARTS = [(4, (2, 2), 260, 260), (6, (3, 2), 2000, 333), (8, (4, 2), 512, 300), (8, (1, 8), 64, 320),
         (2, (2, 1), 640, 96)]
# tests/test_gpu_parity.py test_deep_halo's calls: (generations, BLOCK_GENS | "off" | "on" | None)
DEEP_CALLS = [(5, None), (20, None), (7, None), (31, 32), (12, 12), (9, "off"), (33, None), (1, "on"), (24, None)]
EXACT_CALLS = (32, 12)  # one K-deep apron consumed to its last row, then the refill
LOOP_CALLS = (5, 20, 32)
ONEGEN = [(4, (4, 1), 122, 517), (4, (2, 2), 100, 40), (1, (1, 1), 31, 13)]
ONEGEN_CALLS = (1, 4, 5)
PIPE = [(24, 4160, 1400, (3, 2, 2, 2)), (16, 4160, 1400, (4, 4, 3, 3)), (16, 4160, 1253, (4, 3, 3, 3))]
PIPE_GENS = 48
NX, NY = 8192, 700  # skip-dead: tile columns of 62, 62 and 4 pairs
LONE = (5000, 300)
LONE_CALLS = (61, 3)
PASTE = (200, 160)
PASTE_CALLS = (12, 49)


def cumulative(calls):
    return tuple(int(n) for n in np.cumsum(calls))


def cells_grid(cells, nx=NX, ny=NY):
    g = np.zeros((ny, nx), np.uint8)
    for x, y in cells:
        g[y % ny, x % nx] = 1
    return g


def paste_origin(rows=24):
    """The soup window's origin: centred on the tile corner (3968, 8 rows - 24) of 12-generation passes."""
    return 3968 - PASTE[0] // 2, 8 * rows - 24 - PASTE[1] // 2


def paste_grid(rows=24):
    x0, y0 = paste_origin(rows)
    g = np.zeros((NY, NX), np.uint8)
    g[y0:y0 + PASTE[1], x0:x0 + PASTE[0]] = R.soup(*PASTE, SEED)
    return g


def soup_state(nx, ny):
    return lambda: R.soup(nx, ny, SEED)


# (name, initial state, cumulative generation counts): every state the device is compared on, but for the one-pass
# single cells at the tile corners
STATES = ([("wide", soup_state(*WIDE), tuple(DEPTHS) + cumulative(LOOP_CALLS))] +
          [(f"part-{nx}x{ny}", soup_state(nx, ny), cumulative([c[0] for c in DEEP_CALLS]) + cumulative(EXACT_CALLS))
           for _, _, nx, ny in PARTS] +
          [(f"onegen-{nx}x{ny}", soup_state(nx, ny), cumulative(ONEGEN_CALLS)) for _, _, nx, ny in ONEGEN] +
          [(f"pipe-{nx}x{ny}", soup_state(nx, ny), (PIPE_GENS,)) for _, nx, ny, _ in PIPE[1:]] +
          [("lone-cell", lambda: cells_grid([LONE]), cumulative(LONE_CALLS)),
           ("paste", paste_grid, cumulative(PASTE_CALLS))])

_refs = {}


def ref(key, start, gens):
    """parity_run of the state `start()` after `gens` generations; computed once per module run, read-only."""
    have = _refs.setdefault(key, {})
    if 0 not in have:
        have[0] = start()
        have[0].setflags(write=False)
    if gens not in have:
        have[gens] = R.parity_run(have[0], gens)
        have[gens].setflags(write=False)
    return have[gens]


def soup_ref(nx, ny, gens):
    return ref((nx, ny), soup_state(nx, ny), gens)


def check(life, want, path):
    """The path, the whole grid and the live count."""
    assert life.last_path() == path
    np.testing.assert_array_equal(life.gather(), want)
    assert life.live_count() == int(want.sum())


@pytest.fixture
def tile_rows(gpu, request):
    """Bit tiles of `rows` register rows per wave for one test; the default is back afterwards, also on failure."""
    gpu.tune_temporal(request.param, "bit")
    try:
        yield request.param
    finally:
        gpu.tune_temporal(gpu.TEMPORAL_ROWS["bit"], "bit")


def rows(*values):
    return pytest.mark.parametrize("tile_rows", values, indirect=True, ids=[f"rows{v}" for v in values])


def schedule(gens, bmax, deep, since=0):
    """The pass lengths life::next_pass cuts a call into (tests/test_host_plan.py pins the function itself)."""
    out = []
    while gens:
        seg = min(gens, K - since) if deep and since < K else gens
        n = -(-seg // bmax)
        m = -(-seg // n)
        if since + m > K:
            since = 0
        extend = deep and since + m < K and not (gens == m and since + m + bmax > K)
        since = since + m if extend else 0
        out.append(m)
        gens -= m
    return out


# ------------------------------------------------------------ a. every ghost depth
@rows(24, 16)
@pytest.mark.parametrize("m", DEPTHS)
def test_every_ghost_depth(gpu, tile_rows, m):
    """One pass of m generations over 4160 x 300: windows of 8 x rows rows owning T = 8 rows - 2m, so 2 tile
    rows (24-row waves, m <= 21) to 5 (16-row waves, m >= 27), the last partial and wrapping into tile row 0's
    ghost rows.  At 16 rows whole waves are ghost from m = 17 and T = 64 at m = 32."""
    with gpu.Life(*WIDE, kernel="bit", rule=RULE) as life:
        life.configure(gpu.OPT_BLOCK_GENS, m)
        life.upload(soup_ref(*WIDE, 0))
        life.step(m)
        assert life.call_stats()["passes"] == 1
        check(life, soup_ref(*WIDE, m), "tiles")


# ------------------------------------------------------------ b. deep halo, corner blocks, both schedules
def sharded(gpu, shards, dims, nx, ny, overlap):
    return gpu.Life(nx, ny, shards=shards, dims=dims, kernel="bit", transport=gpu.XPORT_LOCAL, overlap=overlap,
                    rule=RULE)


PARTITIONED = pytest.mark.parametrize("shards,dims,nx,ny", PARTS, ids=[f"{p[2]}x{p[3]}" for p in PARTS])
SCHEDULES = pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])


@SCHEDULES
@PARTITIONED
@pytest.mark.parametrize("deep", [1, 0], ids=["deep", "per-pass"])
def test_deep_halo_aprons_and_corner_blocks(gpu, shards, dims, nx, ny, overlap, deep):
    """test_deep_halo's calls: 1, 2 and 3 passes between exchanges, a pass longer than planned (the exchange is
    forced first), deep off mid-run (the aprons are refilled); compared after every call, with the deep halo
    and with one exchange per pass."""
    with sharded(gpu, shards, dims, nx, ny, overlap) as life:
        life.configure(gpu.OPT_DEEP_HALO, deep)
        life.upload(soup_ref(nx, ny, 0))
        done = 0
        for gens, opt in DEEP_CALLS:
            if opt == "off":
                life.configure(gpu.OPT_DEEP_HALO, 0)
            elif opt == "on":
                life.configure(gpu.OPT_DEEP_HALO, deep)
            elif opt is not None:
                life.configure(gpu.OPT_BLOCK_GENS, opt)
            life.step(gens)
            done += gens
            check(life, soup_ref(nx, ny, done), "tiles")


@SCHEDULES
@PARTITIONED
def test_deep_halo_consumes_an_apron_exactly(gpu, shards, dims, nx, ny, overlap):
    """BLOCK_GENS 12 and step(32) on freshly filled aprons: the passes use the K = 32 apron rows and the corner
    blocks down to the last one before the next exchange; then a call that starts with the refilled ones."""
    want = schedule(EXACT_CALLS[0], 12, True)
    print(f"{nx} x {ny} {dims}: step({EXACT_CALLS[0]}) runs passes of {want}")
    assert sum(want) == EXACT_CALLS[0] == K and len(want) == 3
    with sharded(gpu, shards, dims, nx, ny, overlap) as life:
        life.configure(gpu.OPT_DEEP_HALO, 1)
        life.configure(gpu.OPT_BLOCK_GENS, 12)
        life.upload(soup_ref(nx, ny, 0))
        done = 0
        for gens in EXACT_CALLS:
            life.step(gens)
            done += gens
            assert life.call_stats()["passes"] == len(schedule(gens, 12, True))
            check(life, soup_ref(nx, ny, done), "tiles")


# ------------------------------------------------------------ c. loopback
@pytest.mark.parametrize("axes", [1, 2, 3], ids=["both", "x-only", "y-only"])
def test_loopback_aprons(gpu, axes):
    """The shard as a periodic partition of itself: the aprons of both axes, of x or of y come from halo
    messages to itself; 5 + 20 generations on one exchange, then 32."""
    with gpu.Life(*WIDE, kernel="bit", transport=gpu.XPORT_LOCAL, rule=RULE) as life:
        life.upload(soup_ref(*WIDE, 0))
        life.configure(gpu.OPT_LOOPBACK, axes)
        done = 0
        for gens in LOOP_CALLS:
            life.step(gens)
            done += gens
            check(life, soup_ref(*WIDE, done), "tiles")


# ------------------------------------------------------------ d. one-cell aprons
@pytest.mark.parametrize("shards,dims,nx,ny", ONEGEN, ids=[f"{p[2]}x{p[3]}" for p in ONEGEN])
def test_one_cell_aprons(gpu, shards, dims, nx, ny):
    """The one-generation kernel: blocks narrower than a pair (122 / 4, 100 / 2: no temporal layout), whose
    corner cells arrive through the phase order of the exchange, and 31 x 13 wrapping in its own aprons."""
    kw = dict(shards=shards, dims=dims, transport=gpu.XPORT_LOCAL) if shards > 1 else {}
    with gpu.Life(nx, ny, kernel="bit", rule=RULE, **kw) as life:
        assert life.layout().generations_per_exchange == 1
        life.upload(soup_ref(nx, ny, 0))
        done = 0
        for gens in ONEGEN_CALLS:
            life.step(gens)
            done += gens
            check(life, soup_ref(nx, ny, done), "onegen")


# ------------------------------------------------------------ e. pipelined passes
@pytest.mark.parametrize("tile_rows,nx,ny,regions", PIPE, indirect=["tile_rows"],
                         ids=[f"rows{p[0]}-{p[2]}" for p in PIPE])
def test_pipelined_region_waits(gpu, tile_rows, nx, ny, regions):
    """OPT_PIPELINE 4, 48 generations = 4 passes of 12 in 4 row regions on two streams: a region of pass p + 1
    starts when the regions of pass p its windows read are done.  1253 at 16 rows: a last tile row of 5 rows,
    fewer than m, so tile row 0's window reaches two tile rows up, across a region boundary.  The booked
    work is that of the regions (each lists its own banded items), not of whole launches."""
    import test_gpu_band_split as bs

    T = 8 * tile_rows - 24
    assert -(-ny // T) == sum(regions)
    with gpu.Life(nx, ny, kernel="bit", rule=RULE) as life:
        life.configure(gpu.OPT_PIPELINE, 4)
        life.configure(gpu.OPT_BLOCK_GENS, 12)
        life.upload(soup_ref(nx, ny, 0))
        life.set_timing(True)
        life.step(PIPE_GENS)
        assert life.call_stats()["passes"] == 4
        check(life, soup_ref(nx, ny, PIPE_GENS), "tiles")
        if bs.MODE == "0" and bs._flag("LIFE_BANDS"):  # (timing modes 1 / 2 run whole launches, 3 books nothing)
            items = sum(bs.items_of(nx, r) for r in regions)
            assert items != bs.items_of(nx, sum(regions))
            per_item = 64 * 8 * tile_rows * gpu.RULE_VALU_PER_PAIR_ROW * 12
            assert bs.booked(life) == pytest.approx(4 * items * per_item)


# ------------------------------------------------------------ f. skip-dead at c
def skipping(gpu):
    life = gpu.Life(NX, NY, kernel="bit", small_grid=False, skip_dead=True, rule=RULE)
    life.configure(gpu.OPT_BLOCK_GENS, 12)
    return life


def tiles_of(m, T):
    """(tx, ty, owned pairs, owned rows) of the plain tile grid of a skip-dead pass."""
    W = NX // 64
    return [(tx, ty, range(62 * tx, min(62 * tx + 62, W)), range(ty * T, min(ty * T + T, NY)))
            for ty in range(-(-NY // T)) for tx in range(-(-W // 62))]


def windows_holding(cell, m, T):
    """The tiles whose window -- owned rows +- m, owned pairs +- 1, both wrapped -- holds the cell."""
    W, (x, y) = NX // 64, cell
    return [(tx, ty) for tx, ty, pairs, ys in tiles_of(m, T)
            if y in {r % NY for r in range(ys[0] - m, ys[-1] + 1 + m)}
            and x // 64 in {p % W for p in range(pairs[0] - 1, pairs[-1] + 2)}]


CORNERS = [(24, (3968, 168), (1, 1)), (24, (NX, NY), (0, 0)), (16, (3968, 104), (1, 1)), (16, (NX, NY), (0, 0))]


@pytest.mark.parametrize("tile_rows,corner,tile", CORNERS, indirect=["tile_rows"],
                         ids=["rows24-tile-corner", "rows24-periodic-corner", "rows16-tile-corner",
                              "rows16-periodic-corner"])
@pytest.mark.parametrize("d", [12, 13], ids=["at-m", "at-m+1"])
def test_skip_window_is_tight_at_c(gpu, tile_rows, corner, tile, d):
    """One cell d cells north-west of a tile's corner on the exact diagonal, one pass of m = 12.  d = m: the
    cell lies in the deepest ghost row of the tile's window and reaches the tile's block in the corner cell
    alone, at generation 12; a plan that took a shallower window, or a map that lost the row, leaves it out.
    d = m + 1: the tile must not run.  The periodic corner reaches cell (0, 0) through both wraps and the
    4-pair last tile column.  The run counts are those of the window definition, by brute force."""
    m, T = 12, 8 * tile_rows - 24
    cell = (corner[0] - d, corner[1] - d)
    cx, cy = corner[0] % NX, corner[1] % NY
    assert (cx // 64 // 62, cy // T) == tile and cx % (62 * 64) == 0 and cy % T == 0
    holding = windows_holding(cell, m, T)
    print(f"cell {cell}: windows {holding}")
    assert len(holding) == (4 if d == m else 2) and (tile in holding) == (d == m)
    g0 = cells_grid([cell])
    want = R.parity_run(g0, m)
    _, _, pairs, ys = tiles_of(m, T)[tile[1] * 3 + tile[0]]
    block = want[ys[0]:ys[-1] + 1, 64 * pairs[0]:64 * (pairs[-1] + 1)]
    assert block.sum() == (1 if d == m else 0) and want[cy, cx] == (d == m)
    with skipping(gpu) as life:
        life.clear()
        life.set_cells([cell])
        life.step(m)
        passes, run, cleared, total = life.activity()
        print(f"passes {passes} run {run} cleared {cleared} total {total}")
        check(life, want, "skip")
        assert (passes, total) == (1, 3 * -(-NY // T))
        assert run == len(holding)


def live_windows(state, m, T):
    """The tiles of a pass of m generations whose window holds a live cell of `state`, cell by cell."""
    out = []
    for tx, ty, pairs, ys in tiles_of(m, T):
        rows_ = [r % NY for r in range(ys[0] - m, ys[-1] + 1 + m)]
        cols = [x % NX for x in range(64 * (pairs[0] - 1), 64 * (pairs[-1] + 2))]
        if state[np.ix_(rows_, cols)].any():
            out.append((tx, ty))
    return out


def test_skip_lone_cell_spreads_at_c(gpu):
    """One cell, 61 generations (passes of 11, 10, 10, 10, 10, 10): the pattern's front moves a cell per
    generation in all eight directions, from one tile's block into the windows of its neighbours; three
    more to generation 64, where it collapses to eight cells 64 away.  Every pass must run at least the
    tiles whose window holds a live cell of its input (brute force over the reference states).

    The first pass of the first call writes into the buffer whose content is unknown, so it clears every
    tile it does not run: cleared >= 14 there.  The call to generation 64 is one pass of 3 generations
    with tile rows of 186 rows; the buffer it writes into holds generation 51, whose cells (rows 249..351,
    columns 4949..5051) all lie in the block of tile (1, 1), which is run: no tile of that pass has to be
    cleared, whatever the collapse does to the pattern, so its count is printed and not asserted.  A block
    that should have been cleared and was not shows in the whole-grid comparison."""
    sizes = schedule(61, 12, False)
    assert sizes == [11, 10, 10, 10, 10, 10]
    start = lambda: cells_grid([LONE])  # noqa: E731
    need, done = 0, 0
    for m in sizes:
        need += len(live_windows(ref("lone", start, done), m, 192 - 2 * m))
        done += m
    first = len(live_windows(ref("lone", start, 0), 11, 170))
    with skipping(gpu) as life:
        life.clear()
        life.set_cells([LONE])
        life.step(61)
        passes, run, cleared, total = life.activity()
        print(f"step(61): passes {passes} run {run} (windows holding a live cell: {need}) cleared {cleared} "
              f"total {total}")
        check(life, ref("lone", start, 61), "skip")
        assert passes == 6 and total == 3 * 5 * 6 and need <= run < total
        assert first == 1 and cleared >= 3 * 5 - first
        life.step(3)
        passes, run, cleared, total = life.activity()
        need = len(live_windows(ref("lone", start, 61), 3, 186))
        print(f"step(3): passes {passes} run {run} (windows holding a live cell: {need}) cleared {cleared} "
              f"total {total}")
        want = ref("lone", start, 64)
        assert want.sum() == 8 and all(want[LONE[1] + 64 * j, LONE[0] + 64 * i]
                                       for i in (-1, 0, 1) for j in (-1, 0, 1) if i or j)
        check(life, want, "skip")
        assert (passes, total) == (1, 3 * 4) and need <= run < total


@rows(24, 16)
def test_skip_soup_window_under_poison(gpu, tile_rows, monkeypatch):
    """A 200 x 160 parity soup pasted over the tile corner on buffers that hold 0xA5 (LIFE_POISON is read at
    creation): 12 generations, then 49 (passes of 10, 10, 10, 10, 9), its edge moving out a cell per
    generation."""
    monkeypatch.setenv("LIFE_POISON", "1")
    x0, y0 = paste_origin(tile_rows)
    start = lambda: paste_grid(tile_rows)  # noqa: E731
    with skipping(gpu) as life:
        life.clear()
        life.set_rect(x0, y0, R.soup(*PASTE, SEED))
        np.testing.assert_array_equal(life.gather(), ref(("paste", tile_rows), start, 0))
        done = 0
        for gens in PASTE_CALLS:
            life.step(gens)
            done += gens
            passes, run, cleared, total = life.activity()
            print(f"step({gens}): passes {passes} run {run} cleared {cleared} total {total}")
            check(life, ref(("paste", tile_rows), start, done), "skip")
            assert passes == len(schedule(gens, 12, False)) and 0 < run < total


# ------------------------------------------------------------ afterwards
def test_default_tile_height_is_back(gpu):
    """After the tests above the process runs 24-row bit tiles again: a 12-generation pass over 4160 x 300 is
    2 tile rows of T = 168 (16-row waves: 3 of 104), which the booked work tells apart."""
    import test_gpu_band_split as bs

    with gpu.Life(*WIDE, kernel="bit", rule=RULE) as life:
        life.configure(gpu.OPT_BLOCK_GENS, 12)
        life.upload(soup_ref(*WIDE, 0))
        life.set_timing(True)
        life.step(12)
        check(life, soup_ref(*WIDE, 12), "tiles")
        if bs.MODE != "3":
            assert bs.booked(life) == pytest.approx(bs.items_of(4160, 2) * 64 * 8 * 24 *
                                                    gpu.RULE_VALU_PER_PAIR_ROW * 12)
