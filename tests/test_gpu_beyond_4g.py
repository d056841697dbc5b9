"""Grids beyond 2^32 cells and 4 GiB buffers, pinned to the CPU oracle by windows.

Above 65536^2 the rest of the suite compares one HIP run with another by
census.  Here every expected value comes from the oracle (fill_random_window,
fill_random, life_run: 3-life/life2d.c:104-130 restated) and from numpy written
in this file, at three shapes, the smallest that cross each line:

  S1  bit   131072 x  32800   cell index 2^32 at row 32768
  S2  byte   65536 x  66560   byte offset 4 GiB in the padded buffer
  S3  bit   262144 x 131072   both, in one shard (the C5 grid, index < 2^35)

y4 is the first owned row whose byte offset (y + yapron) * pitch reaches 4 GiB,
taken from the layout, never from constants.

Places (centres of the windows and patches; `places`):

  line     (0, 2^32 / nx): across the x seam, on the row where y * nx crosses
           2^32.  S2 has that row too (65536, above its y4), so it is taken
           there as well.
  corner   (0, 0): across both periodic seams, four pieces for gather_rect.
  above4g  rows above y4, away from every seam (S2, S3).
  meet     partitioned: the point where four blocks meet.
  edge     partitioned: a block corner on the y seam, its upper half above
           row 32768 (S1) or y4 (S3).

Phase A (dense soup): fill_random, then at every place gather_rect of the
inner 512 x 256 window plus a margin of gens + 2 equals the oracle's window;
after step(gens) the inner window equals the inner part of the oracle's run of
the window as a small torus (wrong values enter at the cut edges and move one
cell per generation).

Phase B (soup patches in a dead universe): the whole-grid census, live count
and density map have an exact oracle value at any size.  clear() on a device
created under LIFE_POISON=1 (every device here is), one 640 x 400 patch of soup
per place loaded with set_cells from one shuffled coordinate list, then live
count, checksum, every patch window and three density maps (4096 x 4096 and
two pairs of factors that do not divide the grid) against the patches evolved
on their own small tori, before and after step(gens); a factor pair with
fx * fy >= 2^32 raises LifeError.  S1's rows leave
32 rows between `line` and the y seam, so its `corner` patch would lie on top
of the `line` patch and is not placed: the `line` patch there straddles both
seams itself (`patch_places`).

The helpers below import without a GPU; tests/test_beyond_4g_reference.py
proves the reference side on a scaled-down universe against the oracle's run
of the full grid.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INNER_W, INNER_H = 512, 256
PATCH_W, PATCH_H = 640, 400
SOUP_SEED = 2025
GOLD = 0x9E3779B97F4A7C15
LIFE_EINVAL = -1


class Shape(NamedTuple):
    id: str
    kernel: str
    nx: int
    ny: int
    gens: int  # bit: two full K = 32 exchanges + a partial one; byte: two passes


SHAPES = {s.id: s for s in (Shape("S1", "bit", 131072, 32800, 70), Shape("S2", "byte", 65536, 66560, 40),
                            Shape("S3", "bit", 262144, 131072, 70))}


class Device(NamedTuple):
    id: str
    shape: str
    shards: int
    dims: tuple
    flow: Optional[int]


DEVICES = [Device("S1-flow0", "S1", 1, (0, 0), 0), Device("S1-default", "S1", 1, (0, 0), None),
           Device("S1-2x2", "S1", 4, (2, 2), None), Device("S2", "S2", 1, (0, 0), None),
           Device("S3", "S3", 1, (0, 0), None), Device("S3-4x2", "S3", 8, (4, 2), None)]


class Place(NamedTuple):
    name: str
    cx: int
    cy: int


# ------------------------------------------------------------ where the lines are
def margin(gens):
    return gens + 2


def first_row_above_4g(L, ny):
    """The first owned row whose byte offset in the padded buffer is >= 2^32
    (owned row y starts at (y + yapron) * pitch), or None if the block ends
    below it."""
    y4 = -(-2**32 // L.pitch) - L.yapron
    return y4 if y4 < ny else None


def index_line_row(nx, ny):
    """The row whose first cell has index exactly 2^32, or None."""
    y, rem = divmod(2**32, nx)
    return y if rem == 0 and y < ny else None


def places(nx, ny, origins, yline, y4, gens):
    """The window centres of a device: origins = the (x0, y0) of its shards'
    blocks, yline = index_line_row, y4 = first_row_above_4g of the
    single-shard layout."""
    m = margin(gens)
    out = []
    if yline is not None:
        out.append(Place("line", 0, yline))
    out.append(Place("corner", 0, 0))
    if y4 is not None:
        p = Place("above4g", nx * 11 // 16 + 37, ny - 300)
        assert y4 < p.cy - PATCH_H // 2 - m and p.cy + PATCH_H // 2 + m < ny, (p, y4)
        out.append(p)
    if len(origins) > 1:
        xs, ys = sorted({x for x, _ in origins}), sorted({y for _, y in origins})
        out.append(Place("meet", xs[-1], ys[-1]))  # as _seams in test_gpu_sparse_io.py
        out.append(Place("edge", xs[1] if len(xs) > 1 else 0, 0))
    return tuple(out)


def _wrap_dist(a, b, n):
    return min((a - b) % n, (b - a) % n)


def patch_places(pl, nx, ny, gens):
    """The places that get a patch: every place whose patch plus margin stays
    clear of the patches before it (boxes of one size meet iff their centres
    are closer than the box in x and in y)."""
    m = margin(gens)
    out = []
    for p in pl:
        if all(_wrap_dist(p.cx, q.cx, nx) >= PATCH_W + 2 * m or _wrap_dist(p.cy, q.cy, ny) >= PATCH_H + 2 * m
               for q in out):
            out.append(p)
    return tuple(out)


def inner_origin(p):
    return p.cx - INNER_W // 2, p.cy - INNER_H // 2


def patch_origin(p):
    return p.cx - PATCH_W // 2, p.cy - PATCH_H // 2


# ------------------------------------------------------------ phase A reference
def oracle_window(O, nx, ny, x0, y0, w, h, seed):
    """fill_random's cells of the periodic w x h window at (x0, y0): the
    oracle's window wraps x but not y, so one across the y seam is two calls
    stacked."""
    ay = y0 % ny
    h1 = min(h, ny - ay)
    top = O.fill_random_window(nx, x0, ay, w, h1, seed, 0.5)
    if h1 == h:
        return top
    return np.concatenate([top, O.fill_random_window(nx, x0, 0, w, h - h1, seed, 0.5)])


@functools.lru_cache(maxsize=None)
def soup_windows(nx, ny, gens, pl):
    """Per place: the soup's window with margin, and its inner part after
    `gens` generations of the window as a torus (shared, read-only)."""
    import oracle as O

    m = margin(gens)
    out = {}
    for p in pl:
        x0, y0 = inner_origin(p)
        w0 = oracle_window(O, nx, ny, x0 - m, y0 - m, INNER_W + 2 * m, INNER_H + 2 * m, SOUP_SEED)
        w1 = np.ascontiguousarray(O.life_run(w0, gens, threads=4)[m:-m, m:-m])
        for a in (w0, w1):
            a.setflags(write=False)
        out[p] = (w0, w1)
    return out


# ------------------------------------------------------------ phase B reference
def evolve_patches(O, pp, gens, m):
    """Per patch place: the 640 x 400 soup embedded in a dead (400 + 2m) x
    (640 + 2m) array and run `gens` generations as a torus.  Its outer 2-cell
    frame must still be dead: nothing wrapped, the torus was the infinite
    plane (light speed guarantees it for m >= gens + 2)."""
    out = []
    for k, p in enumerate(pp):
        a = np.zeros((PATCH_H + 2 * m, PATCH_W + 2 * m), np.uint8)
        a[m:m + PATCH_H, m:m + PATCH_W] = O.fill_random(PATCH_W, PATCH_H, seed=100 + k, density=0.5)
        a = O.life_run(a, gens, threads=4)
        frame = a.copy()
        frame[2:-2, 2:-2] = 0
        assert not frame.any(), f"patch {p}: live cells in the outer frame after {gens} generations"
        a.setflags(write=False)
        out.append(a)
    return out


def expected_cells(nx, ny, pp, arrays, m):
    """The live cells of the whole universe: the union of the patch arrays'
    cells at ((x0 + xs) % nx, (y0 + ys) % ny)."""
    gx, gy = [], []
    for p, a in zip(pp, arrays):
        ox, oy = patch_origin(p)
        ys, xs = np.nonzero(a)
        gx.append((xs.astype(np.int64) + (ox - m)) % nx)
        gy.append((ys.astype(np.int64) + (oy - m)) % ny)
    gx, gy = np.concatenate(gx), np.concatenate(gy)
    assert len(np.unique(gy * nx + gx)) == len(gx), "patches overlap"
    return gx, gy


def census_of_cells(gx, gy, nx):
    """(live count, sum of mix64(gy * nx + gx + 1) mod 2^64) from coordinates."""
    v = gy.astype(np.uint64) * np.uint64(nx) + gx.astype(np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        t = v * np.uint64(GOLD)
    return len(gx), int(np.sum(t ^ (t >> np.uint64(29)), dtype=np.uint64))


def density_of_cells(gx, gy, nx, ny, fx, fy):
    exp = np.zeros((-(-ny // fy), -(-nx // fx)), np.uint32)
    np.add.at(exp, (gy // fy, gx // fx), 1)
    return exp


def odd_factors(pp, nx, ny):
    """Density factors that do not divide the grid, with a bin edge inside a
    patch: 11 * fy within 21 rows of a patch centre, 51 * fx within 101 columns
    of one (where a patch lies off the x seam; else 5000, whose last, partial
    bin ends at the seam inside a patch)."""
    cy = next(p.cy for p in pp if p.cy >= PATCH_H)
    fy = (cy // 11) | 1
    cx = next((p.cx for p in pp if p.cx >= PATCH_W), None)
    fx = 5000 if cx is None else (cx // 51) | 1
    assert nx % fx and ny % fy and abs(11 * fy - cy) < PATCH_H // 2 and (cx is None or abs(51 * fx - cx) < PATCH_W // 2)
    return fx, fy


def cell_list(gx, gy, nx, ny, seed=1):
    """(x, y) rows for set_cells: shuffled, the first 10 % repeated, a third
    shifted by whole periods (+nx, -ny, +3 nx), as _cell_list in
    test_gpu_sparse_io.py."""
    cells = np.stack([gx, gy], axis=1).astype(np.int64)
    np.random.default_rng(seed).shuffle(cells)
    cells = np.concatenate([cells, cells[: (len(cells) + 9) // 10]])
    k = np.arange(len(cells))
    cells[k % 9 == 0, 0] += nx
    cells[k % 9 == 3, 1] -= ny
    cells[k % 9 == 6, 0] += 3 * nx
    return cells


@functools.lru_cache(maxsize=None)
def patch_states(nx, ny, gens, pp):
    """Generation 0 and generation `gens` of the patches: (arrays, gx, gy)
    each (shared, read-only)."""
    import oracle as O

    m = margin(gens)
    out = {}
    for g in (0, gens):
        arrays = evolve_patches(O, pp, g, m)
        gx, gy = expected_cells(nx, ny, pp, arrays, m)
        gx.setflags(write=False)
        gy.setflags(write=False)
        out[g] = (arrays, gx, gy)
    return out


# ------------------------------------------------------------ the devices
def single_layout(lm, sh):
    return lm.layout_query(sh.nx, sh.ny, (1, 1), 0, sh.kernel)


@pytest.fixture(scope="module", params=DEVICES, ids=[d.id for d in DEVICES])
def device(request, gpu):
    """One handle per device for both phases: the large buffers are allocated
    once, under LIFE_POISON=1 (read at each create), so they start as 0xA5."""
    dev = request.param
    sh = SHAPES[dev.shape]
    mp = pytest.MonkeyPatch()
    mp.setenv("LIFE_POISON", "1")
    try:
        life = gpu.Life(sh.nx, sh.ny, shards=dev.shards, kernel=sh.kernel, dims=dev.dims, flow=dev.flow,
                        transport=gpu.XPORT_LOCAL if dev.shards > 1 else gpu.XPORT_AUTO)
    finally:
        mp.undo()
    with life:
        lays = [life.layout(i) for i in range(life.world()["nlocal"])]
        assert len(lays) == dev.shards
        L1 = single_layout(gpu, sh)
        if dev.shards == 1:
            assert (lays[0].pitch, lays[0].yapron, lays[0].rows) == (L1.pitch, L1.yapron, L1.rows)
        y4 = first_row_above_4g(L1, sh.ny)
        if dev.shape != "S1":  # a layout change must not leave the line uncrossed
            assert y4 is not None and 0 < y4 < sh.ny - 600, (L1.pitch, L1.yapron, y4)
        yline = index_line_row(sh.nx, sh.ny)
        assert yline is not None
        pl = places(sh.nx, sh.ny, [(L.x0, L.y0) for L in lays], yline, y4, sh.gens)
        yield life, dev, sh, pl


def _tag(dev, p, life=None):
    return f"{dev.id} {p.name} centre ({p.cx}, {p.cy})" + (f" path={life.last_path()}" if life else "")


# ------------------------------------------------------------ phase B
def _check_sparse(life, dev, sh, pp, state, when):
    arrays, gx, gy = state
    m = margin(sh.gens)
    live, ck = census_of_cells(gx, gy, sh.nx)
    assert life.live_count() == live, f"{dev.id} {when} path={life.last_path()}"
    assert life.checksum() == ck, f"{dev.id} {when} path={life.last_path()}"
    for p, a in zip(pp, arrays):
        ox, oy = patch_origin(p)
        got = life.gather_rect(ox - m, oy - m, PATCH_W + 2 * m, PATCH_H + 2 * m)
        np.testing.assert_array_equal(got, a, err_msg=f"{_tag(dev, p, life)} {when}")
    for fx, fy in [(4096, 4096), (5000, 3001), odd_factors(pp, sh.nx, sh.ny)]:
        got = life.gather_density(fx, fy)
        np.testing.assert_array_equal(got, density_of_cells(gx, gy, sh.nx, sh.ny, fx, fy),
                                      err_msg=f"{dev.id} {when} factors {(fx, fy)}")


def test_sparse_patches_in_a_dead_universe(device, gpu, oracle):
    """Defined before phase A: the first call on the fresh, poisoned buffers
    is clear(), so a memset that stops at 4 GiB leaves 0xA5 cells."""
    life, dev, sh, pl = device
    pp = patch_places(pl, sh.nx, sh.ny, sh.gens)
    assert len(pp) == len(pl) - (dev.shape == "S1")  # S1: `corner` lies on `line`
    life.clear()
    assert life.live_count() == 0, dev.id
    assert life.checksum() == 0, dev.id
    st = patch_states(sh.nx, sh.ny, sh.gens, pp)
    _, gx0, gy0 = st[0]
    life.set_cells(cell_list(gx0, gy0, sh.nx, sh.ny))
    _check_sparse(life, dev, sh, pp, st[0], "after set_cells")
    life.step(sh.gens)
    _check_sparse(life, dev, sh, pp, st[sh.gens], f"after {sh.gens} generations")
    with pytest.raises(gpu.LifeError) as e:  # fx * fy >= 2^32: a bin could overflow uint32
        life.gather_density(65536, 65536)
    assert e.value.rc == LIFE_EINVAL


# ------------------------------------------------------------ phase A
def test_dense_soup_windows_against_the_oracle(device, oracle):
    life, dev, sh, pl = device
    m = margin(sh.gens)
    wins = soup_windows(sh.nx, sh.ny, sh.gens, pl)
    life.fill_random(SOUP_SEED, 0.5)
    for p in pl:
        x0, y0 = inner_origin(p)
        got = life.gather_rect(x0 - m, y0 - m, INNER_W + 2 * m, INNER_H + 2 * m)
        np.testing.assert_array_equal(got, wins[p][0], err_msg=f"{_tag(dev, p)} fill")
    life.step(sh.gens)
    for p in pl:
        x0, y0 = inner_origin(p)
        got = life.gather_rect(x0, y0, INNER_W, INNER_H)
        np.testing.assert_array_equal(got, wins[p][1], err_msg=f"{_tag(dev, p, life)} after {sh.gens} generations")
