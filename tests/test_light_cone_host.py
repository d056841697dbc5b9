"""What tests/test_gpu_light_cone.py leans on, checked on the CPU.

1. rule_ref.parity_run, the closed form the GPU module compares with, equals
   iterated rule_ref.rule_run under B1357/S1357 on the states and cumulative
   generation counts of that module (its STATES list; the largest grids at
   two counts).
2. The impulse facts: m generations after a single cell the pattern has its
   four corners (+-m, +-m) and four axis points (+-m, 0), (0, +-m) alive and a
   bounding box of exactly (2m + 1)^2, m = 1..32; hence every input cell
   within Chebyshev distance m of a block of at least 2m x 2m cells reaches
   an owned cell.  The rule is linear over GF(2): flipping that input cell
   flips that owned cell whatever the other cells hold.
3. Teeth: a numpy model of ghost-zone blocking computes one owned block from
   its window alone.  With the window one ghost row short, or with the single
   ghost cell at (m, m) wrong, the block differs from the truth for every seed
   under the parity rule; under B3/S23 mostly not (rates printed, not
   asserted) -- which is why the GPU module runs the parity rule.
"""
import numpy as np
import pytest

import rule_ref as R
import test_gpu_light_cone as glc

BIG = 4160 * 1400  # cells: the grids of about this size are stepped to two generation counts at most


def counts_to_step(gens, cells):
    gens = sorted(set(gens))
    return gens if cells < BIG // 2 else gens[-2:]


@pytest.mark.parametrize("name,start,gens", glc.STATES, ids=[s[0] for s in glc.STATES])
def test_closed_form_equals_stepping(name, start, gens):
    g0 = start()
    assert g0.size <= BIG
    g, done = g0, 0
    for n in counts_to_step(gens, g0.size):
        g = R.rule_run(g, n - done, R.PARITY)
        done = n
        np.testing.assert_array_equal(R.parity_run(g0, n), g, err_msg=f"{name}: generation {n}")


def test_closed_form_on_awkward_sizes():
    """Rolls longer than the grid and rolls that meet: 5 x 3, 7 x 64, 33 x 2, a single row."""
    for nx, ny in ((5, 3), (7, 64), (33, 2), (64, 1), (1, 1)):
        g0 = R.soup(nx, ny, nx + ny)
        for n in (0, 1, 2, 3, 7, 12, 25, 32, 45, 61):
            np.testing.assert_array_equal(R.parity_run(g0, n), R.rule_run(g0, n, R.PARITY), err_msg=f"{nx}x{ny} {n}")


def impulse(m, n=71):
    """The pattern m generations after the single cell (c, c) of an n x n grid, c = n // 2 (n > 2m + 2: no wrap)."""
    g = np.zeros((n, n + 2), np.uint8)
    g[n // 2, n // 2] = 1
    return R.parity_run(g, m)


@pytest.mark.parametrize("m", range(1, 33))
def test_one_cell_spreads_at_c_in_all_eight_directions(m):
    k, c = impulse(m), 71 // 2
    if m <= 12:
        g = np.zeros_like(k)
        g[c, c] = 1
        np.testing.assert_array_equal(k, R.rule_run(g, m, R.PARITY))
    for dx, dy in ((m, m), (m, -m), (-m, m), (-m, -m), (m, 0), (-m, 0), (0, m), (0, -m)):
        assert k[c + dy, c + dx] == 1, (dx, dy)
    ys, xs = np.nonzero(k)
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (c - m, c + m, c - m, c + m)
    # every cell within distance m of a 2m x 2m block reaches it: the number of the pattern's cells that land
    # in the block, for every offset of the input cell, from the pattern's integral image
    box = k[c - m:c + m + 1, c - m:c + m + 1].astype(np.int64)
    pad = np.zeros((6 * m + 1, 6 * m + 1), np.int64)  # the pattern, 2m clear cells around it
    pad[2 * m:4 * m + 1, 2 * m:4 * m + 1] = box
    s = np.zeros((6 * m + 2, 6 * m + 2), np.int64)
    s[1:, 1:] = pad.cumsum(0).cumsum(1)
    w = 2 * m  # windows of 2m x 2m at every offset at which they touch the pattern's box
    hits = s[w:, w:] - s[:-w, w:] - s[w:, :-w] + s[:-w, :-w]
    # window origin o (in pad coordinates) covers [o, o + 2m); the box spans [2m, 4m]: they meet for o in 1..4m
    assert (hits[1:4 * m + 1, 1:4 * m + 1] > 0).all()


def from_window(grid, y0, x0, b, m, rule, short_row=False, wrong_cell=False):
    """The b x b block at (y0, x0) after m generations, computed from its window of m ghost cells on every side
    alone: the window is cut out and stepped as a torus of its own, whose seam corrupts one ring per
    generation and, after m of them, has not reached the block.  short_row: the outermost ghost row above is
    not there (reads as dead).  wrong_cell: the ghost cell at (-m, -m) from the block's corner holds the
    complement of the true cell, as a stale or missing cell may (one that happens to hold the true value is
    no error)."""
    w = np.array(grid[y0 - m:y0 + b + m, x0 - m:x0 + b + m])
    if short_row:
        w[0, :] = 0
    if wrong_cell:
        w[0, 0] ^= 1
    return R.rule_run(w, m, rule)[m:m + b, m:m + b]


@pytest.mark.parametrize("m", [8, 12, 32])
def test_ghost_zone_model_has_teeth_under_parity(m):
    b, seeds = 48, range(20)
    caught = {(r, v): 0 for r in ("B1357/S1357", "B3/S23") for v in ("short_row", "wrong_cell")}
    for seed in seeds:
        n = b + 2 * m + 6
        grid = R.soup(n, n, seed, 0.45)
        y0 = x0 = m + 3
        for name in ("B1357/S1357", "B3/S23"):
            rule = R.NAMED[name]
            truth = R.rule_run(grid, m, rule)[y0:y0 + b, x0:x0 + b]
            np.testing.assert_array_equal(from_window(grid, y0, x0, b, m, rule), truth)  # the model itself
            for variant in ("short_row", "wrong_cell"):
                got = from_window(grid, y0, x0, b, m, rule, **{variant: True})
                caught[(name, variant)] += int(not np.array_equal(got, truth))
    for (name, variant), n in sorted(caught.items()):
        print(f"m = {m:2d} {name:12s} {variant:10s}: caught in {n} of {len(seeds)} seeds")
    assert caught[("B1357/S1357", "short_row")] == len(seeds)
    assert caught[("B1357/S1357", "wrong_cell")] == len(seeds)
