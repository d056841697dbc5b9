"""The reference side of tests/test_gpu_beyond_4g.py, proven on the CPU.

The GPU module's expected values come from helpers that place windows and
patches, wrap coordinates, hash cells from coordinates and bin them.  Here
the same helpers run on universes small enough for the oracle to hold
(4096 x 2048, 20 generations, the places at the same relative spots) and are
compared with the oracle's run of the FULL grid: np.take(mode="wrap") windows,
oracle.checksum, zero-pad + reshape + sum density -- none of it shared with
the helpers under test.
"""
import numpy as np
import pytest

import test_gpu_beyond_4g as B

NX, NY, GENS = 4096, 2048, 20
BLOCKS = [(0, 0), (2048, 0), (0, 1024), (2048, 1024)]
# yline, y4: S3-like (every place gets a patch) and S1-like (`line` 32 rows under the y seam)
UNIVERSES = {"S3-like": (1024, NY - 700), "S1-like": (NY - 32, None)}


def _window(grid, x0, y0, w, h):
    rows = np.take(grid, np.arange(y0, y0 + h), axis=0, mode="wrap")
    return np.take(rows, np.arange(x0, x0 + w), axis=1, mode="wrap")


def _density(grid, fx, fy):
    ny, nx = grid.shape
    bh, bw = -(-ny // fy), -(-nx // fx)
    pad = np.zeros((bh * fy, bw * fx), np.uint32)
    pad[:ny, :nx] = grid
    return pad.reshape(bh, fy, bw, fx).sum(axis=(1, 3)).astype(np.uint32)


def _places(name):
    yline, y4 = UNIVERSES[name]
    return B.places(NX, NY, BLOCKS, yline, y4, GENS)


def test_places_and_lines_of_the_real_shapes(lm):
    """Each shape crosses the line it is there for, by the library's own
    layout rule; the places sit where the module's docstring says."""
    want = {"S1": (32768, False), "S2": (65536, True), "S3": (16384, True)}
    for sh in B.SHAPES.values():
        L = B.single_layout(lm, sh)
        y4 = B.first_row_above_4g(L, sh.ny)
        yline = B.index_line_row(sh.nx, sh.ny)
        assert (yline, y4 is not None) == want[sh.id]
        assert yline * sh.nx == 2**32
        if y4 is not None:
            assert 0 < y4 < sh.ny - 600
            assert (y4 + L.yapron) * L.pitch >= 2**32 > (y4 - 1 + L.yapron) * L.pitch
        else:
            assert L.pitch * L.rows < 2**32
        pl = B.places(sh.nx, sh.ny, [(0, 0)], yline, y4, sh.gens)
        assert [p.name for p in pl] == ["line", "corner"] + ["above4g"] * (y4 is not None)
        pp = B.patch_places(pl, sh.nx, sh.ny, sh.gens)
        assert len(pp) == len(pl) - (sh.id == "S1")
    sh = B.SHAPES["S3"]
    org = [(lm.layout_query(sh.nx, sh.ny, (4, 2), r, "bit").x0, lm.layout_query(sh.nx, sh.ny, (4, 2), r, "bit").y0)
           for r in range(8)]
    pl = B.places(sh.nx, sh.ny, org, 16384, 130000, sh.gens)
    assert pl[3:] == (B.Place("meet", 196608, 65536), B.Place("edge", 65536, 0))
    assert B.patch_places(pl, sh.nx, sh.ny, sh.gens) == pl


@pytest.mark.parametrize("name", sorted(UNIVERSES))
def test_soup_window_reference(oracle, name):
    """Phase A's reference: the stacked oracle windows are the full grid's
    cells, and the window run as a torus equals the full run on its inner
    part."""
    pl = _places(name)
    m = B.margin(GENS)
    g0 = oracle.fill_random(NX, NY, B.SOUP_SEED, 0.5)
    g1 = oracle.life_run(g0, GENS, threads=4)
    wins = B.soup_windows(NX, NY, GENS, pl)
    assert len(wins) == len(pl) == (5 if name == "S3-like" else 4)
    for p in pl:
        x0, y0 = B.inner_origin(p)
        np.testing.assert_array_equal(wins[p][0], _window(g0, x0 - m, y0 - m, B.INNER_W + 2 * m, B.INNER_H + 2 * m),
                                      err_msg=str(p))
        np.testing.assert_array_equal(wins[p][1], _window(g1, x0, y0, B.INNER_W, B.INNER_H), err_msg=str(p))


@pytest.mark.parametrize("name", sorted(UNIVERSES))
def test_sparse_patch_reference(oracle, name):
    """Phase B's reference: the cell list, applied to a full grid and run by
    the oracle, gives the cells, census, windows and density maps the helpers
    derive from the patches alone."""
    pl = _places(name)
    pp = B.patch_places(pl, NX, NY, GENS)
    assert len(pp) == (5 if name == "S3-like" else 3)  # S1-like: `corner` lies on `line`
    m = B.margin(GENS)
    st = B.patch_states(NX, NY, GENS, pp)
    cells = B.cell_list(st[0][1], st[0][2], NX, NY)
    assert (cells[:, 0] >= NX).any() and (cells[:, 1] < 0).any()
    full = np.zeros((NY, NX), np.uint8)
    full[cells[:, 1] % NY, cells[:, 0] % NX] = 1
    for g in (0, GENS):
        arrays, gx, gy = st[g]
        if g:
            full = oracle.life_run(full, GENS, threads=4)
        ys, xs = np.nonzero(full)
        order = np.lexsort((gx, gy))  # row-major, as np.nonzero lists them
        assert np.array_equal(gy[order], ys) and np.array_equal(gx[order], xs)
        assert B.census_of_cells(gx, gy, NX) == (int(full.sum()), oracle.checksum(full))
        for p, a in zip(pp, arrays):
            ox, oy = B.patch_origin(p)
            np.testing.assert_array_equal(a, _window(full, ox - m, oy - m, B.PATCH_W + 2 * m, B.PATCH_H + 2 * m),
                                          err_msg=str(p))
        for fx, fy in [(512, 512), (5000, 3001), (1000, 301), B.odd_factors(pp, NX, NY)]:
            np.testing.assert_array_equal(B.density_of_cells(gx, gy, NX, NY, fx, fy), _density(full, fx, fy),
                                          err_msg=str((fx, fy)))
    # the patches moved: generation GENS is not generation 0 again
    assert not np.array_equal(st[0][1], st[GENS][1])


def test_census_of_cells_in_plain_integers():
    def mix(v):
        t = (v * B.GOLD) % 2**64
        return t ^ (t >> 29)

    nx = 262144
    gx = np.array([0, nx - 1, 5, nx - 1], np.int64)
    gy = np.array([16384, 16383, 131071, 131071], np.int64)  # indices 2^32, 2^32 - 1, ..., 2^35 - 1
    assert int(gy[3]) * nx + int(gx[3]) == 2**35 - 1
    want = sum(mix(int(y) * nx + int(x) + 1) for x, y in zip(gx, gy)) % 2**64
    assert B.census_of_cells(gx, gy, nx) == (4, want)
