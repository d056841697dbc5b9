"""Every data-movement kernel of csrc/life_io.hip at the smallest shapes where
a swapped or dropped field of its block view (pitch, y-apron, x offset, w, h,
units, global origin) shows, in both encodings.

Expected values come from the CPU oracle (fill_random, life_run, checksum) and
plain numpy written here; nothing is compared with another device call.

* Single shard, nx in {1, 17, 65, 129, 200} x ny in {1, 3, 33}, streaming
  kernels (small_grid=False): fill_random, upload -> gather, gather_bits,
  gather_vtk, live_count, checksum, gather_rect (the whole grid and a window
  at (-3, -2) that wraps both axes: 9 x 5, clamped to the grid, which is the
  largest window the call accepts), gather_density(1) and (8, 2), set_cells of
  5 cells alive then dead with one coordinate outside [0, nx).
* Column staging and corners, LOCAL transport, 34 = K + 2 generations (two
  exchanges): 130 x 66 over dims (2, 1) and (2, 2) -- 65-wide blocks, the bit
  encoding's straddling-pair path and the byte encoding's 32-cell path, with
  corner blocks under (2, 2); 6 x 6 over (2, 1), one-cell columns; 95 x 70 in
  one shard, the self-wrapped x-apron.  The outputs are read from the
  partitioned grids too: only there is a block's global origin non-zero.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KERNELS = ["bit", "byte"]
SINGLE = [(nx, ny) for nx in (1, 17, 65, 129, 200) for ny in (1, 3, 33)]
# shards, dims, nx, ny
STAGED = [(2, (2, 1), 130, 66), (4, (2, 2), 130, 66), (2, (2, 1), 6, 6), (1, (1, 1), 95, 70)]
GENS = 34


@functools.lru_cache(maxsize=None)
def _states(nx, ny, gens=0):
    """The oracle's fill (seed and density as the tests pass them to the device), another grid to upload, and
    the fill after `gens` generations (shared, read-only)."""
    import oracle as O

    g0 = O.fill_random(nx, ny, nx * 5 + ny, 0.4)
    up = O.fill_random(nx, ny, nx + 11 * ny, 0.6)
    out = (g0, up, O.life_run(g0, gens) if gens else g0)
    for g in out:
        g.setflags(write=False)
    return out


def _window(grid, x0, y0, w, h):
    rows = np.take(grid, np.arange(y0, y0 + h), axis=0, mode="wrap")
    return np.take(rows, np.arange(x0, x0 + w), axis=1, mode="wrap")


def _density(grid, fx, fy):
    ny, nx = grid.shape
    fx, fy = min(fx, nx), min(fy, ny)  # factors beyond the grid: one bin
    bh, bw = -(-ny // fy), -(-nx // fx)
    pad = np.zeros((bh * fy, bw * fx), np.uint32)
    pad[:ny, :nx] = grid
    return pad.reshape(bh, fy, bw, fx).sum(axis=(1, 3)).astype(np.uint32)


def _vtk_body(grid):
    """'0' / '1' then a newline per cell, x fastest (life_save_vtk)."""
    return np.stack([grid + ord("0"), np.full_like(grid, ord("\n"))], axis=-1).tobytes()


def _check_outputs(life, oracle, grid):
    ny, nx = grid.shape
    np.testing.assert_array_equal(life.gather(), grid)
    np.testing.assert_array_equal(life.gather_bits(), np.packbits(grid, axis=1, bitorder="little"))
    assert life.gather_vtk()[-2 * nx * ny:] == _vtk_body(grid)  # after the host-written header
    assert life.live_count() == int(grid.sum())
    assert life.checksum() == oracle.checksum(grid)
    np.testing.assert_array_equal(life.gather_rect(0, 0, nx, ny), grid)
    w, h = min(9, nx), min(5, ny)
    np.testing.assert_array_equal(life.gather_rect(-3, -2, w, h), _window(grid, -3, -2, w, h))
    np.testing.assert_array_equal(life.gather_density(1), grid.astype(np.uint32))
    np.testing.assert_array_equal(life.gather_density(8, 2), _density(grid, 8, 2))


def _check_set_cells(life, grid):
    ny, nx = grid.shape
    cells = np.array([(k * 7 % nx, k * 3 % ny) for k in range(5)], dtype=np.int64)
    cells[1, 0] += nx   # outside [0, nx): wraps
    cells[3, 1] -= 2 * ny
    want = grid.copy()
    for alive in (True, False):
        life.set_cells(cells, alive=alive)
        want[cells[:, 1] % ny, cells[:, 0] % nx] = 1 if alive else 0
        np.testing.assert_array_equal(life.gather(), want)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", SINGLE)
def test_single_shard(gpu, oracle, nx, ny, kernel):
    g0, up, _ = _states(nx, ny)
    with gpu.Life(nx, ny, kernel=kernel, small_grid=False) as life:
        life.fill_random(nx * 5 + ny, 0.4)
        _check_outputs(life, oracle, g0)
        life.upload(up)
        _check_outputs(life, oracle, up)
        _check_set_cells(life, up)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", STAGED)
def test_column_staging(gpu, oracle, shards, dims, nx, ny, kernel):
    g0, up, end = _states(nx, ny, GENS)
    with gpu.Life(nx, ny, shards=shards, kernel=kernel, dims=dims, small_grid=False,
                  transport=gpu.XPORT_LOCAL if shards > 1 else gpu.XPORT_AUTO) as life:
        life.fill_random(nx * 5 + ny, 0.4)
        np.testing.assert_array_equal(life.gather(), g0)
        life.step(GENS)
        _check_outputs(life, oracle, end)
        _check_set_cells(life, end)
        life.upload(up)  # import into blocks with a global origin
        np.testing.assert_array_equal(life.gather(), up)
