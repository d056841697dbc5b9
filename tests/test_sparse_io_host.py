"""Host half of the sparse I/O: the .cfg coordinate-list loader and the
density-map frame format (cfg.py).  No GPU.

``load_cfg_cells`` must describe the same cells as ``load_cfg`` (which
restates life_init's parsing, 6-cartesian/life_cart.c:92-111) without ever
building the grid; ``density_bytes`` / ``load_density`` are the two ends of
the driver's ``--format density`` frames.
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN

CFGS = sorted(glob.glob(os.path.join(GOLDEN, "cfg", "*.cfg")))


def test_fixtures_present():
    assert len(CFGS) >= 6


@pytest.mark.parametrize("path", CFGS, ids=[os.path.basename(p) for p in CFGS])
def test_cells_scatter_to_the_grid_of_load_cfg(lm, path):
    steps, save_steps, grid = lm.load_cfg(path)
    s2, v2, nx, ny, cells = lm.load_cfg_cells(path)
    assert (s2, v2) == (steps, save_steps)
    assert (ny, nx) == grid.shape
    assert cells.dtype == np.int64 and cells.ndim == 2 and cells.shape[1] == 2
    assert cells.size == 0 or (cells.min() >= 0 and cells[:, 0].max() < nx and cells[:, 1].max() < ny)
    got = np.zeros((ny, nx), np.uint8)
    got[cells[:, 1], cells[:, 0]] = 1
    np.testing.assert_array_equal(got, grid)


def test_cells_keep_order_duplicates_and_wrap(lm, tmp_path):
    p = tmp_path / "w.cfg"
    p.write_text("3\n1\n5 4\n6 -1\n0 0\n6 -1\n-11 9\n4 3\n")
    steps, save_steps, nx, ny, cells = lm.load_cfg_cells(str(p))
    assert (steps, save_steps, nx, ny) == (3, 1, 5, 4)
    # true modulo: 6 -> 1, -1 -> 3, -11 -> 4, 9 -> 1; order and the duplicate kept
    np.testing.assert_array_equal(cells, [[1, 3], [0, 0], [1, 3], [4, 1], [4, 3]])
    _, _, grid = lm.load_cfg(str(p))
    got = np.zeros((ny, nx), np.uint8)
    got[cells[:, 1], cells[:, 0]] = 1
    np.testing.assert_array_equal(got, grid)


def test_header_only_file_has_no_cells(lm, tmp_path):
    p = tmp_path / "e.cfg"
    p.write_text("7\n2\n9 3\n")
    steps, save_steps, nx, ny, cells = lm.load_cfg_cells(str(p))
    assert (steps, save_steps, nx, ny) == (7, 2, 9, 3) and cells.shape == (0, 2)
    assert lm.load_cfg(str(p))[2].sum() == 0


@pytest.mark.parametrize("text", ["", "10\n1\n5\n", "10\n1\n5 5\n1\n", "10\n1\n5 5\n1 x\n", "10\n1\n0 5\n",
                                  "10\n1\n5 -5\n1 1\n", "10 1 5 5 1.5 2\n"],
                         ids=["empty", "short_header", "odd_tokens", "non_integer", "nx_zero", "ny_negative", "float"])
def test_malformed_input_raises_in_both_loaders(lm, tmp_path, text):
    p = tmp_path / "bad.cfg"
    p.write_text(text)
    with pytest.raises(ValueError):
        lm.load_cfg(str(p))
    with pytest.raises(ValueError):
        lm.load_cfg_cells(str(p))


def _density(grid, fx, fy):
    ny, nx = grid.shape
    bh, bw = -(-ny // fy), -(-nx // fx)
    pad = np.zeros((bh * fy, bw * fx), np.uint32)
    pad[:ny, :nx] = grid
    return pad.reshape(bh, fy, bw, fx).sum(axis=(1, 3)).astype(np.uint32)


@pytest.mark.parametrize("nx,ny,fx,fy", [(64, 32, 8, 8), (65, 33, 8, 4), (10, 7, 3, 5), (5, 1, 7, 9), (100, 37, 1, 1)])
def test_density_frame_round_trip(lm, tmp_path, nx, ny, fx, fy):
    rng = np.random.default_rng(nx * 1000 + ny)
    counts = _density((rng.random((ny, nx)) < 0.4).astype(np.uint8), fx, fy)
    raw = lm.density_bytes(counts, nx, ny, fx, fy, 46)
    head = f"LIFEDENS 1 {nx} {ny} {fx} {fy} 46\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + 4 * counts.size
    assert raw[len(head):] == counts.astype("<u4").tobytes()
    p = tmp_path / "f.dens"
    p.write_bytes(raw)
    gen, nx2, ny2, fx2, fy2, got = lm.load_density(str(p))
    assert (gen, nx2, ny2, fx2, fy2) == (46, nx, ny, fx, fy)
    assert got.dtype == np.uint32 and got.shape == (-(-ny // fy), -(-nx // fx))
    np.testing.assert_array_equal(got, counts)


def test_density_frame_errors(lm, tmp_path):
    counts = np.arange(6, dtype=np.uint32).reshape(2, 3)
    raw = lm.density_bytes(counts, 9, 8, 3, 4, 0)
    p = tmp_path / "t.dens"
    p.write_bytes(raw[:-1])  # truncated
    with pytest.raises(ValueError):
        lm.load_density(str(p))
    p.write_bytes(raw + b"\0")  # trailing bytes
    with pytest.raises(ValueError):
        lm.load_density(str(p))
    p.write_bytes(b"LIFEBITS 1 9 8 0\n" + raw)  # another frame format
    with pytest.raises(ValueError):
        lm.load_density(str(p))
    with pytest.raises(ValueError):  # a map of the wrong shape for the factors
        lm.density_bytes(counts, 9, 8, 2, 4, 0)  # 2 x 5 bins
