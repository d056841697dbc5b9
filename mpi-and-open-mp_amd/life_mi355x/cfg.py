"""Reference file formats: the .cfg pattern loader and the VTK frame writer.

* ``load_cfg`` restates the parsing half of life_init
  (6-cartesian/life_cart.c:92-111): ``steps``, ``save_steps``, ``nx ny``,
  then one live cell ``i j`` per line, coordinates wrapped periodically
  (x = i is the contiguous axis).  Malformed input raises instead of looping
  forever as the reference's fscanf loop does.
* ``save_vtk`` / ``vtk_bytes`` restate life_save_vtk (life_cart.c:159-187):
  ASCII STRUCTURED_POINTS, one ``%d\\n`` per cell, y outer, x inner.
* ``load_cfg_cells`` is the same parser without the grid: the coordinate list
  for ``Life.set_cells``; ``density_bytes`` / ``load_density`` are the
  driver's density-map frames; ``bits_bytes`` / ``load_bits`` /
  ``load_bits_packed`` its packed LIFEBITS frames (the last one without
  unpacking, for ``Life.upload_bits``).
"""
from __future__ import annotations

import os

import numpy as np


def _parse_cfg(path: str):
    """-> (steps, save_steps, nx, ny, cells[n, 2] int64 as written in the file)."""
    with open(path, "r") as f:
        toks = f.read().split()
    try:
        vals = [int(t) for t in toks]
    except ValueError as e:
        raise ValueError(f"{path}: non-integer token: {e}") from None
    if len(vals) < 4 or (len(vals) - 4) % 2:
        raise ValueError(f"{path}: expected 'steps save_steps nx ny' then 'i j' pairs")
    steps, save_steps, nx, ny = vals[:4]
    if nx <= 0 or ny <= 0:
        raise ValueError(f"{path}: bad grid size {nx}x{ny}")
    return steps, save_steps, nx, ny, np.asarray(vals[4:], dtype=np.int64).reshape(-1, 2)


def load_cfg(path: str):
    """-> (steps, save_steps, grid[ny, nx] uint8)."""
    steps, save_steps, nx, ny, c = _parse_cfg(path)
    grid = np.zeros((ny, nx), dtype=np.uint8)
    grid[np.mod(c[:, 1], ny), np.mod(c[:, 0], nx)] = 1  # u0[ind(i, j)] = 1
    return steps, save_steps, grid


def load_cfg_cells(path: str):
    """-> (steps, save_steps, nx, ny, cells[n, 2] int64): the live cells as
    (x, y) rows, wrapped into the grid, in the file's order and with its
    duplicates -- the list Life.set_cells takes; no grid is allocated."""
    steps, save_steps, nx, ny, c = _parse_cfg(path)
    return steps, save_steps, nx, ny, np.mod(c, np.asarray([nx, ny], dtype=np.int64))


def vtk_header(nx: int, ny: int) -> bytes:
    return ("# vtk DataFile Version 3.0\n"
            "Created by write_to_vtk2d\n"
            "ASCII\n"
            "DATASET STRUCTURED_POINTS\n"
            f"DIMENSIONS {nx + 1} {ny + 1} 1\n"
            "SPACING 1 1 0.0\n"
            "ORIGIN 0 0 0.0\n"
            f"CELL_DATA {nx * ny}\n"
            "SCALARS life int 1\n"
            "LOOKUP_TABLE life_table\n").encode()


def vtk_bytes(grid: np.ndarray) -> bytes:
    ny, nx = grid.shape
    body = np.empty((ny * nx, 2), dtype=np.uint8)
    body[:, 0] = np.where(grid.reshape(-1) != 0, ord("1"), ord("0"))
    body[:, 1] = ord("\n")
    return vtk_header(nx, ny) + body.tobytes()


def bits_bytes(grid: np.ndarray, generation: int = 0) -> bytes:
    """The driver's packed frame (--format bits): 'LIFEBITS 1 nx ny gen\\n'
    then rows of ceil(nx/8) bytes, cell x at bit x&7 of byte x>>3."""
    ny, nx = grid.shape
    rows = np.packbits(grid.astype(bool), axis=1, bitorder="little")
    return f"LIFEBITS 1 {nx} {ny} {generation}\n".encode() + rows.tobytes()


def load_bits_packed(path: str):
    """-> (generation, nx, ny, packed[ny, ceil(nx/8)] uint8) of a --format bits
    frame, still packed: what Life.upload_bits takes (no nx*ny grid)."""
    with open(path, "rb") as f:
        head = f.readline().split()
        if len(head) != 5 or head[0] != b"LIFEBITS" or head[1] != b"1":
            raise ValueError(f"{path}: not a LIFEBITS v1 frame")
        nx, ny, gen = int(head[2]), int(head[3]), int(head[4])
        raw = np.frombuffer(f.read(), dtype=np.uint8)
    rb = (nx + 7) // 8
    if raw.size != rb * ny:
        raise ValueError(f"{path}: truncated")
    return gen, nx, ny, raw.reshape(ny, rb)


def load_bits(path: str):
    """-> (generation, grid[ny, nx] uint8) of a --format bits frame."""
    gen, nx, _, packed = load_bits_packed(path)
    grid = np.unpackbits(packed, axis=1, bitorder="little")[:, :nx]
    return gen, np.ascontiguousarray(grid, dtype=np.uint8)


def density_bytes(counts: np.ndarray, nx: int, ny: int, fx: int, fy: int, generation: int = 0) -> bytes:
    """The driver's density frame (--format density:FX[xFY]):
    'LIFEDENS 1 nx ny fx fy gen\\n' then ceil(ny/fy) rows of ceil(nx/fx)
    little-endian uint32 live counts (Life.gather_density)."""
    c = np.asarray(counts)
    if c.shape != (-(-ny // fy), -(-nx // fx)):
        raise ValueError(f"density map shape {c.shape} != ({-(-ny // fy)}, {-(-nx // fx)})")
    return f"LIFEDENS 1 {nx} {ny} {fx} {fy} {generation}\n".encode() + c.astype("<u4").tobytes()


def load_density(path: str):
    """-> (generation, nx, ny, fx, fy, counts[ceil(ny/fy), ceil(nx/fx)] uint32)
    of a --format density frame."""
    with open(path, "rb") as f:
        head = f.readline().split()
        if len(head) != 7 or head[0] != b"LIFEDENS" or head[1] != b"1":
            raise ValueError(f"{path}: not a LIFEDENS v1 frame")
        nx, ny, fx, fy, gen = (int(t) for t in head[2:])
        if min(nx, ny, fx, fy) < 1:
            raise ValueError(f"{path}: bad LIFEDENS header")
        raw = f.read()
    bw, bh = -(-nx // fx), -(-ny // fy)
    if len(raw) != 4 * bw * bh:
        raise ValueError(f"{path}: truncated")
    return gen, nx, ny, fx, fy, np.frombuffer(raw, dtype="<u4").reshape(bh, bw).astype(np.uint32)


def save_vtk(path: str, grid: np.ndarray) -> None:
    """life_save_vtk: creates ./vtk if missing (life_cart.c:163-166)."""
    if os.path.basename(os.path.dirname(path)) == "vtk" and not os.path.isdir(os.path.dirname(path)):
        os.makedirs(os.path.dirname(path), mode=0o700, exist_ok=True)
    with open(path, "wb") as f:
        f.write(vtk_bytes(grid))
