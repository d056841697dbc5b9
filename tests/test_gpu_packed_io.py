"""The compact ways INTO a device: upload_bits (packed LIFEBITS rows, the
inverse of gather_bits) and set_rect (a periodic window, the inverse of
gather_rect).

Expected values come from the CPU oracle (fill_random, life_run:
3-life/life2d.c:104-130 restated) and plain numpy written here --
np.packbits(..., bitorder="little") for frames, index arrays taken modulo the
grid for wrapped windows -- never from the library's other calls, except where
a test ties two paths together on purpose (gather_bits after upload_bits; the
readers test_gpu_beyond_4g.py pins to the oracle at its shape).

Shapes: the lists of test_gpu_sparse_io.py -- the smallest that straddle the
64-cell pair, the 128-cell unit, the 16-cell byte unit, the x-apron, 1-wide
blocks, block edges at x % 8 != 0 (47 / 3, 300 / 4) and the K = 32 halo depth
-- and one byte grid whose padded buffer crosses 4 GiB.

test_part_used_aprons_* fail on a build whose calls skip the halo refill
(exchange) after the edit: confirmed once by hand on such a build.
"""
import ctypes
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(ROOT, "mpi-and-open-mp_amd", "driver", "life_mi355x")
GLIDER = os.path.join(GOLDEN, "cfg", "glider_10x10.cfg")

SIZES = [(1, 1), (5, 1), (63, 64), (64, 63), (65, 65), (127, 5), (128, 128), (129, 130), (257, 300), (1000, 37)]
SMALL = [False, "lds", True]
# shards, dims, nx, ny
ONE_CELL = [(4, (0, 0), 65, 33), (6, (0, 0), 47, 29), (8, (4, 2), 4, 2), (8, (0, 0), 300, 130)]
TEMPORAL = [(4, (2, 2), 260, 260), (4, (1, 4), 96, 132), (2, (1, 2), 300, 70)]
PARTS = ONE_CELL + TEMPORAL
KERNELS = ["bit", "byte"]
LIFE_EINVAL = -1
DENSITY = 0.3


def _seed(nx, ny):
    return nx * 7 + ny


@functools.lru_cache(maxsize=None)
def _states(nx, ny):
    """g0 (== the device's fill_random(_seed, DENSITY)) and the oracle's
    generations of it the tests compare with (shared, read-only)."""
    import oracle as O

    g0 = O.fill_random(nx, ny, seed=_seed(nx, ny), density=DENSITY)
    out = {0: g0, 7: O.life_run(g0, 7), 10: O.life_run(g0, 10)}
    out[40] = O.life_run(out[7], 33)
    for g in out.values():
        g.setflags(write=False)
    return out


def _pack(grid, dirty=False):
    """LIFEBITS rows of a grid; dirty: the pad bits of each row's last byte
    (at and beyond nx) all 1, which the device must ignore."""
    nx = grid.shape[1]
    p = np.packbits(grid.astype(bool), axis=1, bitorder="little")
    if dirty and nx % 8:
        p[:, -1] |= (0xFF << (nx % 8)) & 0xFF
    return p


def _single(gpu, nx, ny, kernel, small):
    return gpu.Life(nx, ny, kernel=kernel, small_grid=small)


def _parted(gpu, shards, dims, nx, ny, kernel):
    return gpu.Life(nx, ny, shards=shards, kernel=kernel, dims=dims, transport=gpu.XPORT_LOCAL)


def _seams(life):
    """A block edge in x and in y (a shard's origin; 0 = the periodic seam
    where the axis is not cut)."""
    n = life.world()["nlocal"]
    lays = [life.layout(i) for i in range(n)]
    return max(L.x0 for L in lays), max(L.y0 for L in lays)


def _paste(grid, x0, y0, cells):
    """numpy's set_rect: grid[(y0 + j) % ny, (x0 + i) % nx] = cells[j, i] != 0."""
    ny, nx = grid.shape
    h, w = cells.shape
    grid[np.ix_((y0 + np.arange(h)) % ny, (x0 + np.arange(w)) % nx)] = np.asarray(cells) != 0


# ------------------------------------------------------------ 1. upload_bits == upload
def _check_upload_bits(life, nx, ny, long_run, prefill=True):
    st = _states(nx, ny)
    if prefill:
        life.fill_random(99, 0.5)  # something to overwrite
    life.upload_bits(_pack(st[0], dirty=True))
    np.testing.assert_array_equal(life.gather(), st[0])
    assert life.live_count() == int(st[0].sum())
    life.step(7)
    np.testing.assert_array_equal(life.gather(), st[7])
    if long_run:  # 40 generations in total: beyond the K = 32 halo depth
        life.step(33)
        np.testing.assert_array_equal(life.gather(), st[40])


@pytest.mark.parametrize("small", SMALL, ids=["stream", "lds", "vgpr"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", SIZES)
def test_upload_bits_equals_upload(gpu, oracle, nx, ny, kernel, small):
    with _single(gpu, nx, ny, kernel, small) as life:
        _check_upload_bits(life, nx, ny, False)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", PARTS)
def test_upload_bits_equals_upload_partitioned(gpu, oracle, shards, dims, nx, ny, kernel):
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        _check_upload_bits(life, nx, ny, (shards, dims, nx, ny) in TEMPORAL)


# ------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", PARTS)
def test_gather_bits_returns_what_upload_bits_took(gpu, oracle, shards, dims, nx, ny, kernel):
    g0 = _states(nx, ny)[0]
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        life.upload_bits(_pack(g0, dirty=True))
        got = life.gather_bits()
        assert got.tobytes() == _pack(g0).tobytes()  # byte for byte, the pad bits clean


# ------------------------------------------------------------ 3. part-used aprons
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", TEMPORAL)
def test_part_used_aprons_upload_bits(gpu, oracle, shards, dims, nx, ny, kernel):
    """10 generations leave the K-deep aprons part-used (and, with the deep
    halo, advanced alongside); aprons not refilled after the upload still hold
    cells of the old run, and the next 7 generations differ from the oracle's."""
    st = _states(nx, ny)
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        assert life.layout().generations_per_exchange == 32
        life.fill_random(99, 0.5)
        life.step(10)
        life.upload_bits(_pack(st[0], dirty=True))
        life.step(7)
        np.testing.assert_array_equal(life.gather(), st[7])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", TEMPORAL)
def test_part_used_aprons_set_rect(gpu, oracle, shards, dims, nx, ny, kernel):
    st = _states(nx, ny)
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        sx, sy = _seams(life)
        life.fill_random(_seed(nx, ny), DENSITY)
        life.step(10)
        cells = (np.random.default_rng(5).random((41, 43)) < 0.5).astype(np.uint8)
        life.set_rect(sx - 21, sy - 19, cells)  # across the meeting point of the blocks
        want = st[10].copy()
        _paste(want, sx - 21, sy - 19, cells)
        np.testing.assert_array_equal(life.gather(), want)
        life.step(7)
        np.testing.assert_array_equal(life.gather(), oracle.life_run(want, 7))


# ------------------------------------------------------------ 4. set_rect
def _windows(nx, ny, sx, sy):
    """(x0, y0, w, h): the whole grid; across the periodic corner; across the
    block seam at odd offsets; one cell; a full-width row at x0 = 37 (its two
    pieces share a 64-cell pair); x0 = 61, w = 7 (a pair edge inside, both ends
    mid-byte) where the grid is wide enough."""
    wins = [(0, 0, nx, ny), (-3, -2, min(9, nx), min(7, ny)), (sx - 5, sy - 3, min(11, nx), min(9, ny)),
            (nx // 2, ny // 2, 1, 1), (37, ny // 3, nx, 1)]
    if nx >= 68:
        wins.append((61, 5 % ny, 7, min(3, ny)))
    return wins


def _check_set_rect(life, oracle, nx, ny, upload=True):
    g0 = _states(nx, ny)[0]
    if upload:
        life.upload(g0)
    want = g0.copy()
    sx, sy = _seams(life)
    rng = np.random.default_rng(nx * 1000 + ny)
    for k, (x0, y0, w, h) in enumerate(_windows(nx, ny, sx, sy)):
        cells = (rng.random((h, w)) < 0.5).astype(np.uint8)
        if k == 1:  # any nonzero byte is alive
            cells = cells * rng.choice(np.array([2, 255], np.uint8), size=cells.shape)
        elif k == 3:
            cells = cells.astype(bool)
        elif k == 4:  # wider than a byte: 256 must not be cut to 0
            cells = cells.astype(np.int64) * 256
        life.set_rect(x0, y0, cells)
        _paste(want, x0, y0, cells)
    np.testing.assert_array_equal(life.gather(), want)  # the pasted cells, and every other cell untouched
    life.step(7)
    np.testing.assert_array_equal(life.gather(), oracle.life_run(want, 7))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", [(65, 65), (129, 130), (257, 300)])
def test_set_rect(gpu, oracle, nx, ny, kernel):
    with gpu.Life(nx, ny, kernel=kernel) as life:
        _check_set_rect(life, oracle, nx, ny)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", PARTS)
def test_set_rect_partitioned(gpu, oracle, shards, dims, nx, ny, kernel):
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        _check_set_rect(life, oracle, nx, ny)


# ------------------------------------------------------------ 5. arguments
@pytest.mark.parametrize("kernel", KERNELS)
def test_bad_arguments_leave_the_handle_usable(gpu, oracle, kernel):
    nx, ny = 129, 130
    st = _states(nx, ny)
    lib = gpu._lib()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    with gpu.Life(nx, ny, kernel=kernel) as life:
        life.upload(st[0])
        one = np.ones((1, 1), np.uint8)
        packed = _pack(st[0])
        calls = [lambda: life.set_rect(0, 0, np.zeros((1, 0), np.uint8)),  # w < 1
                 lambda: life.set_rect(0, 0, np.zeros((1, nx + 1), np.uint8)),
                 lambda: life.set_rect(0, 0, np.zeros((ny + 1, 1), np.uint8)),
                 lambda: gpu._check(lib.life_dev_set_rect(life._h, 0, 0, 1, 1, None), "set_rect"),
                 lambda: gpu._check(lib.life_dev_set_rect(None, 0, 0, 1, 1, one.ctypes.data_as(u8)), "set_rect"),
                 lambda: gpu._check(lib.life_dev_upload_bits(life._h, None), "upload_bits"),
                 lambda: gpu._check(lib.life_dev_upload_bits(None, packed.ctypes.data_as(u8)), "upload_bits")]
        for call in calls:
            with pytest.raises(gpu.LifeError) as e:
                call()
            assert e.value.rc == LIFE_EINVAL
        rb = (nx + 7) // 8
        for bad in (np.zeros((ny, rb + 1), np.uint8), np.zeros((ny, rb - 1), np.uint8), np.zeros(ny * rb, np.uint8),
                    np.zeros((rb, ny), np.uint8), np.zeros((ny, rb), np.int8), np.zeros((ny, rb), np.uint16),
                    np.zeros((ny, nx), bool)):
            with pytest.raises(ValueError):
                life.upload_bits(bad)
        for bad in (np.zeros(4, np.uint8), np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2), np.float32)):
            with pytest.raises(ValueError):
                life.set_rect(0, 0, bad)
        np.testing.assert_array_equal(life.gather(), st[0])  # nothing was written
        # whole periods added to the origin change nothing
        cells = (np.random.default_rng(3).random((9, 70)) < 0.5).astype(np.uint8)
        want = st[0].copy()
        _paste(want, 100, 125, cells)
        life.set_rect(100 + 3 * nx, 125 - ny, cells)
        np.testing.assert_array_equal(life.gather(), want)
        life.upload(st[0])
        life.set_rect(100, 125, cells)
        np.testing.assert_array_equal(life.gather(), want)
        life.upload_bits(packed)
        life.step(7)
        np.testing.assert_array_equal(life.gather(), st[7])


# ------------------------------------------------------------ 6. rank mode and loopback
def _check_both_then_40(life, oracle, nx, ny):
    st = _states(nx, ny)
    life.fill_random(99, 0.5)
    life.upload_bits(_pack(st[0], dirty=True))
    life.step(40)
    np.testing.assert_array_equal(life.gather(), st[40])
    cells = (np.random.default_rng(8).random((45, 70)) < 0.5).astype(np.uint8)
    life.set_rect(-33, -20, cells)  # across the periodic corner: both loop-backed seams
    want = st[40].copy()
    _paste(want, -33, -20, cells)
    np.testing.assert_array_equal(life.gather(), want)
    life.step(40)
    np.testing.assert_array_equal(life.gather(), oracle.life_run(want, 40))


@pytest.mark.parametrize("kernel", KERNELS)
def test_rank_mode_world1(gpu, oracle, kernel):
    """A one-rank RCCL communicator (world > 1 has never executed)."""
    with gpu.Life.for_rank(260, 260, 0, 1, gpu.unique_id(), 0, kernel=kernel) as life:
        assert life.shard_info()["rccl_nranks"] == 1
        _check_both_then_40(life, oracle, 260, 260)


@pytest.mark.parametrize("kernel", KERNELS)
def test_loopback(gpu, oracle, kernel):
    """The one shard as a periodic partition of itself: both axes' aprons come
    from the halo exchange the calls must redo."""
    with gpu.Life(260, 260, kernel=kernel) as life:
        life.fill_random(1, 0.5)
        life.configure(gpu.OPT_LOOPBACK, 1)
        _check_both_then_40(life, oracle, 260, 260)


# ------------------------------------------------------------ 7. poisoned buffers
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", [(1, (0, 0), 129, 130), ONE_CELL[3]])
def test_poisoned_buffers(gpu, oracle, monkeypatch, shards, dims, nx, ny, kernel):
    """LIFE_POISON is read at each create: every buffer of the handle starts
    as 0xA5 bytes.  upload_bits is the first call on it, so it must define
    every owned cell; set_rect then edits an uploaded grid."""
    monkeypatch.setenv("LIFE_POISON", "1")
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        _check_upload_bits(life, nx, ny, False, prefill=False)
        _check_set_rect(life, oracle, nx, ny)


# ------------------------------------------------------------ 8. past 4 GiB
PATCH_W, PATCH_H = 640, 400


def _patch_into(packed, nx, ny, ox, oy, cells):
    """The patch into the packed image at its wrapped place, through the
    dense form of the rows it touches only."""
    ys = (oy + np.arange(PATCH_H)) % ny
    xs = (ox + np.arange(PATCH_W)) % nx
    band = np.unpackbits(packed[ys], axis=1, bitorder="little")[:, :nx]
    band[:, xs] = cells
    packed[ys] = np.packbits(band, axis=1, bitorder="little")


def _with_margin(cells, m=2):
    out = np.zeros((cells.shape[0] + 2 * m, cells.shape[1] + 2 * m), np.uint8)
    out[m:-m, m:-m] = cells
    return out


def test_beyond_4gib_buffer(gpu, oracle, monkeypatch):
    """Byte encoding 65536 x 66560: the smallest shape whose padded buffer
    crosses 4 GiB (test_gpu_beyond_4g.py S2, where gather_rect and the census
    are pinned to the oracle).  y4 is the first owned row at or beyond byte
    offset 2^32.  A packed SOURCE beyond 4 GiB needs 2^35 cells and is not
    tested."""
    nx, ny = 65536, 66560
    monkeypatch.setenv("LIFE_POISON", "1")
    with gpu.Life(nx, ny, kernel="byte") as life:
        L = life.layout()
        y4 = -(-2**32 // L.pitch) - L.yapron
        assert 600 < y4 < ny - 1060, (L.pitch, L.yapron, y4)
        origins = [(12345, y4 - PATCH_H // 2),            # across row y4
                   (-PATCH_W // 2, -PATCH_H // 2),        # the periodic corner: both seams
                   (40003, ny - PATCH_H)]                 # ends on the last row
        patches = [oracle.fill_random(PATCH_W, PATCH_H, seed=100 + k, density=0.5) for k in range(len(origins))]
        packed = np.zeros((ny, nx // 8), np.uint8)
        for (ox, oy), c in zip(origins, patches):
            _patch_into(packed, nx, ny, ox, oy, c)
        live = sum(int(c.sum()) for c in patches)
        life.upload_bits(packed)
        assert life.live_count() == live
        for (ox, oy), c in zip(origins, patches):
            got = life.gather_rect(ox - 2, oy - 2, PATCH_W + 4, PATCH_H + 4)
            np.testing.assert_array_equal(got, _with_margin(c), err_msg=str((ox, oy)))
        assert np.array_equal(life.gather_bits(), packed)
        fresh = oracle.fill_random(PATCH_W, PATCH_H, seed=200, density=0.5)
        ox, oy = 20001, y4 + PATCH_H // 2 + 51  # above y4, clear of the three patches
        life.set_rect(ox, oy, fresh)
        np.testing.assert_array_equal(life.gather_rect(ox - 2, oy - 2, PATCH_W + 4, PATCH_H + 4), _with_margin(fresh))
        assert life.live_count() == live + int(fresh.sum())


# ------------------------------------------------------------ 9. driver
def _driver(cwd, *args):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([DRIVER, *args], cwd=cwd, capture_output=True, text=True, timeout=120)


def _frames(cwd):
    return {f: open(os.path.join(cwd, "vtk", f), "rb").read() for f in sorted(os.listdir(os.path.join(cwd, "vtk")))}


@functools.lru_cache(maxsize=None)
def _glider40():
    """Generation 40 of glider_10x10, checked against the golden frame."""
    import life_mi355x as lm
    import oracle as O

    with open(os.path.join(GOLDEN, "golden.json")) as f:
        frames = json.load(f)["patterns"]["glider_10x10"]["frames"]
    g40 = O.life_run(lm.load_cfg(GLIDER)[2], 40)
    assert hashlib.md5(lm.vtk_bytes(g40)).hexdigest() == frames["40"][0]
    g40.setflags(write=False)
    return g40


def test_driver_resume_at(gpu, oracle, tmp_path):
    g40 = _glider40()
    dump = tmp_path / "glider40.bits"
    dump.write_bytes(gpu.bits_bytes(g40, 40))
    run = str(tmp_path / "run")
    r = _driver(run, "--resume", str(dump), "--nx", "300", "--ny", "70", "--at", "295,-3", "--steps", "60",
                "--save-steps", "10", "--format", "bits")
    assert r.returncode == 0, r.stdout + r.stderr
    want = np.zeros((70, 300), np.uint8)
    _paste(want, 295, -3, g40)
    assert int(want.sum()) == int(g40.sum()) == 5
    frames = _frames(run)
    assert sorted(frames) == ["life_000040.bits", "life_000050.bits"]  # numbered from the dump's generation
    for gen in (40, 50):
        assert frames[f"life_{gen:06d}.bits"] == gpu.bits_bytes(oracle.life_run(want, gen - 40), gen), gen


def test_driver_at_is_checked(gpu, tmp_path):
    dump = tmp_path / "glider40.bits"
    dump.write_bytes(gpu.bits_bytes(_glider40(), 40))
    r = _driver(str(tmp_path / "a"), GLIDER, "--at", "1,1")
    assert r.returncode == 1 and "--resume" in r.stderr
    r = _driver(str(tmp_path / "b"), "--at", "1,1")
    assert r.returncode == 1 and "--resume" in r.stderr
    r = _driver(str(tmp_path / "c"), "--resume", str(dump), "--nx", "9", "--ny", "70", "--at", "0,0")
    assert r.returncode == 1 and "does not fit" in r.stderr
    r = _driver(str(tmp_path / "d"), "--resume", str(dump), "--nx", "300", "--ny", "9", "--at", "0,0")
    assert r.returncode == 1 and "does not fit" in r.stderr
    r = _driver(str(tmp_path / "e"), "--resume", str(dump), "--at", "0,0")  # the universe's size is required
    assert r.returncode == 1 and "--nx" in r.stderr
    assert not any(os.path.exists(tmp_path / d / "vtk") for d in "abcde")


def test_driver_resume_ignores_pad_bits(gpu, oracle, tmp_path):
    """--resume goes through life_dev_upload_bits: a 13 x 9 dump whose pad
    bits (13..15 of every row) are all 1 resumes as the clean dump does."""
    grid = oracle.fill_random(13, 9, seed=4, density=0.4)
    clean, dirty = tmp_path / "clean.bits", tmp_path / "dirty.bits"
    clean.write_bytes(gpu.bits_bytes(grid, 3))
    head = b"LIFEBITS 1 13 9 3\n"
    dirty.write_bytes(head + _pack(grid, dirty=True).tobytes())
    assert clean.read_bytes() != dirty.read_bytes() and clean.read_bytes().startswith(head)
    out = {}
    for name, path in (("clean", clean), ("dirty", dirty)):
        r = _driver(str(tmp_path / name), "--resume", str(path), "--steps", "8", "--save-steps", "1", "--format", "bits")
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = _frames(str(tmp_path / name))
    assert sorted(out["clean"]) == [f"life_{g:06d}.bits" for g in range(3, 8)]
    assert out["dirty"] == out["clean"]
    for g in range(3, 8):
        assert out["clean"][f"life_{g:06d}.bits"] == gpu.bits_bytes(oracle.life_run(grid, g - 3), g)
