"""Sparse I/O on the device: clear, set_cells, gather_rect, gather_density.

The four calls let a user load a coordinate list into, and look at, a grid no
host buffer holds.  Expected values come from the CPU oracle (fill_random,
life_run: 3-life/life2d.c:104-130 restated) and plain numpy written here --
np.take(mode="wrap") for windows, zero-pad + reshape + sum for density --
never from the library's other calls, except where a test ties two paths
together (gather_rect of the whole grid == gather()).

Shapes: the smallest that straddle what the kernels index by -- the 64-cell
pair, the 128-cell unit, the 32-cell byte word, the x-apron, 1-wide blocks,
block edges at x % 8 != 0, and the K = 32 halo depth.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(ROOT, "mpi-and-open-mp_amd", "driver", "life_mi355x")
P46 = os.path.join(GOLDEN, "cfg", "p46gun.cfg")

SIZES = [(1, 1), (5, 1), (63, 64), (64, 63), (65, 65), (127, 5), (128, 128), (129, 130), (257, 300), (1000, 37)]
SMALL = [False, "lds", True]
# shards, dims, nx, ny
ONE_CELL = [(4, (0, 0), 65, 33), (6, (0, 0), 47, 29), (8, (4, 2), 4, 2), (8, (0, 0), 300, 130)]
TEMPORAL = [(4, (2, 2), 260, 260), (4, (1, 4), 96, 132), (2, (1, 2), 300, 70)]
PARTS = ONE_CELL + TEMPORAL
KERNELS = ["bit", "byte"]
LIFE_EINVAL = -1


@functools.lru_cache(maxsize=None)
def _states(nx, ny):
    """g0 and the oracle's generations of it the tests compare with (shared, read-only)."""
    import oracle as O

    g0 = O.fill_random(nx, ny, seed=nx * 7 + ny, density=0.3)
    out = {0: g0, 3: O.life_run(g0, 3), 7: O.life_run(g0, 7), 10: O.life_run(g0, 10)}
    out[40] = O.life_run(out[7], 33)
    for g in out.values():
        g.setflags(write=False)
    return out


def _single(gpu, nx, ny, kernel, small):
    return gpu.Life(nx, ny, kernel=kernel, small_grid=small)


def _parted(gpu, shards, dims, nx, ny, kernel):
    return gpu.Life(nx, ny, shards=shards, kernel=kernel, dims=dims, transport=gpu.XPORT_LOCAL)


def _cell_list(g0, seed=1):
    """The live cells of g0 as (x, y) rows: shuffled, the first 10 % repeated,
    a third shifted by whole periods (+nx, -ny, +3 nx) so they must wrap."""
    ny, nx = g0.shape
    ys, xs = np.nonzero(g0)
    cells = np.stack([xs, ys], axis=1).astype(np.int64)
    rng = np.random.default_rng(seed)
    rng.shuffle(cells)
    cells = np.concatenate([cells, cells[: (len(cells) + 9) // 10]])
    k = np.arange(len(cells))
    cells[k % 9 == 0, 0] += nx
    cells[k % 9 == 3, 1] -= ny
    cells[k % 9 == 6, 0] += 3 * nx
    return cells


def _window(grid, x0, y0, w, h):
    rows = np.take(grid, np.arange(y0, y0 + h), axis=0, mode="wrap")
    return np.take(rows, np.arange(x0, x0 + w), axis=1, mode="wrap")


def _density(grid, fx, fy):
    ny, nx = grid.shape
    bh, bw = -(-ny // fy), -(-nx // fx)
    pad = np.zeros((bh * fy, bw * fx), np.uint32)
    pad[:ny, :nx] = grid
    return pad.reshape(bh, fy, bw, fx).sum(axis=(1, 3)).astype(np.uint32)


def _seams(life):
    """A block edge in x and in y (a shard's origin; 0 = the periodic seam
    where the axis is not cut)."""
    n = life.world()["nlocal"]
    lays = [life.layout(i) for i in range(n)]
    return max(L.x0 for L in lays), max(L.y0 for L in lays)


# ------------------------------------------------------------ 1. set_cells == upload
def _check_set_cells(life, oracle, nx, ny, long_run):
    st = _states(nx, ny)
    life.fill_random(99, 0.5)  # something to clear
    life.clear()
    life.set_cells(_cell_list(st[0]))
    np.testing.assert_array_equal(life.gather(), st[0])
    life.step(7)
    np.testing.assert_array_equal(life.gather(), st[7])
    if long_run:  # 40 generations in total: beyond the K = 32 halo depth
        life.step(33)
        np.testing.assert_array_equal(life.gather(), st[40])


@pytest.mark.parametrize("small", SMALL, ids=["stream", "lds", "vgpr"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", SIZES)
def test_set_cells_equals_upload(gpu, oracle, nx, ny, kernel, small):
    with _single(gpu, nx, ny, kernel, small) as life:
        _check_set_cells(life, oracle, nx, ny, False)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", PARTS)
def test_set_cells_equals_upload_partitioned(gpu, oracle, shards, dims, nx, ny, kernel):
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        _check_set_cells(life, oracle, nx, ny, (shards, dims, nx, ny) in TEMPORAL)


def test_set_cells_edge_arguments(gpu, oracle):
    st = _states(65, 65)
    with gpu.Life(65, 65, kernel="bit") as life:
        life.upload(st[0])
        life.set_cells(np.zeros((0, 2), np.int64))  # n == 0: a no-op
        life.set_cells([[3, 4], [3, 4], [3 + 65, 4 - 130]], alive=False)  # duplicates, wrapped
        want = st[0].copy()
        want[4, 3] = 0
        np.testing.assert_array_equal(life.gather(), want)
        life.set_cells([(3, 4)])  # any (n, 2) sequence
        want[4, 3] = 1
        np.testing.assert_array_equal(life.gather(), want)


# ------------------------------------------------------------ 2. edit in mid-run
GLIDER = np.array([(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)], dtype=np.int64)


def _check_edit(life, oracle, nx, ny):
    """10 generations (bit tiles: one pass, the K-deep aprons part-used and,
    with the deep halo, advanced alongside), an edit across block seams, 10
    more.  Aprons not refilled after the edit still hold the cells from before
    it: the second run then differs from the oracle's."""
    st = _states(nx, ny)
    sx, sy = _seams(life)
    life.upload(st[0])
    life.step(10)
    born = np.concatenate([GLIDER + (sx - 1, ny // 3), GLIDER + (nx // 3, sy - 1)])  # across an x and a y seam
    by, bx = np.mgrid[-1:2, -1:2]
    dead = np.stack([bx.ravel() + (sx + nx // 2), by.ravel() + sy], axis=1)  # a 3x3 block on the y seam
    corner = np.stack([bx.ravel(), by.ravel()], axis=1)  # and one on the periodic corner (negative coordinates)
    life.set_cells(born)
    life.set_cells(np.concatenate([dead, corner]), alive=False)
    want = st[10].copy()
    want[born[:, 1] % ny, born[:, 0] % nx] = 1
    for c in (dead, corner):
        want[c[:, 1] % ny, c[:, 0] % nx] = 0
    np.testing.assert_array_equal(life.gather(), want)
    life.step(10)
    np.testing.assert_array_equal(life.gather(), oracle.life_run(want, 10))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", TEMPORAL)
def test_edit_with_part_used_aprons(gpu, oracle, shards, dims, nx, ny, kernel):
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        assert life.layout().generations_per_exchange == 32
        _check_edit(life, oracle, nx, ny)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("loop", [1, 2, 3], ids=["xy", "x", "y"])
def test_edit_with_part_used_aprons_loopback(gpu, oracle, loop, kernel):
    nx, ny = 256, 130
    with gpu.Life(nx, ny, kernel=kernel) as life:
        life.upload(_states(nx, ny)[0])
        life.configure(gpu.OPT_LOOPBACK, loop)
        _check_edit(life, oracle, nx, ny)


# ------------------------------------------------------------ 3. clear
def _check_clear(life, nx, ny):
    life.fill_random(5, 0.5)
    assert life.live_count() > 0 or nx * ny < 8
    life.clear()
    assert life.live_count() == 0
    zero = np.zeros((ny, nx), np.uint8)
    np.testing.assert_array_equal(life.gather(), zero)
    life.step(3)
    np.testing.assert_array_equal(life.gather(), zero)
    assert life.live_count() == 0


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", [(5, 1), (65, 65), (257, 300), (1000, 37)])
@pytest.mark.parametrize("poison", [False, True], ids=["zeroed", "poisoned"])
def test_clear(gpu, monkeypatch, nx, ny, kernel, poison):
    # LIFE_POISON is read at each create (tests/test_gpu_poison.py): every
    # buffer of this handle then starts as 0xA5 bytes
    if poison:
        monkeypatch.setenv("LIFE_POISON", "1")
    with gpu.Life(nx, ny, kernel=kernel, small_grid=False) as life:
        _check_clear(life, nx, ny)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", [ONE_CELL[0], TEMPORAL[0], TEMPORAL[2]])
def test_clear_partitioned_poisoned(gpu, monkeypatch, shards, dims, nx, ny, kernel):
    monkeypatch.setenv("LIFE_POISON", "1")
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        life.fill_random(5, 0.5)
        life.step(10)  # temporal bit shards: part-used aprons
        _check_clear(life, nx, ny)


# ------------------------------------------------------------ 4. gather_rect
def _check_rect(life, nx, ny, centre=None):
    st = _states(nx, ny)
    life.upload(st[0])
    life.step(3)
    want = st[3]
    whole = life.gather_rect(0, 0, nx, ny)
    np.testing.assert_array_equal(whole, want)
    np.testing.assert_array_equal(whole, life.gather())
    wins = [(nx - 3, ny - 2, min(7, nx), min(5, ny)), (-5, -70, min(9, nx), min(3, ny)), (0, 0, 1, 1),
            (3 * nx + 1, 0, nx, 1)]
    if centre is not None:  # a window centred on the meeting point of four blocks
        wins.append((centre[0] - 4, centre[1] - 3, min(9, nx), min(7, ny)))
    for x0, y0, w, h in wins:
        got = life.gather_rect(x0, y0, w, h)
        assert got.shape == (h, w) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, _window(want, x0, y0, w, h), err_msg=str((x0, y0, w, h)))
    out = np.full((min(5, ny), min(7, nx)), 0xEE, np.uint8)  # the caller's buffer
    assert life.gather_rect(nx - 3, ny - 2, out.shape[1], out.shape[0], out=out) is out
    np.testing.assert_array_equal(out, _window(want, nx - 3, ny - 2, out.shape[1], out.shape[0]))


@pytest.mark.parametrize("small", SMALL, ids=["stream", "lds", "vgpr"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", SIZES)
def test_gather_rect(gpu, oracle, nx, ny, kernel, small):
    with _single(gpu, nx, ny, kernel, small) as life:
        _check_rect(life, nx, ny)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", PARTS)
def test_gather_rect_partitioned(gpu, oracle, shards, dims, nx, ny, kernel):
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        _check_rect(life, nx, ny, centre=_seams(life))


# ------------------------------------------------------------ 5. gather_density
def _check_density(life, nx, ny):
    st = _states(nx, ny)
    life.upload(st[0])
    life.step(3)
    want = st[3]
    live = int(want.sum())
    assert life.live_count() == live
    for fx, fy in [(1, 1), (3, 5), (8, 8), (64, 64), (100, 7), (128, 1), (1, 128), (nx, ny), (nx + 5, ny + 9)]:
        got = life.gather_density(fx, fy)
        exp = _density(want, min(fx, nx), min(fy, ny))
        assert got.dtype == np.uint32 and got.shape == exp.shape, (fx, fy)
        np.testing.assert_array_equal(got, exp, err_msg=str((fx, fy)))
        assert int(got.sum(dtype=np.uint64)) == live
    np.testing.assert_array_equal(life.gather_density(1, 1), want)  # the grid itself
    assert life.gather_density(nx, ny).tolist() == [[live]]
    np.testing.assert_array_equal(life.gather_density(8), _density(want, min(8, nx), min(8, ny)))  # fy = fx


@pytest.mark.parametrize("small", SMALL, ids=["stream", "lds", "vgpr"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", SIZES)
def test_gather_density(gpu, oracle, nx, ny, kernel, small):
    with _single(gpu, nx, ny, kernel, small) as life:
        _check_density(life, nx, ny)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shards,dims,nx,ny", PARTS)
def test_gather_density_partitioned(gpu, oracle, shards, dims, nx, ny, kernel):
    with _parted(gpu, shards, dims, nx, ny, kernel) as life:
        _check_density(life, nx, ny)


@pytest.mark.parametrize("kernel", KERNELS)
def test_gather_density_wide_bins(gpu, oracle, kernel):
    """Bins wider than a wave's 64 units (bit: 8192 cells): the lanes of a
    wave share one bin and add up across the wave before the atomic; 9000 is
    no multiple of the unit, so some waves straddle a bin edge."""
    nx, ny = 20000, 70
    g0 = oracle.fill_random(nx, ny, seed=4, density=0.5)
    with gpu.Life(nx, ny, kernel=kernel) as life:
        life.upload(g0)
        for fx, fy in [(8192, 32), (9000, 70), (16384, 3), (2048, 64)]:
            np.testing.assert_array_equal(life.gather_density(fx, fy), _density(g0, fx, fy), err_msg=str((fx, fy)))


# ------------------------------------------------------------ 6. rank mode, world 1
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nx,ny", [(256, 130), (257, 131)])
def test_rank_mode_world1(gpu, oracle, nx, ny, kernel):
    """A one-rank RCCL communicator: the readers' ncclAllReduce combine runs."""
    with gpu.Life.for_rank(nx, ny, 0, 1, gpu.unique_id(), 0, kernel=kernel) as life:
        assert life.shard_info()["rccl_nranks"] == 1
        _check_set_cells(life, oracle, nx, ny, True)
        _check_rect(life, nx, ny)
        _check_density(life, nx, ny)


# ------------------------------------------------------------ 7. a pattern in a big universe
def test_gun_in_a_big_universe_without_a_host_grid(gpu, oracle):
    """p46gun's 50 cells (box x 50..98, y 50..63) placed across the x seam of
    an 8192 x 4096 universe.  After 46 generations nothing lives outside
    x 4..144, y 4..109 of the pattern's own frame, so a 500^2 torus is the
    infinite plane here and the oracle's run on it is the expected window."""
    nx, ny, ox, oy = 8192, 4096, 8192 - 70, 2000
    _, _, _, _, cells = gpu.load_cfg_cells(P46)
    assert len(cells) == 50
    small = np.zeros((500, 500), np.uint8)
    small[cells[:, 1], cells[:, 0]] = 1
    want = oracle.life_run(small, 46)
    assert want[:160, :200].sum() == want.sum()
    with gpu.Life(nx, ny, kernel="bit") as life:
        life.clear()
        life.set_cells(cells + (ox, oy))
        life.step(46)
        np.testing.assert_array_equal(life.gather_rect(ox, oy, 200, 160), want[:160, :200])
        assert life.live_count() == int(want.sum())
        dens = life.gather_density(512)
        assert dens.shape == (8, 16) and int(dens.sum()) == int(want.sum())
        touched = np.zeros_like(dens, dtype=bool)
        for by in {oy // 512, (oy + 159) // 512}:
            for bx in {ox // 512, ((ox + 199) % nx) // 512}:
                touched[by, bx] = True
        assert not dens[~touched].any()
        exp = np.zeros((ny // 512, nx // 512), np.uint32)  # the window's cells binned at their global place
        ys, xs = np.nonzero(want[:160, :200])
        np.add.at(exp, ((ys + oy) % ny // 512, (xs + ox) % nx // 512), 1)
        np.testing.assert_array_equal(dens, exp)


# ------------------------------------------------------------ 8. driver
def _run_driver(cwd, *args):
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([DRIVER, *args], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return {f: open(os.path.join(cwd, "vtk", f), "rb").read() for f in sorted(os.listdir(os.path.join(cwd, "vtk")))}


def test_driver_sparse_writes_the_same_frames(gpu, tmp_path):
    args = [P46, "--steps", "20", "--save-steps", "5"]
    dense = _run_driver(str(tmp_path / "dense"), *args)
    sparse = _run_driver(str(tmp_path / "sparse"), *args, "--sparse")
    assert sorted(dense) == [f"life_{g:06d}.vtk" for g in (0, 5, 10, 15)]
    assert sparse == dense
    assert b"1\n" in dense["life_000015.vtk"][200:]


@pytest.mark.parametrize("steps,save", [(46, 46), (47, 23)])
def test_driver_density_frames(gpu, oracle, tmp_path, steps, save):
    nx, ny, fx, fy = 2048, 1024, 64, 32
    frames = _run_driver(str(tmp_path), P46, "--sparse", "--nx", str(nx), "--ny", str(ny), "--steps", str(steps),
                         "--save-steps", str(save), "--format", f"density:{fx}x{fy}")
    gens = list(range(0, steps, save))
    assert sorted(frames) == [f"life_{g:06d}.dens" for g in gens]
    _, _, _, _, cells = gpu.load_cfg_cells(P46)
    grid = np.zeros((ny, nx), np.uint8)
    grid[cells[:, 1], cells[:, 0]] = 1
    done = 0
    for g in gens:
        grid = oracle.life_run(grid, g - done, threads=4)
        done = g
        gen, nx2, ny2, fx2, fy2, counts = gpu.load_density(str(tmp_path / "vtk" / f"life_{g:06d}.dens"))
        assert (gen, nx2, ny2, fx2, fy2) == (g, nx, ny, fx, fy)
        np.testing.assert_array_equal(counts, _density(grid, fx, fy))
        assert counts.sum() > 0


# ------------------------------------------------------------ 9. errors
@pytest.mark.parametrize("kernel", KERNELS)
def test_bad_arguments_leave_the_handle_usable(gpu, oracle, kernel):
    nx, ny = 129, 130
    st = _states(nx, ny)
    with gpu.Life(nx, ny, kernel=kernel) as life:
        life.upload(st[0])
        for call in (lambda: life.gather_rect(0, 0, nx + 1, 1), lambda: life.gather_rect(0, 0, 1, 0),
                     lambda: life.gather_rect(0, 0, 1, ny + 1), lambda: life.gather_density(0, 1),
                     lambda: life.gather_density(1, 0), lambda: life.gather_density(2**16, 2**16),
                     lambda: life.gather_density(2**31, 2)):
            with pytest.raises(gpu.LifeError) as e:
                call()
            assert e.value.rc == LIFE_EINVAL
        for bad in (np.zeros((4, 3), np.int64), np.zeros(6, np.int64), np.zeros((2, 2, 2), np.int64)):
            with pytest.raises(ValueError):
                life.set_cells(bad)
        life.step(7)
        np.testing.assert_array_equal(life.gather(), st[7])
