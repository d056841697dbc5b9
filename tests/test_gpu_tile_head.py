"""The bit tile's work outside the generation loop: the 32-bit item decode
(csrc/life_tile_decode.h) and the straight-line window load and store
(LIFE_TILE_STRAIGHT, tile_body_bit), bit-exact against the CPU oracle on the
per-launch tiles (small-grid kernels and the dataflow form off; last_path()
says "tiles").

4288 x 393: 67 pairs -- one plain tile column and a banded one of 5 pairs --
and three tile rows at m = 12, the last one cut (57 rows).  h < 65 x 192, so
the y wrap runs through the remainder path; the first tile row's window starts
above row 0 and the last one's runs past row 392, so waves of both cross the
seam inside their 24 rows (the per-row walk) next to waves that do not (the
straight walk); waves 0 and 7 hold ghost rows (r0 > 0, r1 < R) and the last
tile row's waves end beyond the stored rows, so the per-row store runs next to
the straight one.  Passes of 1, 7 and 12 generations, then a 13-generation
call (7 + 6).

8256 x 12600: 129 pairs -- two plain columns and a band -- and 75 tile rows;
h > 65 x 192: the one-step y wrap, and the straight load in every wave but a
few of the first and last tile rows.  13 generations as a pass of 12 and a
pass of 1 against the oracle; a 48-generation call as four pipelined passes of
four region launches each (the decode's region constants, tile rows from ty0 >
0) against the same call with the pipeline off.

Both shapes under both rule arms (LIFE_OPT_RULE7) and, in a child process
(the knob is read once per process), in dispatch order instead of the per-XCD
renumbering (LIFE_XCD_ORDER=0), every grid compared bit for bit.

The half-height tail needs a launch of more than one round of the 768
resident workgroups, and the planner's knobs at known values: two child
processes with LIFE_TAIL_SPLIT, LIFE_BANDS, LIFE_BAND_SPLIT and
LIFE_TIMING_MODE set, whatever this process runs under.  6016 x 84000
(test_gpu_band_split.py's shape): 782 items, the bottom tile rows at half
height.  3053440 x 100: one tile row of 769 plain columns and two banded
sub-columns, 771 items, which the planner re-tiles from its first tile row on
(F = ty0): the region keeps no row and every workgroup is a tail item.  Both
one pass of 12, pinned to the oracle on full-height windows, and the booked
work says which items ran.
Random 50 % fills: live cells in every row and pair.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_band_split as bs
from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL, BIG, SEED = (4288, 393), (8256, 12600), 11
SMALL_CALLS = [(1, 1), (7, 7), (12, 12), (12, 13)]  # (OPT_BLOCK_GENS, generations of the call)
BIG_CALLS = [(12, 12), (12, 1)]
ARMS = [pytest.param(1, id="rule7"), pytest.param(0, id="rule8")]  # RULE7_TILES / the 8-gate kernels


def run_calls(gpu, life, arm, calls):
    """[(generations so far, grid)] after each call."""
    life.configure(gpu.OPT_RULE7, arm)
    life.fill_random(SEED, 0.5)
    done, out = 0, []
    for bmax, gens in calls:
        life.configure(gpu.OPT_BLOCK_GENS, bmax)
        life.step(gens)
        done += gens
        assert life.last_path() == "tiles" and life.last_rule7() == arm
        out.append((done, life.gather(), life.live_count()))
    return out


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("shape,calls", [(SMALL, SMALL_CALLS), (BIG, BIG_CALLS)], ids=["4288x393", "8256x12600"])
def test_tiles_match_oracle(gpu, oracle, shape, calls, arm):
    assert bs.pass_sizes(13, 12) == [7, 6] and -(-393 // 168) == 3 and 393 - 2 * 168 == 57
    assert shape[1] > 65 * 192 or shape is SMALL
    with gpu.Life(*shape, kernel="bit", small_grid=False, flow=0) as life:
        life.configure(gpu.OPT_PIPELINE, 0)
        for done, got, live in run_calls(gpu, life, arm, calls):
            want = bs.reference(oracle, *shape, SEED, done)
            np.testing.assert_array_equal(got, want, err_msg=f"generation {done}")
            assert live == int(want.sum())


@pytest.mark.parametrize("arm", ARMS)
def test_pipelined_regions_match_whole_launches(gpu, arm):
    """48 generations: four passes of 12, each as four region launches, against whole launches."""
    got = {}
    for regions in (4, 0):
        with gpu.Life(*BIG, kernel="bit", small_grid=False, flow=0) as life:
            life.configure(gpu.OPT_PIPELINE, regions)
            life.configure(gpu.OPT_RULE7, arm)
            life.fill_random(SEED, 0.5)
            life.step(48)
            assert life.last_path() == "tiles" and life.last_rule7() == arm
            got[regions] = (life.checksum(), life.live_count(), life.gather())
    assert got[4][:2] == got[0][:2]
    np.testing.assert_array_equal(got[4][2], got[0][2])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {pkg!r})
import life_mi355x as lm
out = {{}}
for shape, calls in {cases!r}:
    for arm in (1, 0):
        with lm.Life(*shape, kernel="bit", small_grid=False, flow=0) as life:
            life.configure(lm.OPT_PIPELINE, 0)
            life.configure(lm.OPT_RULE7, arm)
            life.fill_random({seed}, 0.5)
            done = 0
            for bmax, gens in calls:
                life.configure(lm.OPT_BLOCK_GENS, bmax)
                life.step(gens)
                done += gens
                assert life.last_path() == "tiles" and life.last_rule7() == arm
                out["%dx%d_%d_%d" % (shape[0], shape[1], arm, done)] = np.packbits(life.gather(), axis=1)
np.savez({path!r}, **out)
"""


def test_dispatch_order_matches_oracle(gpu, oracle, tmp_path):
    """LIFE_XCD_ORDER=0: both shapes, both arms, every call, every cell against the oracle's grids (the
    cases of test_tiles_match_oracle: the references are shared; the child hands its grids over packed)."""
    cases = [(SMALL, SMALL_CALLS), (BIG, BIG_CALLS)]
    path = str(tmp_path / "grids.npz")
    script = _CHILD.format(pkg=os.path.join(ROOT, "mpi-and-open-mp_amd"), cases=cases, seed=SEED, path=path)
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, LIFE_XCD_ORDER="0"),
                         capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.load(path)
    n = 0
    for shape, calls in cases:
        for arm in (1, 0):
            done = 0
            for _bmax, gens in calls:
                done += gens
                want = np.packbits(bs.reference(oracle, *shape, SEED, done), axis=1)
                np.testing.assert_array_equal(got[f"{shape[0]}x{shape[1]}_{arm}_{done}"], want,
                                              err_msg=f"{shape} arm {arm} generation {done}")
                n += 1
    assert n == len(got.files) == 12


_TAIL_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {pkg!r})
import life_mi355x as lm
with lm.Life({nx}, {ny}, kernel="bit", small_grid=False, flow=0) as life:
    life.configure(lm.OPT_BLOCK_GENS, 12)
    life.configure(lm.OPT_PIPELINE, 0)
    life.fill_random(7, 0.5)
    life.set_timing(True)
    life.step(12)
    assert life.last_path() == "tiles"
    out = {{"w%d" % i: life.gather_rect(x0, 0, w, {ny}) for i, (x0, w) in enumerate({windows!r})}}
    _, n, _ = life.kernel_stats()
    out["work"] = np.float64(n * life.kernel_work()[1])
np.savez({path!r}, **out)
"""
TAIL_ENV = dict(LIFE_TAIL_SPLIT="2", LIFE_BANDS="1", LIFE_BAND_SPLIT="1", LIFE_TIMING_MODE="0", LIFE_XCD_ORDER="1")
MARGIN = 32  # the oracle's windows are cut: their edges are wrong by at most 12 cells after 12 generations


def run_tail(oracle, tmp_path, nx, ny, windows):
    """One pass of 12 generations in a child process under TAIL_ENV; the periodic windows (x0, w), all rows,
    against the oracle; the items the pass booked, in whole tiles."""
    path = str(tmp_path / "tail.npz")
    script = _TAIL_CHILD.format(pkg=os.path.join(ROOT, "mpi-and-open-mp_amd"), nx=nx, ny=ny, windows=windows,
                                path=path)
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **TAIL_ENV), capture_output=True,
                         text=True, timeout=100)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.load(path)
    for i, (x0, w) in enumerate(windows):
        ref = oracle.fill_random_window(nx, (x0 - MARGIN) % nx, 0, w + 2 * MARGIN, ny, seed=7, density=0.5)
        ref = oracle.life_run(ref, 12, threads=8)
        np.testing.assert_array_equal(got[f"w{i}"], ref[:, MARGIN:MARGIN + w], err_msg=f"window {i}")
    return float(got["work"]) / bs.lane_ops(1, 12)


def tail_items(plain, rows):
    """items of `rows` tile rows: `plain` ordinary columns and a last one as sub-columns of G = 32 and G = 4"""
    return plain * rows + -(-rows // 2) + -(-rows // 16)


def test_half_height_tail(oracle, gpu, tmp_path):
    """6016 x 84000: 500 tile rows, 782 items on 768 slots, so the bottom tile rows run as half-height tiles
    (decode kinds 3 and 4; 12-row waves whose ghost rows span a whole wave: the per-row store).  The window:
    both banded sub-columns (pairs 62..93), the plain tile column's pairs on either side of them and the
    wrap.  Booked: F full tile rows and the ceil((84000 - 168 F) / 72) half rows below them at half a tile
    each, not the 782 whole items."""
    nx, ny = 6016, 84000
    per_pass = run_tail(oracle, tmp_path, nx, ny, [(nx - 2048 - 64, 2048 + 64 + 192)])
    assert tail_items(1, 500) == 782 and per_pass != pytest.approx(782)
    splits = [tail_items(1, F) + 0.5 * tail_items(1, -(-(ny - 168 * F) // 72)) for F in range(500)]
    assert any(per_pass == pytest.approx(s) for s in splits), per_pass


def test_every_item_a_tail_item(oracle, gpu, tmp_path):
    """3053440 x 100: 47710 pairs = 769 plain tile columns and 32 pairs as two sub-columns, one tile row: 771
    items on 768 slots.  The planner re-tiles the launch from its first tile row on: two half-height tile
    rows (72 and 28 owned rows), 1540 items booked at half a tile each, and no full-height item at all --
    the region of the launch has no row left.  Windows: the last plain column, both sub-columns and the
    wrap; a tile column seam in the middle; the first columns."""
    nx, ny = 64 * (62 * 769 + 32), 100
    assert -(-ny // 168) == 1 and tail_items(769, 1) == 771 and -(-ny // 72) == 2
    windows = [(nx - 2048 - 256, 2048 + 256 + 192), (64 * 62 * 400 - 256, 512), (64 * 62 - 128, 256)]
    per_pass = run_tail(oracle, tmp_path, nx, ny, windows)
    assert per_pass == pytest.approx(0.5 * tail_items(769, 2)) and per_pass != pytest.approx(771)
