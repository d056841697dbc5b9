"""Life-like rules on the bit path (life_dev_set_rule): the table-rule
instances of the per-launch tiles and of the one-generation kernel against
the numpy reference of tests/rule_ref.py (pinned to the oracle at B3/S23 by
tests/test_rule_host.py), every cell compared.

`small_grid` and `flow` stay at their defaults throughout: while a rule other
than B3/S23 is set the device must pass the small-grid and dataflow kernels
by, and last_path() says what ran."""
import os
import subprocess

import numpy as np
import pytest

import rule_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(ROOT, "mpi-and-open-mp_amd", "driver", "life_mi355x")
LIFE_EINVAL = -1
HIGHLIFE, DAYNIGHT = R.NAMED["B36/S23"], R.NAMED["B3678/S34678"]

TABLE_RULES = R.conway_flips() + [R.NAMED[k] for k in ("B36/S23", "B3678/S34678", "B2/S", "B1357/S1357",
                                                       "B3/S012345678")]
SOUP_SEED = 0  # 200 x 70 at density 0.5: every (alive, neighbours) pair occurs (checked below)
# Generation 1 of the soup holds every pair too, except under the two rules
# of the set that thin a 50 % soup out in one step: B/S23 (B3 flipped off:
# nothing is born, 19 % of the cells survive; a live cell with 8 live
# neighbours cannot exist after a step without births -- it would have had 8
# before and died) and Seeds (5 % alive).  No seed changes that; step(1) from
# the soup itself meets every table entry under every rule.
GEN1_ABSENT = {
    (0x00, 0x0C): {(0, 7), (0, 8), (1, 4), (1, 5), (1, 6), (1, 7), (1, 8)},
    (0x04, 0x00): {(0, 7), (0, 8), (1, 6), (1, 7), (1, 8)},
}

_refs = {}


def ref(nx, ny, seed, rule, gens):
    """Reference states after the cumulative generation counts `gens`
    (computed once per argument set; read-only)."""
    key = (nx, ny, seed, rule, tuple(gens))
    if key not in _refs:
        g, done, out = R.soup(nx, ny, seed), 0, []
        for n in gens:
            g = R.rule_run(g, n - done, rule)
            done = n
            g.setflags(write=False)
            out.append(g)
        _refs[key] = out
    return _refs[key]


def check_table(gpu, rule):
    """step(1) then step(12) under `rule` from the covering soup on 200 x 70
    (tiles) and from a soup on 31 x 13 (one-generation kernel)."""
    soup = R.soup(200, 70, SOUP_SEED)
    assert R.coverage(soup) == R.ALL_PAIRS
    gen1 = R.rule_step(soup, *rule)
    print("generation-1 pairs absent:", sorted(R.ALL_PAIRS - R.coverage(gen1)))
    assert R.ALL_PAIRS - R.coverage(gen1) == GEN1_ABSENT.get(rule, set())
    for nx, ny, path in ((200, 70, "tiles"), (31, 13, "onegen")):
        want = ref(nx, ny, SOUP_SEED, rule, (1, 13))
        with gpu.Life(nx, ny, kernel="bit", rule=rule) as life:
            assert life.rule == gpu.format_rule(*rule)
            life.upload(R.soup(nx, ny, SOUP_SEED))
            life.step(1)
            np.testing.assert_array_equal(life.gather(), want[0], err_msg=f"{nx}x{ny} generation 1")
            assert life.last_path() == path
            life.step(12)
            np.testing.assert_array_equal(life.gather(), want[1], err_msg=f"{nx}x{ny} generation 13")
            assert life.last_path() == path


@pytest.mark.parametrize("rule", TABLE_RULES, ids=lambda r: f"B{r[0]:03x}S{r[1]:03x}")
def test_table_coverage(gpu, rule):
    check_table(gpu, rule)


BIG = (4160, 1400)  # 65 pairs: one full tile column and a 3-pair banded one; 8 tile rows and a short ninth


def test_tile_geometry_under_a_rule(gpu):
    """Day & Night, 25 generations (passes of 9 + 8 + 8): full tiles, banded
    items, a short last tile row, the half-height tail."""
    want = ref(*BIG, 5, DAYNIGHT, (25,))[0]
    with gpu.Life(*BIG, kernel="bit", rule="B3678/S34678") as life:
        life.upload(R.soup(*BIG, 5))
        life.step(25)
        np.testing.assert_array_equal(life.gather(), want)
        assert life.last_path() == "tiles"


def test_pipelined_passes_under_a_rule(gpu):
    want = ref(*BIG, 5, HIGHLIFE, (48,))[0]
    with gpu.Life(*BIG, kernel="bit", rule=HIGHLIFE) as life:
        life.configure(gpu.OPT_PIPELINE, 4)
        life.upload(R.soup(*BIG, 5))
        life.step(48)
        np.testing.assert_array_equal(life.gather(), want)
        assert life.last_path() == "tiles"


SHARDED = [(4, (2, 2), 260, 260), (8, (1, 8), 64, 320)]


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("shards,dims,nx,ny", SHARDED)
def test_shards_and_deep_halo_under_a_rule(gpu, shards, dims, nx, ny, overlap):
    gens = (1, 4, 10, 45)
    want = ref(nx, ny, 9, HIGHLIFE, gens)
    with gpu.Life(nx, ny, shards=shards, dims=dims, kernel="bit", transport=gpu.XPORT_LOCAL, overlap=overlap,
                  rule="B36/S23") as life:
        life.upload(R.soup(nx, ny, 9))
        done = 0
        for n, w in zip(gens, want):
            life.step(n - done)
            done = n
            np.testing.assert_array_equal(life.gather(), w, err_msg=f"generation {n}")


def test_rule_switch(gpu, oracle):
    """B3/S23 -> HighLife -> B3/S23 between step calls of a 2 x 2 device;
    afterwards the device takes the paths of one that never had a rule."""
    grid = R.soup(260, 260, 9)
    a = oracle.life_run(grid, 10)
    b = R.rule_run(a, 10, HIGHLIFE)
    c = oracle.life_run(b, 10)
    with gpu.Life(260, 260, shards=4, dims=(2, 2), kernel="bit", transport=gpu.XPORT_LOCAL) as life:
        assert life.rule == "B3/S23"
        life.upload(grid)
        life.step(10)
        np.testing.assert_array_equal(life.gather(), a)
        life.set_rule("B36/S23")
        assert life.rule == "B36/S23"
        np.testing.assert_array_equal(life.gather(), a)  # the state is untouched
        life.step(10)
        np.testing.assert_array_equal(life.gather(), b)
        life.set_rule("B3/S23")
        life.step(10)
        np.testing.assert_array_equal(life.gather(), c)
    got = []
    for switched in (False, True):
        with gpu.Life(4096, 4096, kernel="bit") as life:
            life.fill_random(3, 0.5)
            if switched:
                life.set_rule(HIGHLIFE)
                life.step(12)
                assert life.last_path() == "tiles"
                life.fill_random(3, 0.5)
                life.set_rule(R.CONWAY)
            life.step(48)
            got.append((life.last_path(), life.checksum()))
    assert got[0] == got[1]


@pytest.mark.parametrize("kernel,rule", [("bit", "B03/S23"), ("bit", (0x008 | 1 << 9, 0x00C)),
                                         ("bit", (0x008, 0x00C | 1 << 9)), ("byte", "B36/S23")])
def test_refusals_leave_the_state(gpu, kernel, rule):
    grid = R.soup(200, 70, 4)
    with gpu.Life(200, 70, kernel=kernel, small_grid=False) as life:
        life.upload(grid)
        life.step(3)
        before = life.gather()
        with pytest.raises(gpu.LifeError) as e:
            life.set_rule(rule)
        assert e.value.rc == LIFE_EINVAL
        assert life.rule == "B3/S23"
        np.testing.assert_array_equal(life.gather(), before)
        life.set_rule("B3/S23")  # B3/S23 itself is fine on either encoding


def test_driver_rule(gpu, tmp_path):
    cfg = os.path.join(GOLDEN, "cfg", "glider_10x10.cfg")
    r = subprocess.run([DRIVER, cfg, "--rule", "B36/S23"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    steps, save, grid = gpu.load_cfg(cfg)
    last = (steps - 1) // save * save  # the last saved generation
    gpu.save_vtk(str(tmp_path / "want.vtk"), R.rule_run(grid, last, HIGHLIFE))
    assert (tmp_path / "vtk" / f"life_{last:06d}.vtk").read_bytes() == (tmp_path / "want.vtk").read_bytes()
    r = subprocess.run([DRIVER, cfg, "--rule", "nonsense"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "nonsense" in r.stderr
