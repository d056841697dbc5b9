"""life_batch on the GPU: many independent universes stepped in one launch,
every one of them compared with the CPU oracle."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import rule_ref as R

pytestmark = pytest.mark.gpu

WAVE_SHAPES = [(1, 1), (2, 3), (3, 2), (31, 5), (32, 32), (33, 7), (64, 64), (100, 37), (128, 64), (127, 63)]
GROUP_SHAPES = [(160, 96), (500, 500), (2048, 16),
                (129, 64), (128, 65)]  # the first shapes outside the wave tier's 128 x 64 (its last: above)
COUNTS = (1, 5, 67)  # 67: the last workgroup of 4 waves is partly filled
GENS = (0, 1, 2, 33)
LIFE_EINVAL = -1


def oracle_runs(oracle, grids, gens):
    """oracle.life_run of every universe (the C oracle releases the GIL: a few
    threads keep 67 universes of 500 x 500 within the second)."""
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        return np.stack(list(pool.map(lambda g: oracle.life_run(g, gens), grids)))


def soups(nx, ny, count, seed0, density=0.5):
    return np.stack([R.soup(nx, ny, seed0 + u, density) for u in range(count)])


def check_census(batch, oracle, want):
    np.testing.assert_array_equal(batch.live_counts(), want.reshape(len(want), -1).sum(axis=1))
    np.testing.assert_array_equal(batch.checksums(), np.array([oracle.checksum(g) for g in want], dtype=np.uint64))


@pytest.mark.parametrize("nx,ny", WAVE_SHAPES + GROUP_SHAPES)
def test_parity_with_the_oracle(gpu, oracle, nx, ny):
    lm = gpu
    start = soups(nx, ny, max(COUNTS), 100 * nx + ny)
    want, at = {0: start}, 0
    for g in GENS[1:]:  # each state from the one before
        want[g] = oracle_runs(oracle, want[at], g - at)
        at = g
    assert lm.batch_query(nx, ny)[0] == ("wave" if (nx, ny) in WAVE_SHAPES else "group")
    for count in COUNTS:
        with lm.LifeBatch(nx, ny, count) as b:
            for g in GENS:
                b.upload(start[:count])
                assert b.generation == 0
                b.step(g)
                assert b.generation == g
                np.testing.assert_array_equal(b.gather(), want[g][:count], err_msg=f"count {count} gens {g}")
                check_census(b, oracle, want[g][:count])
            b.upload(start[:count])
            b.step(20)
            b.step(13)
            np.testing.assert_array_equal(b.gather(), want[33][:count], err_msg=f"count {count} 20 + 13")
            check_census(b, oracle, want[33][:count])


def test_more_universes_than_resident_waves(gpu, oracle):
    """2051 universes: more than 256 CUs x 4 waves, and no multiple of 4."""
    count = 2051
    start = soups(32, 32, count, 5000)
    want = oracle_runs(oracle, start, 20)
    with gpu.LifeBatch(32, 32, count) as b:
        b.upload(start)
        b.step(20)
        np.testing.assert_array_equal(b.gather(), want)
        check_census(b, oracle, want)


@pytest.mark.parametrize("nx,ny", [(33, 7), (64, 64)])
def test_isolation_at_light_speed(gpu, nx, ny):
    """B1357/S1357 carries every cell's state one cell per generation in all
    directions: a wrap that read the neighbouring universe's words, or the
    padding bits of a 33-wide row, does not survive 70 generations of it."""
    start = soups(nx, ny, 9, 900 + nx)
    start[3] = start[5] = 0
    start[4] = 0
    start[4, 0, 0] = 1
    want = np.stack([R.parity_run(s, 70) for s in start])
    assert not want[3].any() and not want[5].any()
    with gpu.LifeBatch(nx, ny, 9, rule=R.PARITY) as b:
        b.upload(start)
        b.step(70)
        got = b.gather()
        for u in range(9):
            np.testing.assert_array_equal(got[u], want[u], err_msg=f"universe {u}")
        np.testing.assert_array_equal(b.live_counts(), want.reshape(9, -1).sum(axis=1))


RULES = [R.NAMED["B36/S23"], R.NAMED["B3678/S34678"], R.NAMED["B2/S"]] + R.conway_flips()
DENSITIES = (0.08, 0.2, 0.35, 0.5, 0.65, 0.8, 0.92, 0.97)  # sparse to crowded: every (alive, neighbours) pair


@pytest.mark.parametrize("nx,ny", [(33, 7), (64, 64)])
def test_rules(gpu, nx, ny):
    lm = gpu
    start = np.stack([R.soup(nx, ny, 40 + u, d) for u, d in enumerate(DENSITIES)])
    with lm.LifeBatch(nx, ny, len(start)) as b:
        for rule in RULES:
            seen, states = set(), start
            for _ in range(9):  # the states the rule is applied to
                for s in states:
                    seen |= R.coverage(s)
                states = np.stack([R.rule_step(s, *rule) for s in states])
            assert seen == R.ALL_PAIRS, (rule, sorted(R.ALL_PAIRS - seen))
            b.set_rule(rule)
            assert b.rule == lm.format_rule(*rule)
            b.upload(start)
            b.step(9)
            np.testing.assert_array_equal(b.gather(), states, err_msg=lm.format_rule(*rule))


def test_rule_refusals(gpu):
    lm = gpu
    with lm.LifeBatch(500, 500, 2) as b:
        with pytest.raises(lm.LifeError) as e:
            b.set_rule("B36/S23")
        assert e.value.rc == LIFE_EINVAL
        assert b.rule == "B3/S23"
        b.set_rule("B3/S23")
    with lm.LifeBatch(33, 7, 2) as b:
        with pytest.raises(lm.LifeError) as e:
            b.set_rule("B03/S23")
        assert e.value.rc == LIFE_EINVAL
        with pytest.raises(lm.LifeError):
            b.set_rule((1 << 9, 0))
        b.set_rule("23/36")
        assert b.rule == "B36/S23"


@pytest.mark.parametrize("nx,ny", [(33, 7), (500, 500)])
def test_fill_random(gpu, oracle, nx, ny):
    seed, density, count = 2**64 - 3, 0.37, 6  # seed + u wraps modulo 2^64
    with gpu.LifeBatch(nx, ny, count) as b:
        b.step(3)
        b.fill_random(seed, density)
        assert b.generation == 0
        want = np.stack([oracle.fill_random(nx, ny, (seed + u) % 2**64, density) for u in range(count)])
        np.testing.assert_array_equal(b.gather(), want)
        check_census(b, oracle, want)


@pytest.mark.parametrize("nx,ny", [(33, 7), (160, 96)])
def test_ranges(gpu, nx, ny):
    lm = gpu
    start = soups(nx, ny, 7, 300)
    patch = soups(nx, ny, 2, 400)
    with lm.LifeBatch(nx, ny, 7) as b:
        b.upload(start)
        b.step(2)
        b.upload(patch, first=3)
        assert b.generation == 2  # a partial upload does not restart the counter
        want = start.copy()
        want = np.stack([R.rule_run(s, 2, R.CONWAY) for s in want])
        want[3:5] = patch
        full = b.gather()
        np.testing.assert_array_equal(full, want)
        np.testing.assert_array_equal(b.gather(2, 3), full[2:5])
        np.testing.assert_array_equal(b.gather(6), full[6:])
        assert b.gather(7, 0).shape == (0, ny, nx)
        for first, n in ((-1, 1), (0, 8), (7, 1), (3, -1), (8, 0)):
            with pytest.raises(lm.LifeError) as e:
                b.gather(first, n)
            assert e.value.rc == LIFE_EINVAL, (first, n)
        with pytest.raises(lm.LifeError) as e:
            b.upload(patch, first=6)
        assert e.value.rc == LIFE_EINVAL
        np.testing.assert_array_equal(b.gather(), want)  # the refusals wrote nothing
        for bad in (-1, 2**31):
            with pytest.raises(lm.LifeError) as e:
                b.step(bad)
            assert e.value.rc == LIFE_EINVAL


# ---- settle detection
def settle_generation(oracle, grid, limit):
    """The first g >= 2 with S_g == S_(g-2), None when there is none up to `limit`."""
    older, old = grid, oracle.life_step(grid)
    for g in range(2, limit + 1):
        new = oracle.life_step(old)
        if np.array_equal(new, older):
            return g
        older, old = old, new
    return None


@pytest.fixture(scope="module")
def settle_soups(oracle):
    start = np.stack([R.soup(32, 32, 7000 + u, 0.35) for u in range(32)])
    when = [settle_generation(oracle, s, 512) for s in start]
    return start, when


def flags(when, n):
    return np.array([-1 if g is None or g > n else g for g in when], dtype=np.int64)


@pytest.mark.parametrize("n", [512, 511])
def test_settle_soups(gpu, oracle, settle_soups, n):
    start, when = settle_soups
    assert sum(g is not None for g in when) >= 8 and sum(g is None for g in when) >= 4, when
    with gpu.LifeBatch(32, 32, len(start), settle=True) as b:
        b.upload(start)
        b.step(n)
        np.testing.assert_array_equal(b.settled(), flags(when, n))
        want = np.stack([oracle.life_run(s, n) for s in start])
        np.testing.assert_array_equal(b.gather(), want)
        check_census(b, oracle, want)
        b.step(3)  # the flagged universes run 3 mod 2 generations, the others all 3
        np.testing.assert_array_equal(b.gather(), np.stack([oracle.life_run(s, 3) for s in want]))
        assert b.generation == n + 3
        assert (b.settled()[flags(when, n) >= 0] == flags(when, n)[flags(when, n) >= 0]).all()  # flags are kept


def test_settle_by_hand(gpu, oracle, settle_soups):
    start, when = settle_soups
    pick = next(u for u, g in enumerate(when) if g is not None)  # settles exactly at the call's last generation
    n = when[pick]
    grids = np.zeros((5, 32, 32), np.uint8)
    grids[1, 4:6, 4:6] = 1  # block
    grids[2, 10, 9:12] = 1  # blinker
    grids[3, 0, 1] = grids[3, 1, 2] = grids[3, 2, 0] = grids[3, 2, 1] = grids[3, 2, 2] = 1  # glider
    grids[4] = start[pick]
    with gpu.LifeBatch(32, 32, 5, settle=True) as b:
        b.upload(grids)
        b.step(n)
        np.testing.assert_array_equal(b.settled(), [2, 2, 2, -1, n])
        np.testing.assert_array_equal(b.gather(), np.stack([oracle.life_run(g, n) for g in grids]))
        # writing a universe resets its flag and no other; a new rule resets all
        b.upload(grids[3:4], first=1)
        np.testing.assert_array_equal(b.settled(), [2, -1, 2, -1, n])
        b.set_rule("B3/S23")
        np.testing.assert_array_equal(b.settled(), [-1] * 5)


def test_settle_changes_no_state(gpu):
    lm = gpu
    start = soups(33, 7, 9, 8100, 0.35)
    got = []
    for settle in (False, True):
        with lm.LifeBatch(33, 7, 9, settle=settle) as b:
            b.upload(start)
            b.step(301)
            b.step(40)
            got.append((b.gather(), b.live_counts(), b.checksums()))
            if not settle:
                np.testing.assert_array_equal(b.settled(), [-1] * 9)
    for off, on in zip(*got):
        np.testing.assert_array_equal(off, on)
    np.testing.assert_array_equal(got[0][0], np.stack([R.rule_run(s, 341, R.CONWAY) for s in start]))
    with lm.LifeBatch(500, 500, 1) as b:
        with pytest.raises(lm.LifeError) as e:
            b.configure(lm.BATCH_OPT_SETTLE, 1)
        assert e.value.rc == LIFE_EINVAL
    with lm.LifeBatch(33, 7, 1) as b:
        for option, value in ((lm.BATCH_OPT_SETTLE, 2), (2, 1), (0, 0)):
            with pytest.raises(lm.LifeError) as e:
                b.configure(option, value)
            assert e.value.rc == LIFE_EINVAL
