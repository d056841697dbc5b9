"""The group tier of life_batch on the GPU: every strip-height instance of
batch_group_kernel<R> (R in 1 2 3 4 5 6 8 10 12 16 20 25 32) and every
lane-group width (1..64 lanes per strip) against the CPU oracle, by the
protocol of test_gpu_batch.py::test_parity_with_the_oracle.

GROUP_CASES is the one list of shapes; each row states the instance it pins
(R, lanes per strip, strips) and the test asserts lm.batch_plan against it, so
a change of the plan cannot move a shape to another instance unnoticed.
tests/test_batch_plan_host.py holds the list to its coverage without a GPU."""
import ctypes

import numpy as np
import pytest

from test_gpu_batch import GENS, LIFE_EINVAL, check_census, oracle_runs, soups

pytestmark = pytest.mark.gpu

# (nx, ny, R, lanes per strip, strips)
# A. R = 1, 2, 3 at every width.  1 and 2 lanes: jl == jr, a word is its own left and right neighbour (1 lane)
# or has one word as both (2 lanes); (129,1) .. (1025,1): one strip, its own upper and lower neighbour through LDS
CASES_A = [
    (20, 65, 1, 1, 65), (32, 1026, 2, 1, 513), (1, 1029, 3, 1, 343),
    (33, 65, 1, 2, 65), (64, 514, 2, 2, 257), (50, 513, 3, 2, 171),
    (65, 65, 1, 4, 65), (128, 258, 2, 4, 129), (100, 261, 3, 4, 87),  # (65,65): 3 words on 4 lanes
    (129, 1, 1, 8, 1), (256, 130, 2, 8, 65), (255, 129, 3, 8, 43),
    (257, 1, 1, 16, 1), (512, 66, 2, 16, 33), (500, 69, 3, 16, 23),
    (513, 1, 1, 32, 1), (1024, 34, 2, 32, 17), (1000, 33, 3, 32, 11),
    (1025, 1, 1, 64, 1), (2048, 18, 2, 64, 9), (2047, 21, 3, 64, 7),
]
# B. the other ten strip heights, at 64 lanes (the fewest cells)
CASES_B = [
    (1025, 40, 4, 64, 10), (1500, 25, 5, 64, 5), (2047, 54, 6, 64, 9), (2048, 88, 8, 64, 11),
    (1100, 100, 10, 64, 10), (1025, 108, 12, 64, 9), (2000, 176, 16, 64, 11), (2047, 200, 20, 64, 10),
    (1056, 125, 25, 64, 5), (2048, 288, 32, 64, 9),
]
# C. full workgroups, and tall strips on narrow groups (several strips per wave)
CASES_C = [
    (32, 1024, 1, 1, 1024),  # all 1024 threads
    (2048, 512, 32, 64, 16),  # all 1024 threads, R > 1
    (255, 675, 25, 8, 27),  # 216 threads: the last wave is part-filled
    (20, 16416, 32, 1, 513), (64, 4112, 16, 2, 257), (500, 680, 20, 16, 34), (100, 1325, 25, 4, 53),
    (300, 340, 10, 16, 34),  # 10 words on 16 lanes
    (1000, 204, 12, 32, 17),
]
GROUP_CASES = CASES_A + CASES_B + CASES_C
SMALL_CELLS = 50_000  # shapes under it also run 67 universes


def counts_of(nx, ny):
    return (1, 5, 67) if nx * ny < SMALL_CELLS else (1, 5)


def case_id(case):
    nx, ny, rows, lanes, _ = case
    return f"{nx}x{ny}-R{rows}-L{lanes}"


def assert_plan(lm, nx, ny, rows, lanes, strips):
    plan = lm.batch_plan(nx, ny)
    assert (plan.tier, plan.rows, plan.lanes_per_strip, plan.strips) == ("group", rows, lanes, strips), plan
    assert plan.words == -(-nx // 32) and plan.threads == 64 * -(-strips * lanes // 64), plan


@pytest.mark.parametrize("case", GROUP_CASES, ids=case_id)
def test_parity_with_the_oracle(gpu, oracle, case):
    lm = gpu
    nx, ny, rows, lanes, strips = case
    assert_plan(lm, nx, ny, rows, lanes, strips)
    counts = counts_of(nx, ny)
    start = soups(nx, ny, max(counts), 100 * nx + ny)
    want, at = {0: start}, 0
    for g in GENS[1:]:  # each state from the one before
        want[g] = oracle_runs(oracle, want[at], g - at)
        at = g
    for count in counts:
        with lm.LifeBatch(nx, ny, count) as b:
            assert b.tier == "group"
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


TALL = (2047, 21, 3, 64, 7)  # R > 1 and a part-filled last word


def test_fill_random_tall_strips(gpu, oracle):
    """test_gpu_batch.py::test_fill_random at a shape of three-row strips whose last word holds 31 cells."""
    nx, ny = TALL[:2]
    assert_plan(gpu, *TALL)
    seed, density, count = 2**64 - 3, 0.37, 6  # seed + u wraps modulo 2^64
    with gpu.LifeBatch(nx, ny, count) as b:
        b.step(3)
        b.fill_random(seed, density)
        assert b.generation == 0
        want = np.stack([oracle.fill_random(nx, ny, (seed + u) % 2**64, density) for u in range(count)])
        np.testing.assert_array_equal(b.gather(), want)
        check_census(b, oracle, want)


def test_ranges_tall_strips(gpu, oracle):
    """test_gpu_batch.py::test_ranges at the same shape: `first=` offsets of upload and gather."""
    lm = gpu
    nx, ny = TALL[:2]
    assert_plan(lm, *TALL)
    start = soups(nx, ny, 7, 300)
    patch = soups(nx, ny, 2, 400)
    with lm.LifeBatch(nx, ny, 7) as b:
        b.upload(start)
        b.step(2)
        b.upload(patch, first=3)
        assert b.generation == 2  # a partial upload does not restart the counter
        want = oracle_runs(oracle, start, 2)
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
        b.step(5)  # the patched universes step on with the others
        want = oracle_runs(oracle, want, 5)
        np.testing.assert_array_equal(b.gather(), want)
        check_census(b, oracle, want)


@pytest.mark.parametrize("nx,ny", [(129, 131), (2049, 16)])
def test_refused_shape_on_the_device(gpu, nx, ny):
    """A shape in neither tier: life_batch_create says what life_batch_query says and hands out no batch."""
    lm = gpu
    with pytest.raises(lm.LifeError) as e:
        lm.batch_query(nx, ny)
    assert e.value.rc == LIFE_EINVAL
    why = lm._lib().life_last_error().decode()
    assert f"batch of {nx} x {ny} universes" in why
    with lm.LifeBatch(33, 7, 1):  # the device is up, and the last message is no longer the query's
        with pytest.raises(lm.LifeError):
            lm.parse_rule("B9/S")
    assert lm._lib().life_last_error().decode() != why
    with pytest.raises(lm.LifeError) as e:
        lm.LifeBatch(nx, ny, 1)
    assert e.value.rc == LIFE_EINVAL
    assert lm._lib().life_last_error().decode() == why
    handle = ctypes.c_void_p(1)  # nothing allocated: the out pointer is cleared, there is nothing to destroy
    assert lm._lib().life_batch_create(nx, ny, 1, 0, ctypes.byref(handle)) == LIFE_EINVAL
    assert handle.value is None
    assert lm._lib().life_last_error().decode() == why
