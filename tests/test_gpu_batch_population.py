"""Batch population traces on the GPU (LIFE_BATCH_OPT_POPULATION, DESIGN.md
§5.14): every universe's live count after every generation of a step call,
recorded by the kernels that hold the universes.  The wave tier is held to the
numpy rule reference (rule_ref.rule_step, summed per generation), the group
tier to the CPU oracle; states, census, settle flags and cycle pairs to the
same calls with the option off."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import rule_ref as R
from test_batch_survey_host import hand_patterns
from test_gpu_batch import soups
from test_gpu_batch_group import assert_plan

pytestmark = pytest.mark.gpu

LIFE_EINVAL = -1
FLUSH = 128  # kTraceFlush of csrc/life_batch_kernels.hip: a wave stores its pending totals every 128 generations
COUNTS = (1, 5, 67)
WAVE_SHAPES = [(1, 1), (31, 5), (33, 7), (64, 64), (65, 3), (97, 64), (128, 64)]
WAVE_GENS = sorted({1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 257, FLUSH - 1, FLUSH, FLUSH + 1, 2 * FLUSH + 1})
WAVE_RULES = ["B3/S23", "B36/S23", "B1357/S1357"]
FULL = (0, 0x1FF)  # B/S012345678: nothing is born, nothing dies
RULESET = [R.NAMED["B36/S23"], R.NAMED["B3678/S34678"], R.NAMED["B2/S"], R.NAMED["B1357/S1357"],
           R.NAMED["B3/S012345678"]] + R.conway_flips()  # the 22 rules of test_gpu_batch_survey.py


def rule_trace(start, gens, rules):
    """(count, gens) live counts after generations 1 .. gens, by rule_step; `rules` one rule or one per universe."""
    if isinstance(rules, tuple):
        rules = [rules] * len(start)
    out = np.zeros((len(start), gens), np.uint32)
    for u, (grid, rule) in enumerate(zip(start, rules)):
        for g in range(gens):
            grid = R.rule_step(grid, *rule)
            out[u, g] = grid.sum()
    return out


def oracle_trace(oracle, start, gens):
    """The same by the C oracle (B3/S23), a universe per thread."""
    def one(grid):
        row = np.zeros(gens, np.uint32)
        for g in range(gens):
            grid = oracle.life_step(grid)
            row[g] = grid.sum(dtype=np.int64)
        return row
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        return np.stack(list(pool.map(one, start)))


def assert_varied(want, cells):
    """From the reference alone: a constant answer cannot pass.  (Universes of fewer than three cells cannot take
    three values: a 1 x 1 universe is its own eight neighbours and is dead after one generation of these rules.)"""
    if cells >= 3:
        assert len(np.unique(want)) >= 3, np.unique(want)
    else:
        assert not want.any()


def same_as_off(on, off, n):
    """After the same calls: the states and the census of the recording batch are those of the plain one, and the
    trace's last column is the census."""
    trace = on.population()
    assert trace.dtype == np.uint32 and trace.shape == (on.count, n)
    np.testing.assert_array_equal(on.gather(), off.gather())
    live = on.live_counts()
    np.testing.assert_array_equal(live, off.live_counts())
    np.testing.assert_array_equal(on.checksums(), off.checksums())
    np.testing.assert_array_equal(trace[:, -1], live)
    assert on.generation == off.generation
    return trace


# ---- 1. wave tier: the trace against the rule reference
@pytest.mark.parametrize("rule", WAVE_RULES)
@pytest.mark.parametrize("nx,ny", WAVE_SHAPES)
def test_wave_tier_trace(gpu, nx, ny, rule):
    lm = gpu
    assert lm.batch_query(nx, ny)[0] == "wave"
    start = soups(nx, ny, max(COUNTS), 100 * nx + ny)
    want = rule_trace(start, max(WAVE_GENS), R.NAMED[rule])
    assert_varied(want, nx * ny)
    for count in COUNTS:
        with lm.LifeBatch(nx, ny, count, rule=rule, population=True) as on, \
                lm.LifeBatch(nx, ny, count, rule=rule) as off:
            for n in WAVE_GENS:
                for b in (on, off):
                    b.upload(start[:count])
                    b.step(n)
                trace = same_as_off(on, off, n)
                np.testing.assert_array_equal(trace, want[:count, :n], err_msg=f"count {count} gens {n}")
                assert off.population().shape == (count, 0)


# ---- 2. the largest values
def test_largest_values_wave_tier(gpu):
    nx, ny, n = 128, 64, 130
    grids = np.zeros((2, ny, nx), np.uint8)
    grids[0] = 1
    np.testing.assert_array_equal(rule_trace(grids, 3, FULL), [[8192] * 3, [0] * 3])  # the reference agrees
    for rules in (None, [FULL, FULL]):  # the uniform table rule, and a rule per universe
        with gpu.LifeBatch(nx, ny, 2, rule=FULL, rules=rules, population=True) as b:
            b.upload(grids)
            b.step(n)
            trace = b.population()
            assert trace.shape == (2, n)
            assert (trace[0] == 8192).all(), trace[0]  # a packed 13-bit field would have overflowed
            assert (trace[1] == 0).all(), trace[1]
            np.testing.assert_array_equal(b.gather(), grids)


def test_largest_values_group_tier(gpu, oracle):
    nx, ny, n = 2048, 512, 3
    assert_plan(gpu, nx, ny, 32, 64, 16)
    full = np.ones((1, ny, nx), np.uint8)
    soup = soups(nx, ny, 1, 77)
    want_full, want_soup = oracle_trace(oracle, full, n), oracle_trace(oracle, soup, n)
    assert want_full[0, 0] == 0  # B3/S23 kills a full torus at once
    assert want_soup.min() > 2**16 and len(np.unique(want_soup)) == 3
    with gpu.LifeBatch(nx, ny, 1, population=True) as b:
        for grids, want in ((full, want_full), (soup, want_soup)):
            b.upload(grids)
            b.step(n)
            np.testing.assert_array_equal(b.population(), want)
            np.testing.assert_array_equal(b.population()[:, -1], b.live_counts())


# ---- 3. a rule per universe
@pytest.mark.parametrize("nx,ny", [(33, 7), (128, 64)])
def test_a_rule_per_universe(gpu, nx, ny):
    lm = gpu
    assert len(RULESET) == 22
    count, n = 67, 129
    rules = [RULESET[u % len(RULESET)] for u in range(count)]
    start = soups(nx, ny, count, 40, 0.35)
    want = rule_trace(start, n, rules)
    assert_varied(want, nx * ny)
    with lm.LifeBatch(nx, ny, count, rules=rules, population=True) as on, \
            lm.LifeBatch(nx, ny, count, rules=rules) as off:
        for b in (on, off):
            b.upload(start)
            b.step(n)
        trace = same_as_off(on, off, n)
        for u in range(count):
            np.testing.assert_array_equal(trace[u], want[u], err_msg=f"universe {u} {lm.format_rule(*rules[u])}")


# ---- 4. detectors
@pytest.fixture(scope="module")
def detector_case():
    """The hand patterns and the 32 x 32 soups of the settle and cycle tests, and their trace over 300 + 41."""
    start = np.concatenate([hand_patterns(), np.stack([R.soup(32, 32, 7000 + u, 0.35) for u in range(32)])])
    want = rule_trace(start, 341, R.CONWAY)
    assert_varied(want, 32 * 32)
    return start, want


@pytest.mark.parametrize("detector", ["settle", "cycle"])
def test_detectors_leave_the_trace_complete(gpu, detector_case, detector):
    lm = gpu
    start, want = detector_case
    count = len(start)

    def flags(b):
        return b.settled() if detector == "settle" else np.stack(b.cycles())

    with lm.LifeBatch(32, 32, count, population=True, **{detector: True}) as on, \
            lm.LifeBatch(32, 32, count, **{detector: True}) as off, \
            lm.LifeBatch(32, 32, count, population=True) as plain:
        for b in (on, off, plain):
            b.upload(start)
        at = 0
        for call, n in enumerate((300, 41)):
            for b in (on, off, plain):
                b.step(n)
            trace = same_as_off(on, off, n)
            np.testing.assert_array_equal(trace, plain.population(), err_msg=f"call {call}")
            np.testing.assert_array_equal(trace, want[:, at:at + n], err_msg=f"call {call}")
            np.testing.assert_array_equal(flags(on), flags(off), err_msg=f"call {call}")
            np.testing.assert_array_equal(on.gather(), plain.gather())
            at += n
            if call == 0:  # the second call covers universes flagged in the first, and universes not yet flagged
                found = flags(off)[0] if detector == "cycle" else flags(off) + 1
                assert (found > 0).sum() >= 8 and (found <= 0).sum() >= 2, found


# ---- 5. group tier
GROUP_CASES = [(20, 65, 1, 1, 65), (64, 514, 2, 2, 257), (2047, 21, 3, 64, 7), (255, 675, 25, 8, 27),
               (32, 1024, 1, 1, 1024), (2048, 288, 32, 64, 9)]  # (nx, ny, R, lanes per strip, strips)
GROUP_GENS = (1, 2, 3, 33)


@pytest.mark.parametrize("case", GROUP_CASES, ids=lambda c: f"{c[0]}x{c[1]}-R{c[2]}-L{c[3]}")
def test_group_tier_trace(gpu, oracle, case):
    lm = gpu
    nx, ny, rows, lanes, strips = case
    assert_plan(lm, nx, ny, rows, lanes, strips)
    start = soups(nx, ny, 5, 100 * nx + ny)
    want = oracle_trace(oracle, start, max(GROUP_GENS))
    assert_varied(want, nx * ny)
    for count in (1, 5):
        with lm.LifeBatch(nx, ny, count, population=True) as on, lm.LifeBatch(nx, ny, count) as off:
            assert on.tier == "group"
            for n in GROUP_GENS:
                for b in (on, off):
                    b.upload(start[:count])
                    b.step(n)
                trace = same_as_off(on, off, n)
                np.testing.assert_array_equal(trace, want[:count, :n], err_msg=f"count {count} gens {n}")


# ---- 6. protocol
def test_only_the_last_call_is_kept_and_the_option_toggles(gpu):
    lm = gpu
    nx, ny, count = 33, 7, 5
    start = soups(nx, ny, count, 900, 0.4)
    want = rule_trace(start, 33 + 6, R.CONWAY)
    assert_varied(want, nx * ny)
    with lm.LifeBatch(nx, ny, count, population=True) as b:
        assert b.population().shape == (count, 0)  # before any call
        b.upload(start)
        b.step(20)
        np.testing.assert_array_equal(b.population(), want[:, :20])
        b.step(13)
        np.testing.assert_array_equal(b.population(), want[:, 20:33])  # 20 then 13 leaves G = 13
        b.step(0)
        assert b.population().shape == (count, 0) and b.generation == 33
        b.step(2)
        np.testing.assert_array_equal(b.population(), want[:, 33:35])
        b.configure(lm.BATCH_OPT_POPULATION, 0)
        assert b.population().shape == (count, 0)  # off: nothing to read
        b.step(2)
        assert b.population().shape == (count, 0)
        b.configure(lm.BATCH_OPT_POPULATION, 1)
        assert b.population().shape == (count, 0)  # on again: the next call records
        b.step(2)
        np.testing.assert_array_equal(b.population(), want[:, 37:39])
        np.testing.assert_array_equal(b.gather(), np.stack([R.rule_run(s, 39, R.CONWAY) for s in start]))
        for value in (2, -1):
            with pytest.raises(lm.LifeError) as e:
                b.configure(lm.BATCH_OPT_POPULATION, value)
            assert e.value.rc == LIFE_EINVAL
    with lm.LifeBatch(nx, ny, count) as b:  # never on
        b.upload(start)
        b.step(3)
        assert b.population().shape == (count, 0)


def test_ranges_and_what_leaves_the_trace_alone(gpu):
    lm = gpu
    nx, ny, count, n = 33, 7, 7, 9
    start = soups(nx, ny, count, 300)
    want = rule_trace(start, n, R.CONWAY)
    assert_varied(want, nx * ny)
    with lm.LifeBatch(nx, ny, count, population=True) as b:
        b.upload(start)
        b.step(n)
        full = b.population()
        np.testing.assert_array_equal(full, want)
        np.testing.assert_array_equal(b.population(2, 3), want[2:5])
        np.testing.assert_array_equal(b.population(6), want[6:])
        assert b.population(7, 0).shape == (0, n)
        for first, m in ((-1, 1), (0, 8), (7, 1), (3, -1), (8, 0)):  # as gather refuses them
            with pytest.raises(lm.LifeError) as e:
                b.population(first, m)
            assert e.value.rc == LIFE_EINVAL, (first, m)
            with pytest.raises(lm.LifeError):
                b.gather(first, m)
        # uploads, fills and rule changes leave the trace readable
        b.upload(start[:2], first=3)
        np.testing.assert_array_equal(b.population(), want)
        b.set_rule("B36/S23")
        np.testing.assert_array_equal(b.population(), want)
        b.set_rules([R.CONWAY, R.PARITY], first=1)
        np.testing.assert_array_equal(b.population(), want)
        assert lm._lib().life_batch_set_rule_gen(b._h, 0x48, 0x0C, 2) == 0  # two states through the _gen entry point
        assert b.rule == "B36/S23"
        np.testing.assert_array_equal(b.population(), want)
        b.fill_random(5, 0.3)
        np.testing.assert_array_equal(b.population(), want)
        b.step(1)
        assert b.population().shape == (count, 1)


def test_a_call_beyond_the_entry_cap_is_refused(gpu):
    lm = gpu
    nx, ny, count = 33, 7, 67
    start = soups(nx, ny, count, 500)
    with lm.LifeBatch(nx, ny, count, population=True) as b:
        b.upload(start)
        b.step(4)
        before, trace = b.gather(), b.population()
        with pytest.raises(lm.LifeError) as e:
            b.step(2**24 + 1)  # 67 x (2^24 + 1) > 2^30 entries
        assert e.value.rc == LIFE_EINVAL and "split the call" in str(e.value), str(e.value)
        assert b.generation == 4
        np.testing.assert_array_equal(b.gather(), before)
        np.testing.assert_array_equal(b.population(), trace)
        b.configure(lm.BATCH_OPT_POPULATION, 0)  # without the option the cap does not apply: only the range check
        with pytest.raises(lm.LifeError):
            b.step(2**31)


def test_generations_rules_and_the_option_refuse_each_other(gpu):
    lm = gpu
    with lm.LifeBatch(33, 7, 3, rule="B2/S/C3") as b:
        with pytest.raises(lm.LifeError) as e:
            b.configure(lm.BATCH_OPT_POPULATION, 1)
        assert e.value.rc == LIFE_EINVAL and "life_batch_set_rule_gen" in str(e.value), str(e.value)
        b.set_rule("B3/S23")
        b.configure(lm.BATCH_OPT_POPULATION, 1)
    with lm.LifeBatch(33, 7, 3, rules=["B3/S23", "B2/S/C3", "B3/S23"]) as b:
        with pytest.raises(lm.LifeError) as e:
            b.configure(lm.BATCH_OPT_POPULATION, 1)
        assert e.value.rc == LIFE_EINVAL and "life_batch_set_rules_gen" in str(e.value), str(e.value)
    with lm.LifeBatch(33, 7, 3, population=True) as b:
        for call in (lambda: b.set_rule("B2/S/C3"), lambda: b.set_rules(["B3/S23", "B2/S/C3"], first=1)):
            with pytest.raises(lm.LifeError) as e:
                call()
            assert e.value.rc == LIFE_EINVAL and "LIFE_BATCH_OPT_POPULATION" in str(e.value), str(e.value)
        assert b.rule == "B3/S23"  # nothing changed
        u32 = np.uint32
        birth, survive, states = np.array([0x48, 0x04], u32), np.array([0x0C, 0x00], u32), np.array([2, 2], u32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        assert lm._lib().life_batch_set_rules_gen(b._h, 1, 2, birth.ctypes.data_as(u32p), survive.ctypes.data_as(u32p),
                                                  states.ctypes.data_as(u32p)) == 0  # two states each: accepted
        assert b.rules == ["B3/S23", "B36/S23", "B2/S"]
        start = soups(33, 7, 3, 700)
        b.upload(start)
        b.step(5)
        np.testing.assert_array_equal(b.population(), rule_trace(start, 5, [R.CONWAY, (0x48, 0x0C), (0x04, 0x00)]))


def test_group_tier_takes_the_option_and_no_other(gpu):
    lm = gpu
    with lm.LifeBatch(160, 96, 2) as b:
        b.configure(lm.BATCH_OPT_POPULATION, 1)
        for option in (lm.BATCH_OPT_SETTLE, lm.BATCH_OPT_CYCLE):
            with pytest.raises(lm.LifeError) as e:
                b.configure(option, 1)
            assert e.value.rc == LIFE_EINVAL
        start = soups(160, 96, 2, 800)
        b.upload(start)
        b.step(20)
        b.step(13)
        np.testing.assert_array_equal(b.population(),
                                      rule_trace(np.stack([R.rule_run(s, 20, R.CONWAY) for s in start]), 13, R.CONWAY))
