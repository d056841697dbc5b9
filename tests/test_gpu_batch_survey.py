"""Batch surveys on the GPU: a rule per universe
(life_batch_set_rules) and cycle detection of any period (LIFE_BATCH_OPT_CYCLE),
every universe compared with the numpy rule reference and the oracle, every
(period, generation) pair with the CPU replay of the algorithm as the header
defines it (test_batch_survey_host.py pins that replay to brute force)."""
import numpy as np
import pytest

import rule_ref as R
from test_batch_survey_host import HAND_WANT, brent_run, hand_patterns
from test_gpu_batch import DENSITIES, check_census, oracle_runs

pytestmark = pytest.mark.gpu

LIFE_EINVAL, LIFE_ESTATE = -1, -5
RULESET = [R.NAMED["B36/S23"], R.NAMED["B3678/S34678"], R.NAMED["B2/S"], R.NAMED["B1357/S1357"],
           R.NAMED["B3/S012345678"]] + R.conway_flips()  # 22: the four waves of a workgroup always differ
COUNT = 67
SHAPES = [(33, 7), (64, 64), (128, 64), (1, 1)]


def rules_of(count):
    return [RULESET[u % len(RULESET)] for u in range(count)]


def mixed_start(nx, ny, count=COUNT):
    return np.stack([R.soup(nx, ny, 40 + u, DENSITIES[u % len(DENSITIES)]) for u in range(count)])


def runs(start, gens, rules):
    return np.stack([R.rule_run(s, gens, r) for s, r in zip(start, rules)])


def pairs(hits):
    return np.array([h[0] for h in hits], np.int64), np.array([h[1] for h in hits], np.int64)


def check_cycles(batch, hits, gen0=0):
    period, found = batch.cycles()
    want_p, want_g = pairs(hits)
    np.testing.assert_array_equal(period, want_p)
    np.testing.assert_array_equal(found, np.where(want_g < 0, -1, want_g + gen0))


# ---- 1. per-universe rules
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_a_rule_per_universe(gpu, oracle, nx, ny):
    lm = gpu
    assert len(RULESET) == 22
    rules, start = rules_of(COUNT), mixed_start(nx, ny)
    seen, states = set(), start
    for _ in range(9):  # the states the rules are applied to
        if (nx, ny) != (1, 1):
            for s in states:
                seen |= R.coverage(s)
        states = np.stack([R.rule_step(s, *r) for s, r in zip(states, rules)])
    if (nx, ny) != (1, 1):  # (a 1 x 1 universe is its own eight neighbours: two pairs only)
        assert seen == R.ALL_PAIRS, sorted(R.ALL_PAIRS - seen)
    with lm.LifeBatch(nx, ny, COUNT) as b:
        b.set_rules(rules)
        assert b.rules == [lm.format_rule(*r) for r in rules]
        b.upload(start)
        b.step(9)
        got = b.gather()
        for u in range(COUNT):
            np.testing.assert_array_equal(got[u], states[u], err_msg=f"universe {u} {lm.format_rule(*rules[u])}")
        assert b.generation == 9
        # back to one rule: the uniform kernels, the oracle's rule
        b.set_rule("B3/S23")
        b.upload(start)
        b.step(9)
        want = oracle_runs(oracle, start, 9)
        np.testing.assert_array_equal(b.gather(), want)
        check_census(b, oracle, want)
        assert b.rule == "B3/S23"
        assert b.rules == ["B3/S23"] * COUNT
    with lm.LifeBatch(nx, ny, 5, rules=rules[:5]) as b:  # the constructor's form; B3/S23 universes run the table too
        b.set_rules([R.CONWAY], first=4)
        b.upload(start[:5])
        b.step(9)
        np.testing.assert_array_equal(b.gather(), runs(start[:5], 9, rules[:4] + [R.CONWAY]))


# ---- 2. ranges and refusals
def test_ranges_and_refusals(gpu):
    lm = gpu
    nx, ny = 33, 7
    start = mixed_start(nx, ny, 7)
    highlife, seeds, conway = R.NAMED["B36/S23"], R.NAMED["B2/S"], R.CONWAY
    with lm.LifeBatch(nx, ny, 7, rule="B3678/S34678") as b:
        daynight = R.NAMED["B3678/S34678"]
        b.set_rules([highlife, seeds], first=3)
        want_rules = [daynight] * 3 + [highlife, seeds] + [daynight] * 2
        assert b.rules == [lm.format_rule(*r) for r in want_rules]
        birth, survive = b.rule_masks(3, 2)
        assert birth.tolist() == [highlife[0], seeds[0]] and survive.tolist() == [highlife[1], seeds[1]]
        with pytest.raises(lm.LifeError) as e:
            b.rule
        assert e.value.rc == LIFE_ESTATE and "life_batch_get_rules" in str(e.value)
        b.upload(start)
        b.step(9)
        np.testing.assert_array_equal(b.gather(), runs(start, 9, want_rules))
        assert b.generation == 9
        b.set_rules([])  # a no-op
        b.set_rules([], first=7)
        # a refused call changes nothing, and names the entry and its rule
        for bad, text in (((conway[0] | 1, conway[1]), "B03/S23"), ((conway[0], 1 << 9), "0x200")):
            with pytest.raises(lm.LifeError) as e:
                b.set_rules([seeds, bad, seeds], first=0)
            assert e.value.rc == LIFE_EINVAL
            assert "entry 1" in str(e.value) and text in str(e.value), str(e.value)
        for first, n in ((-1, 1), (0, 8), (7, 1), (6, 2), (8, 0)):
            with pytest.raises(lm.LifeError) as e:
                b.set_rules([seeds] * n, first=first)
            assert e.value.rc == LIFE_EINVAL, (first, n)
            with pytest.raises(lm.LifeError) as e:
                b.rule_masks(first, n)
            assert e.value.rc == LIFE_EINVAL, (first, n)
        with pytest.raises(lm.LifeError) as e:
            b.rule_masks(3, -1)
        assert e.value.rc == LIFE_EINVAL
        assert b.rules == [lm.format_rule(*r) for r in want_rules]
        assert b.generation == 9  # the generation counter and the states were left alone
        b.step(4)
        np.testing.assert_array_equal(b.gather(), runs(start, 13, want_rules))
        # mixed whatever the values, until set_rule
        b.set_rules([daynight] * 7)
        with pytest.raises(lm.LifeError) as e:
            b.rule
        assert e.value.rc == LIFE_ESTATE
        b.set_rule(daynight)
        assert b.rule == "B3678/S34678"
    with lm.LifeBatch(500, 500, 3) as b:  # group tier: set_rule's refusal
        with pytest.raises(lm.LifeError) as e:
            b.set_rules([conway, highlife, conway])
        assert e.value.rc == LIFE_EINVAL and "entry 1" in str(e.value) and "B36/S23" in str(e.value)
        b.set_rules([conway] * 3)
        b.set_rules([conway], first=2)
        assert b.rules == ["B3/S23"] * 3


# ---- 3. settle under mixed rules
def test_settle_under_mixed_rules(gpu, oracle):
    lm = gpu
    nx, ny = 33, 7
    rules, start = rules_of(COUNT), mixed_start(nx, ny)
    got = []
    for settle in (False, True):
        with lm.LifeBatch(nx, ny, COUNT, rules=rules, settle=settle) as b:
            b.upload(start)
            b.step(301)
            b.step(40)
            got.append((b.gather(), b.live_counts(), b.checksums()))
            flagged = b.settled() >= 0
            assert flagged.any() == settle
    for off, on in zip(*got):
        np.testing.assert_array_equal(off, on)
    want = runs(start, 341, rules)
    np.testing.assert_array_equal(got[1][0], want)
    np.testing.assert_array_equal(got[1][1], want.reshape(COUNT, -1).sum(axis=1))
    np.testing.assert_array_equal(got[1][2], np.array([oracle.checksum(g) for g in want], dtype=np.uint64))


# ---- 4. cycles by hand
def test_cycles_by_hand(gpu, oracle):
    lm = gpu
    grids = hand_patterns()
    replay = [brent_run(g, 700, R.CONWAY)[0] for g in grids]
    assert replay == HAND_WANT
    with lm.LifeBatch(32, 32, 7, cycle=True) as b:
        period, found = b.cycles()
        assert period.tolist() == [0] * 7 and found.tolist() == [-1] * 7
        b.upload(grids)
        b.step(700)
        period, found = b.cycles()
        assert list(zip(period.tolist(), found.tolist())) == HAND_WANT
        check_cycles(b, replay)
        want = oracle_runs(oracle, grids, 700)
        np.testing.assert_array_equal(b.gather(), want)
        check_census(b, oracle, want)
        b.step(7)  # the flagged universes run 7 mod period generations, the soup a new detection from 700 on
        again = brent_run(want[6], 7, R.CONWAY)[0]
        want = oracle_runs(oracle, want, 7)
        np.testing.assert_array_equal(b.gather(), want)
        assert b.generation == 707
        period, found = b.cycles()  # what was found is kept
        now = HAND_WANT[:6] + [(again[0], 700 + again[1] if again[0] else -1)]
        assert list(zip(period.tolist(), found.tolist())) == now
        np.testing.assert_array_equal(b.settled(), [-1] * 7)
        # an upload resets its universe's pair and no other; a new rule resets all
        b.upload(grids[3:4], first=1)
        period, found = b.cycles()
        assert list(zip(period.tolist(), found.tolist())) == [now[0], (0, -1)] + now[2:]
        b.set_rules([R.CONWAY], first=2)
        period, found = b.cycles()
        assert list(zip(period.tolist(), found.tolist())) == [now[0], (0, -1), (0, -1)] + now[3:]
        b.set_rule("B3/S23")
        period, found = b.cycles()
        assert period.tolist() == [0] * 7 and found.tolist() == [-1] * 7
        b.step(5)
        b.fill_random(3, 0.5)
        period, found = b.cycles()
        assert period.tolist() == [0] * 7 and found.tolist() == [-1] * 7


def test_cycle_detection_restarts_per_call(gpu, oracle):
    """The glider of a 32 x 32 torus, period 128: found at generation 255 of
    one call and by no shorter one, nor by two calls that add up to it."""
    glider = hand_patterns()[3:4]
    for calls, want in (((254,), (0, -1)), ((255,), (128, 255)), ((100, 155), (0, -1))):
        with gpu.LifeBatch(32, 32, 1, cycle=True) as b:
            b.upload(glider)
            for n in calls:
                b.step(n)
            period, found = b.cycles()
            assert (int(period[0]), int(found[0])) == want, calls
            np.testing.assert_array_equal(b.gather(), oracle_runs(oracle, glider, sum(calls)))


# ---- 5. cycle soups
@pytest.fixture(scope="module")
def cycle_soups():
    start = np.stack([R.soup(32, 32, 7000 + u, 0.35) for u in range(32)])
    out = [brent_run(s, 2048, R.CONWAY, keep=(2047, 2048)) for s in start]
    return start, [o[0] for o in out], {n: np.stack([o[1][n] for o in out]) for n in (2047, 2048)}


@pytest.mark.parametrize("n", [2048, 2047])
def test_cycle_soups(gpu, oracle, cycle_soups, n):
    start, hits, states = cycle_soups
    hits = [h if 0 < h[1] <= n else (0, -1) for h in hits]  # one Brent run: what a call of n finds is what it found by n
    found = sum(h[0] > 0 for h in hits)
    print("cycle soups", n, "found", found, "periods", sorted({h[0] for h in hits}), hits)
    assert found >= 20 and len(hits) - found >= 2, hits
    with gpu.LifeBatch(32, 32, len(start), cycle=True) as b:
        b.upload(start)
        b.step(n)
        check_cycles(b, hits)
        np.testing.assert_array_equal(b.gather(), states[n])
        check_census(b, oracle, states[n])
        np.testing.assert_array_equal(b.settled(), [-1] * len(start))
    if n == 2048:  # the reference of this file is the oracle's
        np.testing.assert_array_equal(states[n][:4], oracle_runs(oracle, start[:4], n))


# ---- 6. cycles under mixed rules
def test_cycles_under_mixed_rules(gpu):
    lm = gpu
    nx, ny, n = 33, 7, 1500
    rules = RULESET + RULESET
    start = np.stack([R.soup(nx, ny, 40, 0.2)] * 22 + [R.soup(nx, ny, 41, 0.5)] * 22)
    out = [brent_run(s, n, r, keep=(n,)) for s, r in zip(start, rules)]
    hits, want = [o[0] for o in out], np.stack([o[1][n] for o in out])
    found = sum(h[0] > 0 for h in hits)
    print("mixed cycles found", found, "periods", sorted({h[0] for h in hits}), hits)
    assert found >= 20 and len(hits) - found >= 8 and max(h[0] for h in hits) > 2, hits
    with lm.LifeBatch(nx, ny, len(start), rules=rules, cycle=True) as b:
        b.upload(start)
        b.step(n)
        check_cycles(b, hits)
        got = b.gather()
        for u in range(len(start)):
            np.testing.assert_array_equal(got[u], want[u], err_msg=f"universe {u} {lm.format_rule(*rules[u])}")
        np.testing.assert_array_equal(b.live_counts(), want.reshape(len(want), -1).sum(axis=1))


# ---- 7. option refusals
def test_option_refusals_and_identical_states(gpu):
    lm = gpu
    assert lm.BATCH_OPT_CYCLE == 3
    with lm.LifeBatch(500, 500, 1) as b:
        with pytest.raises(lm.LifeError) as e:
            b.configure(lm.BATCH_OPT_CYCLE, 1)
        assert e.value.rc == LIFE_EINVAL
    with lm.LifeBatch(33, 7, 1) as b:
        b.configure(lm.BATCH_OPT_SETTLE, 1)
        with pytest.raises(lm.LifeError) as e:
            b.configure(lm.BATCH_OPT_CYCLE, 1)
        assert e.value.rc == LIFE_EINVAL
        b.configure(lm.BATCH_OPT_CYCLE, 0)
        b.configure(lm.BATCH_OPT_SETTLE, 0)
        b.configure(lm.BATCH_OPT_CYCLE, 1)
        with pytest.raises(lm.LifeError) as e:
            b.configure(lm.BATCH_OPT_SETTLE, 1)
        assert e.value.rc == LIFE_EINVAL
        for option, value in ((lm.BATCH_OPT_CYCLE, 2), (lm.BATCH_OPT_CYCLE, -1), (2, 1), (2, 0)):
            with pytest.raises(lm.LifeError) as e:
                b.configure(option, value)
            assert e.value.rc == LIFE_EINVAL, (option, value)
    with pytest.raises(lm.LifeError) as e:
        lm.LifeBatch(33, 7, 1, settle=True, cycle=True)
    assert e.value.rc == LIFE_EINVAL
    with lm.LifeBatch(32, 32, 2, settle=True) as b:  # the settled flags are not the cycle option's
        b.upload(hand_patterns()[1:3])
        b.step(4)
        assert b.settled().tolist() == [2, 2]
        b.configure(lm.BATCH_OPT_SETTLE, 0)
        b.configure(lm.BATCH_OPT_CYCLE, 1)
        b.step(4)
        assert b.settled().tolist() == [2, 2]
        period, found = b.cycles()
        assert period.tolist() == [1, 2] and found.tolist() == [5, 7]
    nx, ny = 127, 63
    start = np.stack([R.soup(nx, ny, 8100 + u, 0.35) for u in range(9)])
    got = []
    for cycle in (False, True):
        with lm.LifeBatch(nx, ny, 9, cycle=cycle) as b:
            b.upload(start)
            b.step(301)
            b.step(40)
            got.append((b.gather(), b.live_counts(), b.checksums()))
            if not cycle:
                period, found = b.cycles()
                assert period.tolist() == [0] * 9 and found.tolist() == [-1] * 9
    for off, on in zip(*got):
        np.testing.assert_array_equal(off, on)
    np.testing.assert_array_equal(got[0][0], np.stack([R.rule_run(s, 341, R.CONWAY) for s in start]))
