"""Generations rules on the batch's wave tier: every cell of
every universe compared with the numpy reference written from the contract
(gen_ref.py; test_gen_host.py pins it), through upload_states / gather_states."""
import numpy as np
import pytest

import gen_ref as G
import rule_ref as R
from test_gpu_batch import check_census, soups

pytestmark = pytest.mark.gpu

LIFE_EINVAL, LIFE_ESTATE = -1, -5
SHAPES = [(1, 1), (2, 3), (32, 32), (33, 7), (64, 64), (100, 37), (127, 63), (128, 64)]  # every W; q < 32 and q = 32
COUNTS = (5, 67)
# B2/S/C3, B34/S12/C3, B2/S345/C4, Frogs' masks at C = 5 ... one rule for each count of planes and HighLife as a
# two-state rule through the _gen call
RULES = [(0x04, 0x00, 3), (0x18, 0x06, 3), (0x04, 0x38, 4), (0x18, 0x06, 5), (0x0C, 0x1C, 9), (0x04, 0x38, 16),
         (0x48, 0x0C, 2)]
# mixed_soup(128, 64, c, seed) holds every (class, neighbours) pair at these seeds (asserted below)
SEEDS = {2: 46, 3: 1, 4: 1, 5: 1, 9: 3, 16: 4}


def rule_id(rule):
    return f"B{rule[0]:03x}S{rule[1]:03x}C{rule[2]}"


def soup_stack(nx, ny, c, count=max(COUNTS)):
    return np.stack([G.mixed_soup(nx, ny, c, SEEDS[c] + 1000 * u) for u in range(count)])


def check_states(batch, want, what=""):
    """every cell, and the three figures of census_gen"""
    n = len(want)
    np.testing.assert_array_equal(batch.gather_states(), want, err_msg=what)
    live, dying, sums = batch.census_gen()
    want_live, want_dying, want_sums = G.census_stack(want)
    np.testing.assert_array_equal(live[:n], want_live, err_msg=what)
    np.testing.assert_array_equal(dying[:n], want_dying, err_msg=what)
    np.testing.assert_array_equal(sums[:n], want_sums, err_msg=what)
    np.testing.assert_array_equal(batch.dying_counts(), want_dying)
    np.testing.assert_array_equal(batch.state_checksums(), want_sums)


# ---- 1. parity with the reference
@pytest.mark.parametrize("rule", RULES, ids=rule_id)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_parity_with_the_reference(gpu, nx, ny, rule):
    lm = gpu
    c = rule[2]
    start = soup_stack(nx, ny, c)
    if (nx, ny) == (128, 64):
        assert G.classes(start[0]) == G.all_classes(c), sorted(G.all_classes(c) - G.classes(start[0]))
    stops = sorted({0, 1, 2, c + 1, 33})
    want, state = {0: start}, start
    for g in range(1, 34):
        state = G.gen_step(state, *rule)
        if g in stops or g == 20:
            want[g] = state
    if nx * ny >= 1024:  # (the smaller shapes have fewer cells than states)
        for g in stops:
            if g <= c + 1:
                assert set(np.unique(want[g]).tolist()) == set(range(c)), g
    text = lm.format_rule_gen(*rule)
    for count in COUNTS:
        with lm.LifeBatch(nx, ny, count) as b:
            # the _gen call itself, at two states too (LifeBatch.set_rule routes those to life_batch_set_rule)
            lm._check(lm._lib().life_batch_set_rule_gen(b._h, *rule), "life_batch_set_rule_gen")
            assert b.rule == text and b.rules == [text] * count
            assert b.states.tolist() == [c] * count
            b.upload_states(start[:count])
            at = 0
            for g in stops:
                b.step(g - at)
                at = g
                assert b.generation == g
                check_states(b, want[g][:count], f"count {count} generation {g}")
            b.upload_states(start[:count])
            assert b.generation == 0
            b.step(20)
            check_states(b, want[20][:count], f"count {count} 20")
            b.step(13)
            check_states(b, want[33][:count], f"count {count} 20 + 13")


# ---- 2. a (rule, C) per universe
MIXES = {  # each with differing B/S; the largest C decides the planes the kernel carries for all
    "P4": [(0x04, 0x00, 3), (0x48, 0x0C, 2), (0x04, 0x38, 4), (0x0C, 0x1C, 9), (0x04, 0x38, 16), (0x08, 0x0C, 2),
           (0x18, 0x06, 3)],
    "P2": [(0x04, 0x00, 3), (0x48, 0x0C, 2), (0x18, 0x06, 5), (0x04, 0x38, 4)],
    "P1": [(0x04, 0x00, 3), (0x48, 0x0C, 2), (0x18, 0x06, 3)],
}


@pytest.mark.parametrize("detector", ["none", "settle", "cycle"])
@pytest.mark.parametrize("nx,ny,mix", [(33, 7, "P4"), (33, 7, "P2"), (33, 7, "P1"), (128, 64, "P4"), (64, 64, "P2")])
def test_a_rule_and_a_state_count_per_universe(gpu, nx, ny, mix, detector):
    lm = gpu
    count = 67
    rules = [MIXES[mix][u % len(MIXES[mix])] for u in range(count)]
    if mix == "P4":
        assert {r[2] for r in rules} == {2, 3, 4, 9, 16}
    start = np.stack([G.mixed_soup(nx, ny, r[2], 70 + u) for u, r in enumerate(rules)])
    want = {0: start}
    for g, frm in ((1, 0), (21, 1)):
        want[g] = np.stack([G.gen_run(s, g - frm, r) for s, r in zip(want[frm], rules)])
    with lm.LifeBatch(nx, ny, count, rules=rules, settle=detector == "settle", cycle=detector == "cycle") as b:
        birth, survive, states = b.rule_triples()
        assert list(zip(birth.tolist(), survive.tolist(), states.tolist())) == rules
        assert b.rules == [lm.format_rule_gen(*r) for r in rules]
        assert b.states.tolist() == [r[2] for r in rules]
        old_birth, old_survive = b.rule_masks()  # the two-state call gives the masks alone
        assert old_birth.tolist() == [r[0] for r in rules] and old_survive.tolist() == [r[1] for r in rules]
        with pytest.raises(lm.LifeError) as e:
            b.rule
        assert e.value.rc == LIFE_ESTATE
        b.upload_states(start)
        check_states(b, start)
        b.step(1)
        check_states(b, want[1], "generation 1")
        b.step(20)
        check_states(b, want[21], "generation 21")
        # a range takes new rules: its dying cells go dead, its alive cells stay, the others keep every state
        fresh = [(0x04, 0x38, 16), (0x48, 0x0C, 2), (0x04, 0x00, 3)]
        b.set_rules(fresh, first=5)
        after = want[21].copy()
        after[5:8] = after[5:8] == 1
        check_states(b, after, "after set_rules")
        rules[5:8] = fresh
        assert b.rules == [lm.format_rule_gen(*r) for r in rules]
        b.step(3)
        check_states(b, np.stack([G.gen_run(s, 3, r) for s, r in zip(after, rules)]), "3 more")


# ---- 3. the detectors see the whole state
def lone_cell():
    grid = np.zeros((1, 5, 33), np.uint8)
    grid[0, 2, 17] = 1
    return grid


def test_settle_compares_every_plane(gpu):
    """B/S/C16: a lone cell is dead from generation 15 on, so S_g == S_(g-2)
    first at 17; its alive plane alone is empty from generation 1 on (3)."""
    with gpu.LifeBatch(33, 5, 1, rule="B/S/C16", settle=True) as b:
        b.upload_states(lone_cell())
        b.step(64)
        assert b.settled().tolist() == [17]
        assert not b.gather_states().any()


def test_cycle_compares_every_plane(gpu):
    """Brent's checkpoints fall at 0, 1, 3, 7, 15: the dead state of generation
    15 repeats at 16 (the alive plane alone: generation 1 repeats at 2)."""
    with gpu.LifeBatch(33, 5, 1, rule="B/S/C16", cycle=True) as b:
        b.upload_states(lone_cell())
        b.step(64)
        period, found = b.cycles()
        assert (period.tolist(), found.tolist()) == ([1], [16])
        assert not b.gather_states().any()


def test_cycle_of_the_brain_ship(gpu):
    """Period 40 on a 40 x 7 torus: the first checkpoint c with c + 1 >= 40 is
    63, so it is found at 103."""
    start = G.brain_ship(40, 7, True)[None]
    want = G.gen_run(start, 128, G.BRAIN)
    np.testing.assert_array_equal(want, np.roll(start, 128 % 40, 2))
    with gpu.LifeBatch(40, 7, 1, rule="B2/S/C3", cycle=True) as b:
        b.upload_states(start)
        b.step(128)
        period, found = b.cycles()
        assert (period.tolist(), found.tolist()) == ([40], [103])
        check_states(b, want)


@pytest.mark.parametrize("rule", [(0x04, 0x00, 3), (0x18, 0x06, 5), (0x04, 0x38, 16)], ids=rule_id)
def test_detectors_change_no_state(gpu, rule):
    lm = gpu
    nx, ny, count, c = 33, 7, 9, rule[2]
    start = soup_stack(nx, ny, c, count)
    start[7] = 0
    start[8] = 0
    start[8, 3, 4] = 1  # a lone cell: settles, and is found cyclic, whatever the rule (B2 at the least)
    want = G.gen_run(start, 150, rule)
    got = []
    for detector in ("none", "settle", "cycle"):
        with lm.LifeBatch(nx, ny, count, rule=rule, settle=detector == "settle", cycle=detector == "cycle") as b:
            b.upload_states(start)
            b.step(97)
            b.step(53)
            got.append(b.gather_states())
            if detector == "settle":
                assert b.settled()[7] == 2 and b.settled()[8] > 0
            if detector == "cycle":
                assert b.cycles()[0][7] == 1 and b.cycles()[0][8] == 1
    for g in got:
        np.testing.assert_array_equal(g, want)


# ---- 4. the two-state calls on a Generations batch
def test_old_calls_on_a_generations_batch(gpu, oracle):
    lm = gpu
    nx, ny, count = 100, 37, 7
    rule = (0x04, 0x38, 4)
    start = soup_stack(nx, ny, 4, count)
    with lm.LifeBatch(nx, ny, count, rule="B2/S345/C4") as b:
        b.upload_states(start)
        alive = (start == 1).astype(np.uint8)
        np.testing.assert_array_equal(b.gather(), alive)  # gather: the alive plane
        check_census(b, oracle, alive)  # census: the alive cells alone
        assert b.dying_counts().sum() > 0
        with pytest.raises(lm.LifeError) as e:
            lm._check(lm._lib().life_batch_get_rule(b._h, None, None), "life_batch_get_rule")
        assert e.value.rc == LIFE_ESTATE and "life_batch_get_rule_gen" in str(e.value)
        b.step(2)
        check_states(b, G.gen_run(start, 2, rule))
        # upload: nonzero is alive, and the universes written lose their dying cells; the others keep theirs
        b.upload_states(start)
        b.upload(start[2:5], first=2)
        want = start.copy()
        want[2:5] = start[2:5] != 0
        check_states(b, want)
        # fill_random: the alive plane of a two-state batch with the same seed, nothing dying
        b.upload_states(start)
        b.fill_random(77, 0.5)
        with lm.LifeBatch(nx, ny, count) as two:
            two.fill_random(77, 0.5)
            filled = two.gather()
        check_states(b, filled)
        assert b.dying_counts().tolist() == [0] * count
        b.step(5)
        check_states(b, G.gen_run(filled, 5, rule))
        # back to two states: the dying cells are dropped, the run is the Life-like rule's
        b.upload_states(start)
        b.set_rule("B3/S23")
        assert b.rule == "B3/S23" and b.states.tolist() == [2] * count
        check_states(b, alive)
        b.step(9)
        want = np.stack([R.rule_run(g, 9, R.CONWAY) for g in alive])
        np.testing.assert_array_equal(want, np.stack([oracle.life_run(g, 9) for g in alive]))
        np.testing.assert_array_equal(b.gather(), want)
        check_states(b, want)
        check_census(b, oracle, want)
        with pytest.raises(lm.LifeError) as e:  # a two-state batch takes no dying cell
            b.upload_states(start)
        assert e.value.rc == LIFE_EINVAL
    with lm.LifeBatch(nx, ny, count) as b:  # a batch that never saw such a rule: the state calls are upload / gather
        b.upload_states(alive)
        np.testing.assert_array_equal(b.gather_states(), alive)
        check_states(b, alive)


# ---- 5. refusals change nothing
def test_refusals_change_nothing(gpu):
    lm = gpu
    nx, ny, count = 33, 7, 6
    rule = (0x04, 0x38, 4)
    start = soup_stack(nx, ny, 4, count)

    def refused(call, *needles):
        with pytest.raises(lm.LifeError) as e:
            call()
        assert e.value.rc == LIFE_EINVAL, str(e.value)
        for needle in needles:
            assert needle in str(e.value), str(e.value)

    for mixed in (False, True):
        with lm.LifeBatch(nx, ny, count, rule=rule) as b:
            rules = [rule] * count
            if mixed:
                rules[1:3] = [(0x04, 0x00, 3), (0x48, 0x0C, 2)]
                b.set_rules(rules[1:3], first=1)
                start[1] = np.minimum(start[1], 2)
                start[2] = start[2] == 1
            b.upload_states(start)
            b.step(3)
            before = G.gen_run(start[0], 3, rule)

            def unchanged():
                assert b.rules == [lm.format_rule_gen(*r) for r in rules]
                np.testing.assert_array_equal(b.gather_states()[0], before)
                np.testing.assert_array_equal(b.gather_states(3), np.stack([G.gen_run(s, 3, rule) for s in start[3:]]))
                assert b.generation == 3

            for bad, needle in (((4, 0, 1), "1 states"), ((4, 0, 17), "17 states"), ((4, 0, 0), "0 states"),
                                ((5, 0, 3), "B0"), ((1 << 9, 0, 3), "bits above 8"), ((4, 1 << 9, 3), "bits above 8")):
                refused(lambda: lm._check(lm._lib().life_batch_set_rule_gen(b._h, *bad), "set_rule_gen"), needle)
                unchanged()
                refused(lambda: b.set_rules([(4, 0, 3), bad, (4, 0, 16)], first=2), "entry 1", needle)
                unchanged()
            for first, n in ((-1, 1), (0, count + 1), (count, 1), (count - 1, 2), (count + 1, 0)):
                refused(lambda: b.set_rules([(4, 0, 3)] * n, first=first))
                refused(lambda: b.rule_triples(first, n))
                refused(lambda: b.upload_states(start[:1].repeat(n, 0), first=first))
                refused(lambda: b.gather_states(first, n))
                unchanged()
            refused(lambda: b.rule_triples(3, -1))
            refused(lambda: b.gather_states(3, -1))
            # a byte at or above the state count of its universe: the universe and the value are named
            bad = start.copy()
            bad[4, 5, 6] = 4
            refused(lambda: b.upload_states(bad), "universe 4", "holds 4")
            refused(lambda: b.upload_states(bad[3:], first=3), "universe 4", "holds 4")
            unchanged()
            if mixed:  # universe 1 has three states, universe 2 two
                bad = start.copy()
                bad[1, 0, 0] = 3
                refused(lambda: b.upload_states(bad), "universe 1", "holds 3")
                bad = start.copy()
                bad[2, 6, 32] = 2
                refused(lambda: b.upload_states(bad), "universe 2", "holds 2")
                unchanged()
    with lm.LifeBatch(500, 500, 2) as b:  # group tier: two states
        grids = soups(500, 500, 2, 9)
        b.upload(grids)
        refused(lambda: b.set_rule("B3/S23/C3"), "group-tier")
        refused(lambda: b.set_rules(["B3/S23", "B3/S23/C3"]), "entry 1", "group-tier")
        assert b.rule == "B3/S23" and b.states.tolist() == [2, 2]
        b.set_rule((0x08, 0x0C, 2))  # B3/S23 as a triple is the two-state call
        np.testing.assert_array_equal(b.gather_states(), grids)
        np.testing.assert_array_equal(b.dying_counts(), [0, 0])
        np.testing.assert_array_equal(b.state_checksums(), b.checksums())
