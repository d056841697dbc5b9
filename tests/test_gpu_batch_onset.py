"""Cycle onsets on the GPU (LIFE_BATCH_OPT_ONSET): every onset
compared with brute force over the numpy references (every state of the orbit
stored: test_batch_survey_host.brute_force, and its Generations equivalent
over gen_ref.gen_step), never with the library; the cycle pairs and the final
states beside them, and the option's resets and refusals."""
import functools

import numpy as np
import pytest

import gen_ref as G
import rule_ref as R
from test_batch_onset_host import (GEN_LINES, SOUP_LINES, gen_soups, onset_run, orbit, soups, state_after, want_of)
from test_batch_survey_host import brute_force, hand_patterns
from test_gpu_batch_survey import COUNT as MIXED_COUNT
from test_gpu_batch_survey import mixed_start, rules_of

pytestmark = pytest.mark.gpu

LIFE_EINVAL = -1


def columns(wants):
    """(period, found, onset) int64 arrays of a list of ((period, found), onset)"""
    return tuple(np.array(c, np.int64) for c in zip(*[(h[0], h[1], mu) for h, mu in wants]))


def check(batch, wants, gen0=0):
    period, found = batch.cycles()
    want_p, want_g, want_mu = columns(wants)
    np.testing.assert_array_equal(period, want_p)
    np.testing.assert_array_equal(found, np.where(want_g < 0, -1, want_g + gen0))
    np.testing.assert_array_equal(batch.onsets(), np.where(want_mu < 0, -1, want_mu + gen0))


def all_found_late(founds, n):
    """The condition of the soup tests, asserted on the reference before the
    GPU is compared: every cycle is found within the call, and mu > 0."""
    wants = [want_of(f, n) for f in founds]
    assert all(h[0] > 0 and mu > 0 for h, mu in wants), wants
    return wants


@functools.lru_cache(maxsize=None)
def soup_reference(nx, ny, rule, n):
    start = soups(nx, ny)
    founds = [brute_force(g, n, rule) for g in start]
    return start, founds, np.stack([state_after(g, n, f, rule) for g, f in zip(start, founds)])


# ---- 1. hand patterns
def test_onsets_by_hand(gpu):
    grids = hand_patterns()
    founds = [brute_force(g, 1500, R.CONWAY) for g in grids]
    wants = [want_of(f, 700) for f in founds]
    print("hand patterns", founds, wants)
    assert [mu for _, mu in wants[:4]] == [0, 0, 0, 0] and wants[6] == ((0, -1), -1)
    assert all(mu >= 0 for _, mu in wants[:6])
    with gpu.LifeBatch(32, 32, 7, cycle=True, onset=True) as b:
        np.testing.assert_array_equal(b.onsets(), [-1] * 7)
        b.upload(grids)
        b.step(700)
        check(b, wants)
        np.testing.assert_array_equal(b.gather(), np.stack([R.rule_run(g, 700, R.CONWAY) for g in grids]))
        assert b.generation == 700


# ---- 2. soups, every W
@pytest.mark.parametrize("nx,ny,rule,n", SOUP_LINES)
def test_soup_onsets(gpu, nx, ny, rule, n):
    start, founds, final = soup_reference(nx, ny, rule, n)
    wants = all_found_late(founds, n)
    print("soups", nx, ny, rule, "largest mu", max(mu for _, mu in wants), "periods", sorted({h[0] for h, _ in wants}))
    with gpu.LifeBatch(nx, ny, len(start), rule=rule, cycle=True, onset=True) as b:
        b.upload(start)
        b.step(n)
        check(b, wants)
        np.testing.assert_array_equal(b.gather(), final)
        np.testing.assert_array_equal(b.live_counts(), final.reshape(len(final), -1).sum(axis=1))


# ---- 3. a rule per universe
def test_onsets_under_a_rule_per_universe(gpu):
    lm = gpu
    nx, ny, n = 33, 7, 511
    rules, start = rules_of(MIXED_COUNT), mixed_start(nx, ny)
    wants = [onset_run(s, n, r) for s, r in zip(start, rules)]
    found = [(u, w) for u, w in enumerate(wants) if w[0][0]]
    print("mixed onsets", wants)
    assert len(found) >= 20 and len(wants) - len(found) >= 4 and sum(mu > 0 for _, (_, mu) in found) >= 10, wants
    final = np.stack([state_after(s, n, (w[1], w[0][0]) if w[0][0] else None, r)
                      for s, r, w in zip(start, rules, wants)])
    with lm.LifeBatch(nx, ny, MIXED_COUNT, rules=rules, cycle=True, onset=True) as b:
        b.upload(start)
        b.step(n)
        check(b, wants)
        got = b.gather()
        for u in range(MIXED_COUNT):
            np.testing.assert_array_equal(got[u], final[u], err_msg=f"universe {u} {lm.format_rule(*rules[u])}")


# ---- 4. Generations
@functools.lru_cache(maxsize=None)
def gen_reference(nx, ny, rules, n):
    start = np.stack([G.mixed_soup(nx, ny, r[2], 900 + u) for u, r in enumerate(rules)])
    founds = [orbit(g, n, r, G.gen_step) for g, r in zip(start, rules)]
    return start, founds, np.stack([state_after(g, n, f, r, G.gen_step) for g, f, r in zip(start, founds, rules)])


@pytest.mark.parametrize("nx,ny,rule", GEN_LINES)
def test_generations_onsets(gpu, nx, ny, rule):
    n = 1023
    start, founds, final = gen_reference(nx, ny, (rule,) * 48, n)
    np.testing.assert_array_equal(start, gen_soups(nx, ny, rule[2]))
    wants = all_found_late(founds, n)
    print("generations", nx, ny, rule, "largest mu", max(mu for _, mu in wants), "periods",
          sorted({h[0] for h, _ in wants}))
    with gpu.LifeBatch(nx, ny, len(start), rule=rule, cycle=True, onset=True) as b:
        b.upload_states(start)
        b.step(n)
        check(b, wants)
        np.testing.assert_array_equal(b.gather_states(), final)


MIX = (G.STARWARS, G.BRAIN, (0x08, 0x0C, 16), (0x08, 0x0C, 2))  # two, one and four planes' worth, and a two-state rule


def test_generations_onsets_under_a_rule_per_universe(gpu):
    nx, ny, n = 33, 7, 1023
    rules = tuple(MIX[u % len(MIX)] for u in range(48))
    start, founds, final = gen_reference(nx, ny, rules, n)
    wants = all_found_late(founds, n)
    with gpu.LifeBatch(nx, ny, len(start), rules=list(rules), cycle=True, onset=True) as b:
        b.upload_states(start)
        b.step(n)
        check(b, wants)
        np.testing.assert_array_equal(b.gather_states(), final)


# ---- 5. later calls
def test_onsets_of_later_calls(gpu):
    nx, ny, rule, n = SOUP_LINES[0]
    start, founds, _ = soup_reference(nx, ny, rule, n)
    first = [want_of(f, 100) for f in founds]  # found within step(100): the onset is mu
    # else the second call starts anew from S_100, whose orbit is (max(mu - 100, 0), lambda)
    later = [want_of((max(f[0] - 100, 0), f[1]), 1023) for f in founds]
    wants = [a if a[0][0] else ((h[0], h[1] + 100 if h[0] else -1), mu + 100 if h[0] else -1)
             for a, (h, mu) in zip(first, later)]
    early = [u for u, a in enumerate(first) if a[0][0]]
    late = [u for u, a in enumerate(first) if not a[0][0] and later[u][0][0]]
    print("later calls: found in the first", early, "in the second", late)
    assert len(early) >= 3 and len(late) >= 3
    for u in late:  # max(mu, 100), and both of its arms occur
        assert wants[u][1] == max(founds[u][0], 100)
    assert any(founds[u][0] > 100 for u in late) and any(founds[u][0] <= 100 for u in late)
    with gpu.LifeBatch(nx, ny, len(start), cycle=True, onset=True) as b:
        b.upload(start)
        b.step(100)
        check(b, first)
        b.step(1023)
        check(b, wants)
        np.testing.assert_array_equal(b.gather(), np.stack([state_after(g, 1123, f, rule)
                                                            for g, f in zip(start, founds)]))
        b.step(50)  # what was found is kept
        check(b, wants)
        assert b.generation == 1173


# ---- 6. identity
def test_everything_else_is_identical_with_the_option_on_and_off(gpu):
    nx, ny, rule, n = SOUP_LINES[1]
    start, founds, final = soup_reference(nx, ny, rule, n)
    got = {}
    for onset in (False, True):
        for population in (False, True):
            with gpu.LifeBatch(nx, ny, len(start), cycle=True, onset=onset, population=population) as b:
                b.upload(start)
                b.step(n)
                got[onset, population] = (b.gather(), *b.cycles(), b.live_counts(), b.checksums(), b.population(),
                                          b.onsets(), b.generation)
    for population in (False, True):
        for off, on in zip(got[False, population][:6], got[True, population][:6]):
            np.testing.assert_array_equal(off, on)
        assert got[False, population][7] == got[True, population][7] == n
        np.testing.assert_array_equal(got[False, population][6], [-1] * len(start))
    assert got[True, True][5].shape == (len(start), n)
    np.testing.assert_array_equal(got[True, True][6], got[True, False][6])  # the onsets, recording or not
    np.testing.assert_array_equal(got[True, True][6], [f[0] for f in founds])
    np.testing.assert_array_equal(got[True, True][0], final)
    # the trace itself, against the reference, for one universe: the search has recorded nothing
    state, counts = start[5], []
    for _ in range(n):
        state = R.rule_step(state, *rule)
        counts.append(int(state.sum()))
    np.testing.assert_array_equal(got[True, True][5][5], counts)


# ---- 7. resets and refusals
def test_resets(gpu):
    lm = gpu
    nx, ny, rule, n = SOUP_LINES[0]
    start, founds, _ = soup_reference(nx, ny, rule, n)
    want = np.array([f[0] for f in founds], np.int64)
    with lm.LifeBatch(nx, ny, len(start), cycle=True, onset=True) as b:
        def run():
            b.upload(start)
            b.step(n)
            np.testing.assert_array_equal(b.onsets(), want)

        run()
        b.upload(start[3:8], first=10)  # a partial upload clears exactly its range
        np.testing.assert_array_equal(b.onsets(), np.where((np.arange(len(start)) >= 10) & (np.arange(len(start)) < 15),
                                                           -1, want))
        b.set_rules([R.CONWAY] * 2, first=20)
        cleared = np.isin(np.arange(len(start)), [10, 11, 12, 13, 14, 20, 21])
        np.testing.assert_array_equal(b.onsets(), np.where(cleared, -1, want))
        period, found = b.cycles()
        np.testing.assert_array_equal(period == 0, cleared)  # exactly where the cycle pair went back to 0 / -1
        np.testing.assert_array_equal(found == -1, cleared)
        b.set_rule("B3/S23")
        np.testing.assert_array_equal(b.onsets(), [-1] * len(start))
        run()
        b.fill_random(3, 0.5)
        np.testing.assert_array_equal(b.onsets(), [-1] * len(start))
        run()
        # cycle off turns onset off: the next calls record neither, and cycle on again does not bring it back
        b.configure(lm.BATCH_OPT_CYCLE, 0)
        b.upload(start)
        b.step(n)
        np.testing.assert_array_equal(b.onsets(), [-1] * len(start))
        b.configure(lm.BATCH_OPT_CYCLE, 1)
        b.upload(start)
        b.step(n)
        assert (b.cycles()[0] > 0).all()
        np.testing.assert_array_equal(b.onsets(), [-1] * len(start))
        # turned on after the universes were flagged: they keep -1 until their flags are reset
        b.configure(lm.BATCH_OPT_ONSET, 1)
        b.step(n)
        np.testing.assert_array_equal(b.onsets(), [-1] * len(start))
        run()


def test_refusals(gpu):
    lm = gpu
    assert lm.BATCH_OPT_ONSET == 5
    group = soups(160, 96, 2)
    with lm.LifeBatch(160, 96, 2) as b:  # group tier
        b.upload(group)
        b.step(3)
        with pytest.raises(lm.LifeError) as e:
            b.configure(lm.BATCH_OPT_ONSET, 1)
        assert e.value.rc == LIFE_EINVAL and "group-tier" in str(e.value)
        assert b.generation == 3
        np.testing.assert_array_equal(b.gather(), np.stack([R.rule_run(g, 3, R.CONWAY) for g in group]))
        np.testing.assert_array_equal(b.onsets(), [-1, -1])
    with pytest.raises(lm.LifeError) as e:
        lm.LifeBatch(160, 96, 1, onset=True)
    assert e.value.rc == LIFE_EINVAL
    start = soups(33, 7, 3)
    with lm.LifeBatch(33, 7, 3) as b:
        b.upload(start)
        b.step(3)
        with pytest.raises(lm.LifeError) as e:  # onset without cycle
            b.configure(lm.BATCH_OPT_ONSET, 1)
        assert e.value.rc == LIFE_EINVAL and "LIFE_BATCH_OPT_CYCLE" in str(e.value)
        b.configure(lm.BATCH_OPT_ONSET, 0)  # off is always accepted
        b.configure(lm.BATCH_OPT_CYCLE, 1)
        for value in (2, -1):
            with pytest.raises(lm.LifeError) as e:
                b.configure(lm.BATCH_OPT_ONSET, value)
            assert e.value.rc == LIFE_EINVAL, value
        assert b.generation == 3
        np.testing.assert_array_equal(b.gather(), np.stack([R.rule_run(g, 3, R.CONWAY) for g in start]))
        b.step(40)  # the refused values left the option off
        np.testing.assert_array_equal(b.onsets(), [-1] * 3)
        b.configure(lm.BATCH_OPT_ONSET, 1)
    with pytest.raises(lm.LifeError) as e:
        lm.LifeBatch(33, 7, 1, onset=True)  # the constructor's form of onset without cycle
    assert e.value.rc == LIFE_EINVAL
    with lm.LifeBatch(33, 7, 3, cycle=True) as b:  # a batch that never had the option
        b.upload(start)
        b.step(600)
        np.testing.assert_array_equal(b.onsets(), [-1] * 3)
