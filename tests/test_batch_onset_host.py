"""Cycle onsets, host side (no GPU): the new option and call
are in the header and the binding, and the CPU replay of LIFE_BATCH_OPT_ONSET
-- Brent's two phases exactly as include/life_mi355x.h states them -- gives
the onset that brute force finds, wherever the first phase finds the cycle.
tests/test_gpu_batch_onset.py holds the GPU to the same brute force."""
import os
import re

import numpy as np
import pytest

import gen_ref as G
import rule_ref as R
from test_abi import declared_functions
from test_batch_survey_host import brent_from, brent_run, brute_force, hand_patterns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITIES = (0.25, 0.35, 0.5)
COUNT = 48
# (nx, ny, rule, n) of the soup lines of the GPU test: one shape per word count W = 1 .. 4, and two more rules
SOUP_LINES = [(16, 16, R.CONWAY, 1023), (33, 7, R.CONWAY, 1023), (70, 9, R.CONWAY, 1023), (100, 12, R.CONWAY, 2047),
              (16, 16, R.NAMED["B36/S23"], 1023), (33, 7, R.NAMED["B3678/S34678"], 1023)]
# (nx, ny, rule) of the Generations lines, n = 1023
GEN_LINES = [(33, 7, G.STARWARS), (12, 12, G.STARWARS), (33, 7, G.BRAIN), (70, 9, (0x08, 0x0C, 16))]


def soups(nx, ny, count=COUNT):
    return np.stack([R.soup(nx, ny, 900 + u, DENSITIES[u % 3]) for u in range(count)])


def gen_soups(nx, ny, c, count=COUNT):
    return np.stack([G.mixed_soup(nx, ny, c, 900 + u) for u in range(count)])


def orbit(grid, n, rule, step=R.rule_step):
    """brute_force of test_batch_survey_host.py under any step function (the
    Generations equivalent with G.gen_step): (mu, lambda) by storing every
    state up to n, None when no state repeats within n generations."""
    seen, state = {grid.tobytes(): 0}, grid
    for g in range(1, n + 1):
        state = step(state, *rule)
        first = seen.setdefault(state.tobytes(), g)
        if first != g:
            return first, g - first
    return None


def state_after(grid, n, found, rule, step=R.rule_step):
    """S_n, given (mu, lambda) of the orbit or None: on the cycle S_n is
    S_(mu + (n - mu) mod lambda), so no more than mu + lambda steps are taken."""
    if found and n > found[0]:
        n = found[0] + (n - found[0]) % found[1]
    for _ in range(n):
        grid = step(grid, *rule)
    return grid


def onset_run(grid, n, rule, step=R.rule_step):
    """One step call of n generations from S_0 = grid with LIFE_BATCH_OPT_CYCLE
    and LIFE_BATCH_OPT_ONSET on, as the header states it: ((period, generation
    found at), mu), or ((0, -1), -1) when the first phase finds nothing in n."""
    state, T, power, lam, g = grid, grid, 1, 0, 0
    while True:  # the first phase: Brent's detection
        if g == n:
            return (0, -1), -1
        g += 1
        state = step(state, *rule)
        lam += 1
        if np.array_equal(state, T):
            break
        if lam == power:
            T, power, lam = state, 2 * power, 0
    a = b = grid  # the second phase: S_0, and a copy advanced lam generations
    for _ in range(lam):
        b = step(b, *rule)
    mu = g - lam  # (never reached: S_(g-lam) == S_g)
    for m in range(g - lam):
        if np.array_equal(a, b):
            mu = m
            break
        a, b = step(a, *rule), step(b, *rule)
    return (lam, g), mu


def want_of(found, n):
    """What a call of n generations records for an orbit (mu, lambda) or None:
    ((period, found at), onset)."""
    hit = brent_from(*found, n) if found else (0, -1)
    return hit, (found[0] if hit[0] else -1)


def test_header_and_binding_know_the_option_and_the_call(lm):
    declared = declared_functions()
    assert "life_batch_onsets" in declared and "life_batch_onsets" in lm.ABI_SYMBOLS
    assert getattr(lm._lib(), "life_batch_onsets") is not None
    assert declared == sorted(lm.ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "life_mi355x.h")).read()
    # every option define, evaluated: a number, or an expression over the defines before it
    values = {}
    for name, text in re.findall(r"^#define (LIFE_BATCH_OPT_\w+) (.+)$", header, re.M):
        assert re.fullmatch(r"[\w\s()+]+", text), (name, text)
        values[name] = eval(text, {"__builtins__": {}}, dict(values))
    assert values["LIFE_BATCH_OPT_ONSET"] == lm.BATCH_OPT_ONSET == 5
    assert sorted(values.values()) == [1, 3, 4, 5]  # option 2 stays unassigned, and no number is used twice
    assert values == {"LIFE_BATCH_OPT_SETTLE": lm.BATCH_OPT_SETTLE, "LIFE_BATCH_OPT_CYCLE": lm.BATCH_OPT_CYCLE,
                      "LIFE_BATCH_OPT_POPULATION": lm.BATCH_OPT_POPULATION, "LIFE_BATCH_OPT_ONSET": lm.BATCH_OPT_ONSET}


@pytest.mark.parametrize("n", [700, 255, 30, 6])
def test_onset_replay_agrees_with_brute_force_on_the_hand_patterns(n):
    got = []
    for u, grid in enumerate(hand_patterns()):
        found = brute_force(grid, 1500, R.CONWAY)
        assert found == orbit(grid, 1500, R.CONWAY), u
        hit, mu = onset_run(grid, n, R.CONWAY)
        assert (hit, mu) == want_of(found, n), (u, n, found)
        assert hit == brent_run(grid, n, R.CONWAY)[0], u  # the first phase is the replay of LIFE_BATCH_OPT_CYCLE
        got.append(mu)
    if n == 700:  # empty, block, blinker and glider cycle from the start; the soup is not found
        assert got[:4] == [0, 0, 0, 0] and got[6] == -1 and min(got[4:6]) >= 0, got


@pytest.mark.parametrize("nx,ny,rule,n", SOUP_LINES)
def test_onset_replay_agrees_with_brute_force_on_the_soups(nx, ny, rule, n):
    mus = []
    for u, grid in enumerate(soups(nx, ny)):
        found = brute_force(grid, n, rule)
        hit, mu = onset_run(grid, n, rule)
        assert (hit, mu) == want_of(found, n), (u, found)
        mus.append(mu)
    # the condition the GPU test leans on: every cycle is found within the call, and none at generation 0
    assert min(mus) > 0, mus
    print("soups", nx, ny, rule, "largest mu", max(mus))


def test_onset_replay_under_generations():
    nx, ny, rule = GEN_LINES[1]
    for u, grid in enumerate(gen_soups(nx, ny, rule[2])):
        found = orbit(grid, 1023, rule, G.gen_step)
        hit, mu = onset_run(grid, 1023, rule, G.gen_step)
        assert (hit, mu) == want_of(found, 1023), (u, found)
        assert mu > 0
        if u < 3:  # the shortcut the GPU test takes to the final state
            np.testing.assert_array_equal(state_after(grid, 1023, found, rule, G.gen_step),
                                          G.gen_run(grid, 1023, rule))
