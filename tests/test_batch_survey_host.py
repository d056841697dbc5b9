"""Batch surveys, host side (no GPU): the new calls are in the
header and the binding, the leaf definition the device expands a universe's
masks with is the one life::rule_words uses, and the CPU replay of
LIFE_BATCH_OPT_CYCLE (Brent's algorithm as include/life_mi355x.h defines it,
which tests/test_gpu_batch_survey.py holds the GPU to) agrees with brute
force on the hand patterns."""
import os
import re

import numpy as np
import pytest

import rule_ref as R
from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")
NEW_CALLS = ("life_batch_set_rules", "life_batch_get_rules", "life_batch_cycles")


def brent_run(grid, n, rule, keep=()):
    """One step call of n generations with LIFE_BATCH_OPT_CYCLE on: (period,
    generation of the call at which it was found) or (0, -1), and the states
    after the generations in `keep`, every one of them by rule_step."""
    state, T, power, lam, hit, kept = grid, grid, 1, 0, (0, -1), {}
    for g in range(1, n + 1):
        state = R.rule_step(state, *rule)
        if g in keep:
            kept[g] = state
        if hit[0] == 0:
            lam += 1
            if np.array_equal(state, T):
                hit = (lam, g)
            elif lam == power:
                T, power, lam = state, 2 * power, 0
    return hit, kept


def brute_force(grid, n, rule):
    """(mu, lambda) of the orbit by storing every state up to n; None when no
    state repeats within n generations."""
    seen, state = {grid.tobytes(): 0}, grid
    for g in range(1, n + 1):
        state = R.rule_step(state, *rule)
        first = seen.setdefault(state.tobytes(), g)
        if first != g:
            return first, g - first
    return None


def brent_from(mu, lam, n):
    """Where Brent, restarted at generation 0, finds a cycle (mu, lambda): at
    c + lambda for the first checkpoint c = 2^k - 1 >= mu with c + 1 >= lambda."""
    c = 0
    while c < mu or c + 1 < lam:
        c = 2 * c + 1
    return (lam, c + lam) if c + lam <= n else (0, -1)


def hand_patterns():
    """The seven 32 x 32 universes of the GPU test, B3/S23."""
    g = np.zeros((7, 32, 32), np.uint8)
    g[1, 4:6, 4:6] = 1  # block
    g[2, 10, 9:12] = 1  # blinker
    g[3, 0, 1] = g[3, 1, 2] = g[3, 2, 0] = g[3, 2, 1] = g[3, 2, 2] = 1  # glider: period 4 x 32 on the torus
    g[4, 16, 11:21] = 1  # a row of ten: a phase of the pentadecathlon
    for a in (0, 5, 7, 12):  # pulsar
        for k in (2, 3, 4, 8, 9, 10):
            g[5, 8 + a, 8 + k] = g[5, 8 + k, 8 + a] = 1
    g[6] = R.soup(32, 32, 1, 0.5)
    return g


HAND_WANT = [(1, 1), (1, 1), (2, 3), (128, 255), (15, 30), (3, 6), (0, -1)]  # one step(700)


def test_header_and_binding_know_the_new_calls(lm):
    declared = declared_functions()
    for name in NEW_CALLS:
        assert name in declared and name in lm.ABI_SYMBOLS, name
        assert getattr(lm._lib(), name) is not None
    assert declared == sorted(lm.ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "life_mi355x.h")).read()
    assert re.search(r"#define LIFE_BATCH_OPT_CYCLE (\d+)", header).group(1) == str(lm.BATCH_OPT_CYCLE) == "3"
    assert re.search(r"#define LIFE_BATCH_OPT_SETTLE (\d+)", header).group(1) == str(lm.BATCH_OPT_SETTLE)
    assert not re.search(r"#define LIFE_BATCH_OPT_\w+ 2\b", header)  # option 2 stays unassigned


def test_one_leaf_definition_for_host_and_device():
    """life::rule_words (pinned by tests/test_rule_host.py) and the batch kernels
    both expand masks through life::rule_leaf of life_host.h, and nowhere else."""
    host = open(os.path.join(CSRC, "life_host.h")).read()
    plan = open(os.path.join(CSRC, "life_plan.cpp")).read()
    kernels = open(os.path.join(CSRC, "life_batch_kernels.hip")).read()
    assert re.search(r"LIFE_HOST_DEVICE inline RuleLeaf rule_leaf\(", host)
    words = plan[plan.index("life::rule_words(uint32_t birth"):]
    words = words[:words.index("\n}\n")]
    assert "rule_leaf(birth, survive, alive, s)" in words and ">>" not in words
    assert "rule_leaf(m.x, m.y, q / 5, q % 5)" in kernels
    assert kernels.count("rule_leaf(") == 1


@pytest.mark.parametrize("n", [700, 255, 254, 30, 29, 6, 5, 3, 2, 1])
def test_brent_replay_agrees_with_brute_force(n):
    for u, grid in enumerate(hand_patterns()):
        found = brute_force(grid, 1500, R.CONWAY)
        want = brent_from(*found, n) if found else (0, -1)
        hit, kept = brent_run(grid, n, R.CONWAY, keep=(n,))
        assert hit == want, (u, n, found)
        np.testing.assert_array_equal(kept[n], R.rule_run(grid, n, R.CONWAY))
        if n == 700:
            assert hit == HAND_WANT[u], u
            if hit[0]:  # the period is the minimal one
                assert found[1] == hit[0]


def test_brent_replay_under_other_rules():
    """A soup under HighLife and under Seeds: the replay still finds exactly
    what brute force predicts, or nothing where nothing repeats."""
    for rule, seed, density in ((R.NAMED["B36/S23"], 40, 0.2), (R.NAMED["B2/S"], 41, 0.5),
                                (R.NAMED["B3/S012345678"], 41, 0.5)):
        grid = R.soup(33, 7, seed, density)
        found = brute_force(grid, 1500, rule)
        want = brent_from(*found, 1500) if found else (0, -1)
        assert brent_run(grid, 1500, rule)[0] == want, rule
