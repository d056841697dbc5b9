"""Generations rules without a GPU: the text forms
(life_rule_parse_gen / life_rule_format_gen) and the numpy reference the GPU
tests lean on (gen_ref.py), pinned to rule_ref at two states and to two
patterns worked by hand."""
import numpy as np
import pytest

import gen_ref as G
import rule_ref as R
from test_gpu_rule import TABLE_RULES

LIFE_EINVAL = -1


# ---- the text forms
@pytest.mark.parametrize("text,want", [
    ("B2/S/C3", (0x04, 0x00, 3)), ("b2/s345/c4", (0x04, 0x38, 4)), ("B2/S345/G4", (0x04, 0x38, 4)),
    ("B2/S345/g4", (0x04, 0x38, 4)), ("345/2/4", (0x04, 0x38, 4)), ("/2/3", (0x04, 0x00, 3)),
    ("B36/S23/C2", (0x48, 0x0C, 2)), ("B3/S23/C16", (0x08, 0x0C, 16)), ("23/3/16", (0x08, 0x0C, 16)),
    ("345/2/C4", (0x04, 0x38, 4)), ("B/S/C16", (0, 0, 16)), ("B3333/S2323/C10", (0x08, 0x0C, 10)),
])
def test_parse_gen(lm, text, want):
    assert lm.parse_rule_gen(text) == want


@pytest.mark.parametrize("text", ["B36/S23", "b3/s23", "23/3", "B2/S", "/", "B012345678/S012345678"])
def test_parse_gen_takes_what_parse_takes(lm, text):
    assert lm.parse_rule_gen(text) == lm.parse_rule(text) + (2,)


@pytest.mark.parametrize("text", [
    "B2/S/C1", "B2/S/C17", "B2/S/C0", "B2/S/C", "B2/S/", "B2/S/C3/C4", "B2/S/C3/", "B2/S/C3 ", "B2/S/C3x", "B2/S/C03",
    "B2/S/C100", "B2/S/CC3", "B2/S/-3", "B2/S/+3", "B2/S/D3", "345/2/", "345/2/4/5", "345/2/1", "345/2/17", "B9/S/C3",
    "B2/C3", "B2/S3x/C3", "C3", "", "B2S/C3", "S23/B3/C4",
])
def test_parse_gen_refusals(lm, text):
    with pytest.raises(lm.LifeError) as e:
        lm.parse_rule_gen(text)
    assert e.value.rc == LIFE_EINVAL
    assert f'"{text}"' in str(e.value)  # the message quotes the text


def test_parse_is_untouched(lm):
    for text in ("B2/S/C3", "345/2/4", "B3/S23/C2"):
        with pytest.raises(lm.LifeError) as e:
            lm.parse_rule(text)
        assert e.value.rc == LIFE_EINVAL
    with pytest.raises(lm.LifeError):
        lm.format_rule(1 << 9, 0)


def test_format_gen_round_trips(lm):
    rng = np.random.default_rng(5)
    for c in range(2, 17):
        for _ in range(8):
            b, s = int(rng.integers(0, 512)), int(rng.integers(0, 512))
            text = lm.format_rule_gen(b, s, c)
            assert lm.parse_rule_gen(text) == (b, s, c)
            assert text == lm.format_rule(b, s) + (f"/C{c}" if c > 2 else "")  # two states: exactly format_rule's
    assert lm.format_rule_gen(0x04, 0x38, 4) == "B2/S345/C4"
    assert lm.format_rule_gen(0x1FF, 0x1FF, 16) == "B012345678/S012345678/C16"
    assert lm.format_rule_gen(0, 0, 3) == "B/S/C3"
    for bad in ((1 << 9, 0, 3), (0, 1 << 9, 3), (4, 0, 1), (4, 0, 17), (4, 0, 0)):
        with pytest.raises(lm.LifeError) as e:
            lm.format_rule_gen(*bad)
        assert e.value.rc == LIFE_EINVAL


def test_life_refuses_a_generations_rule(lm):
    """Life runs two-state rules: the message says where Generations rules run."""
    with pytest.raises((lm.LifeError, ValueError)) as e:
        lm._rule_masks("B2/S/C3")
    assert "Generations" in str(e.value) and "LifeBatch" in str(e.value)
    with pytest.raises(lm.LifeError):  # what is no rule at all keeps life_rule_parse's message
        lm._rule_masks("B2/S/C99")


# ---- the reference
@pytest.mark.parametrize("rule", TABLE_RULES, ids=lambda r: f"B{r[0]:03x}S{r[1]:03x}")
def test_two_states_is_the_life_like_rule(rule):
    grid = R.soup(70, 41, 3)
    assert R.coverage(grid) == R.ALL_PAIRS
    for _ in range(4):
        want = R.rule_step(grid, *rule)
        np.testing.assert_array_equal(G.gen_step(grid, rule[0], rule[1], 2), want)
        grid = want


def test_census_at_two_states_is_the_oracle_checksum(oracle):
    grid = R.soup(37, 13, 11)
    live, dying, total = G.census(grid)
    assert (live, dying, total) == (int(grid.sum()), 0, int(oracle.checksum(grid)))
    stack = np.stack([G.mixed_soup(37, 13, 16, seed) for seed in range(3)])  # and the stack form is the same sums
    for k, got in enumerate(zip(*G.census_stack(stack))):
        assert tuple(int(v) for v in got) == G.census(stack[k])


@pytest.mark.parametrize("nx,ny,along_x", [(40, 7, True), (33, 9, False)])
def test_brain_ship_moves_one_cell_per_generation(nx, ny, along_x):
    start = G.brain_ship(nx, ny, along_x)
    state = start
    for g in range(1, (nx if along_x else ny) + 1):
        state = G.gen_step(state, *G.BRAIN)
        np.testing.assert_array_equal(state, np.roll(start, g, 1 if along_x else 0), err_msg=f"generation {g}")
    np.testing.assert_array_equal(state, start)  # once round the torus


def test_a_lone_cell_walks_through_every_dying_state():
    state = np.zeros((5, 33), np.uint8)
    state[2, 17] = 1
    for g in range(1, 15):
        state = G.gen_step(state, 0, 0, 16)
        assert state[2, 17] == g + 1 and int((state != 0).sum()) == 1, g
    state = G.gen_step(state, 0, 0, 16)
    assert not state.any()  # dead at generation 15


def test_the_soups_hold_what_the_gpu_tests_need():
    for c in (2, 3, 4, 5, 9, 16):
        soup = G.mixed_soup(128, 64, c, 1)
        assert set(np.unique(soup).tolist()) == set(range(c))
        # 40 % alive outright, and one in c of the rest (8192 cells: three sigma is 0.016)
        assert abs((soup == 1).mean() - (0.4 + 0.6 / c)) < 0.02, c
