"""The numpy reference of the Life-like rules (the oracle knows B3/S23 only)
and the rule sets the rule tests share.  tests/test_rule_host.py pins
rule_run at B3/S23 to oracle.life_run; the GPU tests lean on it."""
import numpy as np

CONWAY = (1 << 3, (1 << 2) | (1 << 3))  # (birth, survive)
NAMED = {"B3/S23": CONWAY, "B36/S23": (0x48, 0x0C), "B3678/S34678": (0x1C8, 0x1D8), "B2/S": (0x04, 0x00),
         "B1357/S1357": (0xAA, 0xAA), "B3/S012345678": (0x08, 0x1FF)}  # Life, HighLife, Day & Night, Seeds,
#                                                                       Replicator, Life without death


def neighbours(grid: np.ndarray) -> np.ndarray:
    """Live neighbours (of 8) of every cell of a periodic (ny, nx) 0/1 grid."""
    g = grid.astype(np.uint8)
    h = g + np.roll(g, 1, 1) + np.roll(g, -1, 1)  # the 3 x 3 block, rows first, then minus the cell
    return h + np.roll(h, 1, 0) + np.roll(h, -1, 0) - g


def rule_step(grid: np.ndarray, birth: int, survive: int) -> np.ndarray:
    table = np.array([[(birth >> k) & 1 for k in range(9)], [(survive >> k) & 1 for k in range(9)]], np.uint8)
    return table.ravel()[grid.astype(np.uint8) * 9 + neighbours(grid)]


def rule_run(grid: np.ndarray, gens: int, rule) -> np.ndarray:
    for _ in range(gens):
        grid = rule_step(grid, *rule)
    return grid


PARITY = NAMED["B1357/S1357"]  # the next state is the XOR of the eight neighbours: linear over GF(2)


def parity_run(grid: np.ndarray, gens: int) -> np.ndarray:
    """`gens` generations of PARITY on a periodic grid of any size, without
    stepping.  One generation is the operator P = the XOR of the eight copies
    of the grid rolled by one cell; over GF(2) squaring is linear, so P^(2^k)
    is the XOR of the eight copies rolled by 2^k, and P^gens the product of
    those over the set bits k of gens.  np.roll wraps at any size, so this
    holds on widths and heights that are no powers of two (a roll by more than
    the size, or two rolls that meet, are still what iterated steps give).
    tests/test_light_cone_host.py pins it to rule_run."""
    g = np.array(grid, dtype=np.uint8)
    k = 1
    while k <= gens:
        if gens & k:
            h = g ^ np.roll(g, k, 1) ^ np.roll(g, -k, 1)  # the 3 x 3 block at spacing k, rows first, then
            g = h ^ np.roll(h, k, 0) ^ np.roll(h, -k, 0) ^ g  # minus the cell
        k <<= 1
    return g


def conway_flips():
    """B3/S23 with one of its 18 table bits flipped, B0 excluded: 17 rules."""
    out = [(CONWAY[0] ^ (1 << k), CONWAY[1]) for k in range(1, 9)]
    return out + [(CONWAY[0], CONWAY[1] ^ (1 << k)) for k in range(9)]


def coverage(grid: np.ndarray) -> set:
    """The (alive, neighbours) pairs that occur in the grid."""
    return set(zip(grid.ravel().tolist(), neighbours(grid).ravel().tolist()))


ALL_PAIRS = {(a, n) for a in (0, 1) for n in range(9)}


def soup(nx: int, ny: int, seed: int, density: float = 0.5) -> np.ndarray:
    return (np.random.default_rng(seed).random((ny, nx)) < density).astype(np.uint8)
