"""The numpy reference of the Generations rules (include/life_mi355x.h,
life_rule_parse_gen), written from the contract and from nothing else: a cell
state s in [0, C), 0 dead, 1 alive, 2 .. C - 1 dying; n the number of the 8
Moore neighbours on the periodic torus whose state is exactly 1;
  s = 0: 1 if birth bit n is set, else 0
  s = 1: 1 if survive bit n is set, else 2 mod C
  s >= 2: (s + 1) mod C.
tests/test_gen_host.py pins it at C = 2 to rule_ref.rule_step and to two hand
anchors; the GPU tests lean on it."""
import numpy as np

MAX_STATES = 16
BRAIN = (0x04, 0x00, 3)  # B2/S/C3 Brian's Brain
STARWARS = (0x04, 0x38, 4)  # B2/S345/C4 Star Wars
_MASK64 = (1 << 64) - 1


def alive_neighbours(states: np.ndarray) -> np.ndarray:
    """Neighbours (of 8) in state 1 of every cell of a periodic (ny, nx) grid,
    or of every grid of a (..., ny, nx) stack."""
    a = (np.asarray(states) == 1).astype(np.uint8)
    total = np.zeros_like(a)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                total += np.roll(np.roll(a, dy, -2), dx, -1)
    return total


def gen_step(states: np.ndarray, birth: int, survive: int, c: int) -> np.ndarray:
    s = np.asarray(states).astype(np.int64)
    n = alive_neighbours(s).astype(np.int64)
    born = (birth >> n) & 1
    stays = (survive >> n) & 1
    out = np.where(s == 0, born, np.where(s == 1, np.where(stays == 1, 1, 2 % c), (s + 1) % c))
    return out.astype(np.uint8)


def gen_run(states: np.ndarray, gens: int, rule) -> np.ndarray:
    states = np.asarray(states, dtype=np.uint8)
    for _ in range(gens):
        states = gen_step(states, *rule)
    return states


def mixed_soup(nx: int, ny: int, c: int, seed: int) -> np.ndarray:
    """About 40 % alive, the rest uniform over 0 .. c - 1."""
    rng = np.random.default_rng(seed)
    rest = rng.integers(0, c, size=(ny, nx))
    return np.where(rng.random((ny, nx)) < 0.4, 1, rest).astype(np.uint8)


def classes(states: np.ndarray) -> set:
    """The (state class, alive neighbours) pairs that occur: class 0 dead, 1
    alive, 2 dying."""
    s = np.minimum(np.asarray(states), 2)
    return set(zip(s.ravel().tolist(), alive_neighbours(states).ravel().tolist()))


def all_classes(c: int) -> set:
    return {(k, n) for k in range(3 if c > 2 else 2) for n in range(9)}


def mix64(v: int) -> int:
    v = (v * 0x9E3779B97F4A7C15) & _MASK64
    return v ^ (v >> 29)


def census(states: np.ndarray):
    """(live, dying, checksum) of life_batch_census_gen for one (ny, nx) grid,
    in Python integers."""
    s = np.asarray(states)
    ny, nx = s.shape
    total = 0
    for y, x in zip(*np.nonzero(s)):
        total = (total + int(s[y, x]) * mix64(int(y) * nx + int(x) + 1)) & _MASK64
    return int((s == 1).sum()), int((s >= 2).sum()), total


def census_stack(stack: np.ndarray):
    """census of every grid of an (n, ny, nx) stack: int64, int64 and uint64
    arrays (uint64 arithmetic wraps modulo 2^64; test_gen_host.py pins it to
    census)."""
    s = np.asarray(stack)
    n, ny, nx = s.shape
    v = np.arange(1, nx * ny + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    weights = (v ^ (v >> np.uint64(29))).reshape(ny, nx)
    sums = (s.astype(np.uint64) * weights).reshape(n, -1).sum(axis=1, dtype=np.uint64)
    flat = s.reshape(n, -1)
    return (flat == 1).sum(axis=1).astype(np.int64), (flat >= 2).sum(axis=1).astype(np.int64), sums


def brain_ship(nx: int, ny: int, along_x: bool) -> np.ndarray:
    """Two alive cells with two dying cells behind them: under B2/S/C3 the
    pattern moves one cell per generation towards its alive side."""
    g = np.zeros((ny, nx), np.uint8)
    if along_x:
        g[2:4, 5] = 1
        g[2:4, 4] = 2
    else:
        g[5, 2:4] = 1
        g[4, 2:4] = 2
    return g
