"""The whole batch plan without a GPU (life_batch_query_plan, csrc/life_plan.cpp
batch_plan): which kernel instance and launch a shape takes, against a
restatement of the contract that the refusal message spells out, and a guard
that holds the shape list of tests/test_gpu_batch_group.py to its coverage of
the group tier's instances."""
import ctypes

import pytest

from test_gpu_batch_group import CASES_A, CASES_B, CASES_C, GROUP_CASES

ROWS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 25, 32)  # the strip heights batch_group_kernel is compiled for
LANES = (1, 2, 4, 8, 16, 32, 64)
GROUP_THREADS, WAVE_THREADS = 1024, 256
LIFE_EINVAL = -1


def restated(nx, ny):
    """(tier, words, lanes per strip, R, strips, threads, bytes), None where refused."""
    if nx < 1 or ny < 1 or nx > 2048:
        return None
    words = -(-nx // 32)
    if nx <= 128 and ny <= 64:
        return "wave", words, 0, 0, 0, WAVE_THREADS, 4 * words * ny
    lanes = 1
    while lanes < words:
        lanes *= 2
    for rows in ROWS:
        if ny % rows == 0 and ny // rows <= GROUP_THREADS // lanes:
            strips = ny // rows
            return "group", words, lanes, rows, strips, 64 * -(-strips * lanes // 64), 4 * words * ny
    return None


def planned(lm, nx, ny):
    """The same of the library, by the C calls themselves."""
    lib = lm._lib()
    out = [ctypes.c_int() for _ in range(6)]
    nbytes, tier = ctypes.c_int64(), ctypes.c_int()
    rc = lib.life_batch_query_plan(nx, ny, *map(ctypes.byref, out))
    assert rc == lib.life_batch_query(nx, ny, ctypes.byref(tier), ctypes.byref(nbytes)), (nx, ny)
    if rc != 0:
        assert rc == LIFE_EINVAL, (nx, ny)
        return None
    assert tier.value == out[0].value, (nx, ny)
    return (lm.BATCH_TIERS[out[0].value],) + tuple(v.value for v in out[1:]) + (nbytes.value,)


def heights_swept(lanes):
    """Every ny in 1..1100, and R * k for k at and around the most strips a workgroup holds, for every R."""
    most = GROUP_THREADS // lanes
    edge = {rows * k for rows in ROWS for k in (most - 1, most, most + 1) if k >= 1}
    return sorted(set(range(1, 1101)) | edge)


@pytest.mark.parametrize("words", range(1, 65))
def test_plan_matches_its_contract(lm, words):
    lanes = next(v for v in LANES if v >= words)
    accepted = refused = 0
    for nx in (32 * (words - 1) + 1, 32 * words):  # the narrowest and the widest row of `words` words
        for ny in heights_swept(lanes):
            want = restated(nx, ny)
            assert planned(lm, nx, ny) == want, (nx, ny)
            accepted += want is not None
            refused += want is None
    assert accepted and refused  # 1031 is prime and beyond every width's strips: the sweep meets both


def test_sweep_reaches_every_instance():
    """The sweep itself runs through all 13 strip heights at all 7 widths."""
    seen = set()
    for words in range(1, 65):
        lanes = next(v for v in LANES if v >= words)
        for ny in heights_swept(lanes):
            want = restated(32 * words, ny)
            if want and want[0] == "group":
                seen.add((want[3], want[2]))
    assert seen == {(rows, lanes) for rows in ROWS for lanes in LANES}


REFUSED = [(0, 5), (5, 0), (-1, 5), (5, -1), (0, 0), (2049, 1), (2049, 16), (4096, 4096), (129, 131), (2048, 1031),
           (32, 1031 * 32 + 32), (1, 2**62), (2**62, 1)]  # the last two: refused before any product of the shape


@pytest.mark.parametrize("nx,ny", REFUSED)
def test_refusals_are_those_of_the_query(lm, nx, ny):
    assert restated(nx, ny) is None
    lib = lm._lib()
    with pytest.raises(lm.LifeError) as e:
        lm.batch_query(nx, ny)
    assert e.value.rc == LIFE_EINVAL
    why = lib.life_last_error().decode()
    assert why.startswith(f"batch of {nx} x {ny} universes: ")
    with pytest.raises(lm.LifeError):  # another refusal in between: the message below is the plan call's own
        lm.parse_rule("B9/S")
    assert lib.life_last_error().decode() != why
    out = [ctypes.c_int(-7) for _ in range(6)]
    assert lib.life_batch_query_plan(nx, ny, *map(ctypes.byref, out)) == LIFE_EINVAL
    assert lib.life_last_error().decode() == why
    assert [v.value for v in out] == [-7] * 6  # a refusal writes nothing
    with pytest.raises(lm.LifeError) as e:
        lm.batch_plan(nx, ny)
    assert e.value.rc == LIFE_EINVAL and why in str(e.value)


def test_binding_and_optional_out_pointers(lm):
    assert lm.batch_plan(33, 7) == ("wave", 2, 0, 0, 0, WAVE_THREADS)
    plan = lm.batch_plan(500, 500)
    assert plan == ("group", 16, 16, 10, 50, 832)
    assert (plan.tier, plan.words, plan.lanes_per_strip, plan.rows, plan.strips, plan.threads) == plan
    lib = lm._lib()
    assert lib.life_batch_query_plan(500, 500, None, None, None, None, None, None) == 0
    rows = ctypes.c_int()
    assert lib.life_batch_query_plan(500, 500, None, None, None, ctypes.byref(rows), None, None) == 0
    assert rows.value == 10


# ---- the coverage of the GPU shape list
# The instances the list has to run, as (R, lanes per strip, strips): R = 1, 2, 3 at every width (A), the other
# ten strip heights at 64 lanes (B), full workgroups and tall strips on narrow lane groups (C).
PINNED = {
    (1, 1, 65), (2, 1, 513), (3, 1, 343), (1, 2, 65), (2, 2, 257), (3, 2, 171), (1, 4, 65), (2, 4, 129), (3, 4, 87),
    (1, 8, 1), (2, 8, 65), (3, 8, 43), (1, 16, 1), (2, 16, 33), (3, 16, 23), (1, 32, 1), (2, 32, 17), (3, 32, 11),
    (1, 64, 1), (2, 64, 9), (3, 64, 7),
    (4, 64, 10), (5, 64, 5), (6, 64, 9), (8, 64, 11), (10, 64, 10), (12, 64, 9), (16, 64, 11), (20, 64, 10),
    (25, 64, 5), (32, 64, 9),
    (1, 1, 1024), (32, 64, 16), (25, 8, 27), (32, 1, 513), (16, 2, 257), (20, 16, 34), (25, 4, 53), (10, 16, 34),
    (12, 32, 17),
}


def coverage_gaps(lm, cases):
    """What `cases` leaves unrun, by the library's own plan of every shape (the columns a case states are not
    trusted here: the GPU test asserts them)."""
    plans = [(nx, lm.batch_plan(nx, ny)) for nx, ny, *_ in cases]
    assert all(p.tier == "group" for _, p in plans)
    gaps = []

    def need(ok, what):
        if not ok:
            gaps.append(what)

    for rows in ROWS:
        need(any(p.rows == rows for _, p in plans), f"R = {rows}")
    for lanes in LANES:
        need(any(p.lanes_per_strip == lanes for _, p in plans), f"{lanes} lanes per strip")
        for rows in (1, 2, 3):
            need(any((p.rows, p.lanes_per_strip) == (rows, lanes) for _, p in plans), f"R = {rows} at {lanes} lanes")
    need(any(p.strips == 1 for _, p in plans), "one strip per universe")
    used = lambda p: p.strips * p.lanes_per_strip  # noqa: E731
    need(any(used(p) == 1024 and p.rows == 1 for _, p in plans), "1024 used threads with R = 1")
    need(any(used(p) == 1024 and p.rows > 1 for _, p in plans), "1024 used threads with R > 1")
    need(any(used(p) % 64 and p.rows > 1 for _, p in plans), "a part-filled last wave with R > 1")
    full = {p.lanes_per_strip for nx, p in plans if p.words == p.lanes_per_strip and nx % 32 == 0}
    partial = {p.lanes_per_strip for nx, p in plans if p.words == p.lanes_per_strip and nx % 32}
    padded = {p.lanes_per_strip for _, p in plans if p.words < p.lanes_per_strip}
    need(len(full) >= 3, f"W == Wp with nx a multiple of 32 at three widths (has {sorted(full)})")
    need(len(partial) >= 3, f"W == Wp with a partial last word at three widths (has {sorted(partial)})")
    need(len(padded) >= 3, f"W < Wp at three widths (has {sorted(padded)})")
    for inst in sorted(PINNED - {(p.rows, p.lanes_per_strip, p.strips) for _, p in plans}):
        need(False, "the instance R = %d, %d lanes per strip, %d strips" % inst)
    return gaps


def test_gpu_shape_list_covers_the_group_tier(lm):
    assert len(GROUP_CASES) == len(set(GROUP_CASES)) == len(CASES_A) + len(CASES_B) + len(CASES_C)
    assert coverage_gaps(lm, GROUP_CASES) == []
    for nx, ny, rows, lanes, strips in GROUP_CASES:  # what a row states is what the plan gives
        plan = lm.batch_plan(nx, ny)
        assert (plan.rows, plan.lanes_per_strip, plan.strips) == (rows, lanes, strips), (nx, ny, plan)


def test_guard_misses_any_one_shape(lm):
    """The guard is not vacuous: the list without any one of its rows fails it."""
    for k, case in enumerate(GROUP_CASES):
        assert coverage_gaps(lm, GROUP_CASES[:k] + GROUP_CASES[k + 1:]), case
    # and each of the structural requirements alone, on a list that keeps every R and width
    without = lambda pred: [c for c in GROUP_CASES if not pred(c)]  # noqa: E731
    assert "one strip per universe" in coverage_gaps(lm, without(lambda c: c[4] == 1))
    assert "1024 used threads with R > 1" in coverage_gaps(lm, without(lambda c: c[:2] == (2048, 512)))
    assert "1024 used threads with R = 1" in coverage_gaps(lm, without(lambda c: c[:2] == (32, 1024)))
    assert "a part-filled last wave with R > 1" in coverage_gaps(
        lm, without(lambda c: c[2] > 1 and c[3] * c[4] % 64 != 0))
