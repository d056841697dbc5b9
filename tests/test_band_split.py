"""The banded last tile column as up to two sub-columns (life::band_split and
the band-list planners, csrc/life_plan.cpp; CPU only).

A tile column that owns o < 62 pairs runs as sub-columns of G = 2^gsh lanes
(1 ghost + own <= G - 2 owned + ghost pairs, 2 <= gsh <= 5), 64 / G tile rows
per workgroup; band_split(o) picks the cut that takes the fewest lanes per
tile row.  Checked with a g++ harness:

* band_split(o), o = 1..62, against a brute-force search over every cut;
* tail_makespan2 / tail_plan with a band list against a heap simulation of
  the same list schedule, and the one-band forms as their special case;
* the items per pass of 65536^2 (1024 pairs: 16 whole columns + {30, 2}).
"""
import heapq
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "life_host.h"
static life::BandRows bands(char **v) {  // B0 B1 (0: absent)
    life::BandRows b;
    for (int i = 0; i < 2; i++)
        if (atoll(v[i]) > 0) b.B[b.n++] = atoll(v[i]);
    return b;
}
int main(int argc, char **argv) {
    if (!strcmp(argv[1], "split")) {  // every o: n then (first own gsh) per part, for max_parts 2 and 1
        for (int o = 1; o <= 62; o++)
            for (int parts = 2; parts >= 1; parts--) {
                const life::BandSplit s = life::band_split(o, parts);
                printf("%d %d %d", o, parts, s.n);
                for (int i = 0; i < s.n; i++) printf(" %d %d %d", s.b[i].first, s.b[i].own, s.b[i].gsh);
                printf("\n");
            }
        const life::BandSplit d = life::band_split(32);  // the default: two parts
        printf("default %d\n", d.n);
        return 0;
    }
    if (!strcmp(argv[1], "items")) {  // nfull B0 B1 rows
        printf("%lld\n", (long long)life::tail_row_items(atoll(argv[2]), bands(argv + 3), atoll(argv[5])));
        return 0;
    }
    if (!strcmp(argv[1], "span")) {  // nfull B0 B1 F n2 slots c
        printf("%.9f\n", life::tail_makespan2(atoll(argv[2]), bands(argv + 3), atoll(argv[5]), atoll(argv[6]),
                                              atoll(argv[7]), atof(argv[8])));
        return 0;
    }
    if (!strcmp(argv[1], "plan")) {  // nfull B0 B1 ty0 ty1 yend T T2 slots mode c
        const life::TailPlan p = life::tail_plan(atoll(argv[2]), bands(argv + 3), atoll(argv[5]), atoll(argv[6]),
                                                 atoll(argv[7]), atoll(argv[8]), atoll(argv[9]), atoll(argv[10]),
                                                 atoi(argv[11]), atof(argv[12]));
        printf("%lld %lld %.9f\n", (long long)p.F, (long long)p.n2, p.makespan);
        return 0;
    }
    if (!strcmp(argv[1], "oldplan")) {  // ntx B ty0 ty1 yend T T2 slots mode c
        const life::TailPlan p = life::tail_plan(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]),
                                                 atoll(argv[6]), atoll(argv[7]), atoll(argv[8]), atoll(argv[9]),
                                                 atoi(argv[10]), atof(argv[11]));
        printf("%lld %lld %.9f\n", (long long)p.F, (long long)p.n2, p.makespan);
        return 0;
    }
    if (!strcmp(argv[1], "pipe")) {  // nty B0 B1 R S
        const life::PipePlan p = life::pipe_plan(atoll(argv[2]), bands(argv + 3), atoi(argv[5]), atoi(argv[6]));
        const life::PipePlan q = life::pipe_plan(atoll(argv[2]), bands(argv + 3).largest(), atoi(argv[5]), atoi(argv[6]));
        printf("%d %d", p.R, (int)p.aligned);
        for (int r = 0; r <= p.R; r++) printf(" %lld", (long long)p.ty[r]);
        printf(" %d\n", (int)(p.R == q.R && !memcmp(p.ty, q.ty, sizeof p.ty) && !memcmp(p.wait, q.wait, sizeof p.wait)));
        return 0;
    }
    return 2;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("bands")
    (d / "h.cpp").write_text(HARNESS)
    out = d / "h"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    str(d / "h.cpp"), os.path.join(CSRC, "life_plan.cpp"), "-o", str(out)], check=True)
    return str(out)


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.split()


def lanes_of(own):
    """lanes of the smallest group that holds `own` owned pairs and two ghosts; None beyond 30"""
    for gsh in range(2, 6):
        if own <= (1 << gsh) - 2:
            return 1 << gsh
    return None


def brute(o):
    """(fewest lanes of one sub-column or None, fewest lanes of any two contiguous parts or None)"""
    pairs = [lanes_of(a) + lanes_of(o - a) for a in range(1, o) if lanes_of(a) and lanes_of(o - a)]
    return lanes_of(o), min(pairs) if pairs else None


@pytest.fixture(scope="module")
def splits(exe):
    out = subprocess.run([exe, "split"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[-1] == "default 2"
    got = {}
    for line in out[:-1]:
        v = list(map(int, line.split()))
        got[v[0], v[1]] = [tuple(v[3 + 3 * i:6 + 3 * i]) for i in range(v[2])]
    return got


@pytest.mark.parametrize("o", range(1, 63))
def test_band_split_is_the_brute_force_minimum(splits, o):
    parts = splits[o, 2]
    one, two = brute(o)
    best = min(x for x in (one, two, 64) if x is not None)
    if best >= 64:
        assert parts == []  # a whole tile
        assert o >= 45
    else:
        assert o <= 44
        assert sum(1 << g for _, _, g in parts) == best
        # contiguous and covering [0, o), every part inside its group's cap
        at = 0
        for first, own, gsh in parts:
            assert first == at and own >= 1 and 2 <= gsh <= 5 and own <= (1 << gsh) - 2
            at += own
        assert at == o
        # ties keep ONE sub-column, at the smallest group that holds o (the rule before the split)
        if one is not None and one == best:
            assert parts == [(0, o, one.bit_length() - 1)]
        else:
            assert len(parts) == 2
    # one part allowed: the rule before the split
    assert splits[o, 1] == ([(0, o, one.bit_length() - 1)] if one else [])


def test_band_split_known_columns(splits):
    assert splits[32, 2] == [(0, 30, 5), (30, 2, 2)]  # 65536 wide: 36 lanes instead of 64
    assert splits[16, 2] == [(0, 14, 4), (14, 2, 2)]  # 32768 wide: 20 instead of 32
    assert splits[8, 2] == [(0, 6, 3), (6, 2, 2)]     # 16384 wide: 12 instead of 16
    assert splits[2, 2] == [(0, 2, 2)] and splits[3, 2] == [(0, 3, 3)] and splits[30, 2] == [(0, 30, 5)]
    for o in range(31, 45):
        assert 36 <= sum(1 << g for _, _, g in splits[o, 2]) <= 48
    for o in range(45, 63):
        assert splits[o, 2] == []


def row_items(nfull, B, rows):
    return 0 if rows <= 0 else nfull * rows + sum(-(-rows // b) for b in B if b)


def heap_span(nfull, B, F, n2, slots, c):
    free, end = [0.0] * slots, 0.0
    for d, n in ((1.0, row_items(nfull, B, F)), (c + (1 - c) * 0.5, row_items(nfull, B, n2))):
        for _ in range(n):
            t = heapq.heappop(free) + d
            end = max(end, t)
            heapq.heappush(free, t)
    return end


# nfull, (B0, B1), full tile rows, half tile rows, slots; the first is the headline pass (65536^2, m = 12)
SPANS = [(16, (2, 16), 391, 0, 768), (16, (2, 16), 380, 22, 768), (4, (4, 16), 7, 2, 13), (0, (2, 16), 40, 9, 3),
         (8, (8, 16), 0, 11, 8), (1, (2, 4), 196, 37, 64), (8, (4, 16), 180, 36, 768)]


@pytest.mark.parametrize("nfull,B,F,n2,slots", SPANS)
@pytest.mark.parametrize("c", [0.0, 0.06, 0.2])
def test_band_list_schedule_is_the_list_schedule(exe, nfull, B, F, n2, slots, c):
    assert int(run(exe, "items", nfull, *B, F)[0]) == row_items(nfull, B, F)
    got = float(run(exe, "span", nfull, *B, F, n2, slots, c)[0])
    assert got == pytest.approx(heap_span(nfull, B, F, n2, slots, c), abs=1e-9)


@pytest.mark.parametrize("nfull,B,h,m", [(16, (2, 16), 65536, 12), (16, (2, 16), 65536, 10), (8, (4, 16), 65536, 12),
                                         (4, (8, 16), 32768, 12), (1, (2, 16), 84000, 12), (2, (2, 4), 9001, 5)])
def test_band_list_plan_covers_and_is_optimal(exe, nfull, B, h, m):
    slots, c, T, T2 = 768, 0.06, 192 - 2 * m, 96 - 2 * m
    nty = -(-h // T)
    F, n2, span = run(exe, "plan", nfull, *B, 0, nty, h, T, T2, slots, 2, c)
    F, n2, span = int(F), int(n2), float(span)
    assert 0 <= F <= nty
    if F < nty:
        rest = h - F * T
        assert n2 * T2 >= rest > (n2 - 1) * T2
    else:
        assert n2 == 0
    assert span == pytest.approx(heap_span(nfull, B, F, n2, slots, c), abs=1e-9)
    whole = heap_span(nfull, B, nty, 0, slots, c)
    assert span <= whole + 1e-9
    n = row_items(nfull, B, nty)
    if n > slots and n % slots:  # (an underfilled launch is left whole)
        best = min(heap_span(nfull, B, f, -(-(h - f * T) // T2), slots, c) for f in range(max(0, nty - 40), nty))
        assert span <= min(best, whole) + 1e-9


@pytest.mark.parametrize("ntx,B", [(17, 1), (9, 2), (5, 4), (2, 16), (1, 8)])
def test_one_band_forms_are_the_one_band_case(exe, ntx, B):
    nty, h, T, T2 = 171, 32768, 192, 72
    old = run(exe, "oldplan", ntx, B, 0, nty, h, T, T2, 768, 2, 0.06)
    new = run(exe, "plan", ntx - 1 if B > 1 else ntx, B if B > 1 else 0, 0, 0, nty, h, T, T2, 768, 2, 0.06)
    assert old == new


@pytest.mark.parametrize("m,want", [(12, 6477), (11, 6394), (10, 6327)])
def test_items_per_pass_of_the_headline_grid(exe, splits, m, want):
    """W = 1024 pairs, h = 65536: 16 whole tile columns and o = 32 as {30, 2} (2 and 16 tile rows per
    banded item); one band only: 17 whole columns."""
    W, h = 1024, 65536
    ntx = -(-W // 62)
    parts = splits[W - 62 * (ntx - 1), 2]
    B = [64 >> g for _, _, g in parts]
    assert B == [2, 16]
    nty = -(-h // (192 - 2 * m))
    assert int(run(exe, "items", ntx - 1, *B, nty)[0]) == want
    assert int(run(exe, "items", ntx, 0, 0, nty)[0]) == ntx * nty > want


@pytest.mark.parametrize("nty,B,R", [(391, (2, 16), 4), (66, (2, 16), 4), (9, (2, 16), 4), (100, (8, 4), 6)])
def test_pipelined_regions_align_on_the_largest_band(exe, nty, B, R):
    out = run(exe, "pipe", nty, *B, R, 2)
    big = max(B)
    assert int(out[-1]) == 1  # the plan of the largest band alone
    if nty < 2 * R:
        assert int(out[0]) == 0
        return
    ty = list(map(int, out[2:3 + R]))
    assert ty[0] == 0 and ty[-1] == nty and int(out[1]) == (1 if nty // big >= R else 0)
    if nty // big >= R:  # whole banded items of EVERY sub-column in every region: the pass's item count
        assert all(t % big == 0 for t in ty[:-1])
        assert sum(row_items(0, B, b - a) for a, b in zip(ty, ty[1:])) == row_items(0, B, nty)
