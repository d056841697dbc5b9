"""life::pipe_plan (csrc/life_plan.cpp), the schedule of pipelined passes
(LIFE_OPT_PIPELINE), checked on the CPU with a g++ harness linked against
life_plan.cpp alone, as tests/test_host_plan.py does.

A pass of nty tile rows is R launches of row regions; pass p launches region
(p + j) % R at position j, launch i = p R + j runs on stream i % S, and the
plan lists, per position, the earlier launches waited for by event.  Swept
over nty 1..400, R 3..8, B (tile rows per banded item) 1 / 2 / 4 / 16 and
1..R + 2 passes:

* regions: a partition of [0, nty) into R contiguous groups of at least 2
  tile rows, of nearly equal size, on multiples of B when every region can
  hold a whole band (nty // B >= R); no plan when nty < 2 R;
* waits: same-stream order plus the planned waits, closed transitively,
  order every launch (p, r) behind the launches of regions r - 1, r, r + 1 of
  pass p - 1;
* concurrency: two launches that order leaves free to run side by side never
  have one writing rows the other reads or writes -- row intervals of 168-row
  tiles with 12 ghost rows at each window end, the y axis periodic, the last
  tile row full or 5 rows short of a ghost depth (tile row 0's window then
  reaches two tile rows up).

The waits depend on R and S only, so the order is worked out once per (R, S,
passes) -- which pairs of (region, region, same / other buffer parity) may
overlap -- and every tile grid is checked against those pairs.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include "life_host.h"
// per plan one line: nty B R S planR aligned | ty[0..planR] | per position: nwait waits... record
int main(int argc, char **argv) {
    const int S = atoi(argv[1]);
    const long long Bs[4] = {1, 2, 4, 16};
    for (long long nty = 1; nty <= 400; nty++)
        for (int R = 3; R <= 8; R++)
            for (long long B : Bs) {
                const life::PipePlan p = life::pipe_plan(nty, B, R, S);
                printf("%lld %lld %d %d %d %d |", nty, B, R, S, p.R, (int)p.aligned);
                for (int r = 0; r <= p.R && p.R; r++) printf(" %lld", (long long)p.ty[r]);
                printf(" |");
                for (int j = 0; j < p.R; j++) {
                    printf(" %d", p.nwait[j]);
                    for (int w = 0; w < p.nwait[j]; w++) printf(" %d", p.wait[j][w]);
                    printf(" %d", (int)p.record[j]);
                }
                printf("\n");
            }
    // out of range: no plan
    printf("X %d %d %d %d\n", life::pipe_plan(100, 1, 2, 2).R, life::pipe_plan(100, 1, 17, 2).R,
           life::pipe_plan(100, 1, 4, 0).R, life::pipe_plan(100, 1, 4, 5).R);
    return 0;
}
"""

T, M = 168, 12  # owned rows per tile and ghost rows per window end at 12 generations per pass


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{S: [plan dict, ...]} for S = 1, 2, 3 streams."""
    d = tmp_path_factory.mktemp("pipe")
    (d / "h.cpp").write_text(HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    str(d / "h.cpp"), os.path.join(CSRC, "life_plan.cpp"), "-o", str(exe)], check=True)
    out = {}
    for S in (1, 2, 3):
        rows = []
        for ln in subprocess.run([str(exe), str(S)], capture_output=True, text=True, check=True).stdout.splitlines():
            if ln.startswith("X"):
                assert ln.split()[1:] == ["0", "0", "0", "0"], ln
                continue
            head, ty, waits = ln.split("|")
            nty, B, R, S_, planR, aligned = map(int, head.split())
            w = list(map(int, waits.split()))
            per, k = [], 0
            for _ in range(planR):
                n = w[k]
                per.append((tuple(w[k + 1:k + 1 + n]), bool(w[k + 1 + n])))
                k += n + 2
            assert k == len(w) and S_ == S
            rows.append(dict(nty=nty, B=B, R=R, planR=planR, aligned=bool(aligned), ty=list(map(int, ty.split())),
                             waits=tuple(per)))
        assert len(rows) == 400 * 6 * 4
        out[S] = rows
    return out


def test_regions(plans):
    for p in plans[2]:
        nty, B, R, ty = p["nty"], p["B"], p["R"], p["ty"]
        where = f"nty {nty} B {B} R {R}: {ty}"
        if nty < 2 * R:
            assert p["planR"] == 0, where
            continue
        assert p["planR"] == R and len(ty) == R + 1, where
        assert ty[0] == 0 and ty[-1] == nty, where
        sizes = [b - a for a, b in zip(ty, ty[1:])]
        assert min(sizes) >= 2, where
        banded = B > 1 and nty // B >= R  # every region can hold a whole banded item
        assert p["aligned"] == banded, where
        if banded:
            assert all(t % B == 0 for t in ty[:-1]), where
            assert max(sizes) - min(sizes) < 2 * B, where  # one band apart, plus the rows B does not divide
        else:
            assert max(sizes) - min(sizes) <= 1, where


def wait_patterns(plans, S):
    """{R: per-position (waits, record)}; the waits do not depend on the tile grid."""
    pat = {}
    for p in plans[S]:
        if p["planR"]:
            assert pat.setdefault(p["R"], p["waits"]) == p["waits"], p
    assert sorted(pat) == [3, 4, 5, 6, 7, 8]
    return pat


def order(R, S, passes, waits):
    """before[i] = bit set of the launches ordered before launch i (stream order and the planned
    waits, closed transitively); pass 0 starts behind the call's fence only."""
    before = []
    for i in range(passes * R):
        p, j = divmod(i, R)
        direct = [i - S] if i >= S else []
        if p > 0:
            for d in waits[j][0]:
                assert 1 <= d <= i and (i - d) % S != i % S, (R, S, i, d)  # an earlier launch of another stream
                assert waits[(i - d) % R][1], (R, S, i, d)               # which records its event
                direct.append(i - d)
        m = 0
        for q in direct:
            m |= before[q] | 1 << q
        before.append(m)
    return before


@pytest.mark.parametrize("S", [1, 2, 3])
def test_waits_cover_dependencies(plans, S):
    pat = wait_patterns(plans, S)
    for R, waits in pat.items():
        for passes in range(1, R + 3):
            before = order(R, S, passes, waits)
            for i in range(R, passes * R):
                p, j = divmod(i, R)
                r = (p + j) % R
                for dr in (-1, 0, 1):
                    q = (p - 1) * R + (r + dr - (p - 1)) % R  # region r + dr of pass p - 1
                    assert (q // R + q % R) % R == (r + dr) % R
                    assert before[i] >> q & 1, f"R {R} S {S} passes {passes}: launch {i} not behind {q}"
                if S == 1:
                    assert waits[j][0] == ()
    if S == 2:  # R = 4 on two streams: one wait, three launches back
        assert [w for w, _ in pat[4]] == [(3,), (3,), (3,), ()]


def free_pairs(R, S, passes, waits):
    """The (region a, region b, same buffer parity) of every two launches that may run side by side."""
    before = order(R, S, passes, waits)
    out = set()
    for i in range(passes * R):
        for q in range(i):
            if not before[i] >> q & 1:
                out.add(((q // R + q % R) % R, (i // R + i % R) % R, (i // R - q // R) % 2 == 0))
    return out


def segments(a, b, h):
    """The cyclic row interval [a, b) (b - a <= h) as pieces of [0, h)."""
    assert 0 < b - a <= h
    a %= h
    b = a + (b - a)
    return [(a, b)] if b <= h else [(a, h), (0, b - h)]


def meet(x, y):
    return any(a < d and c < b for a, b in x for c, d in y)


def test_no_concurrent_hazard(plans):
    pat = wait_patterns(plans, 2)
    free = {R: set().union(*(free_pairs(R, 2, passes, pat[R]) for passes in range(1, R + 3))) for R in pat}
    # the order leaves something to overlap: the next pass's first region beside this pass's last (R >= 4)
    assert all(free[R] for R in free) and all((R - 1, 1 % R, False) in free[R] for R in free if R >= 4)
    checked = 0
    for p in plans[2]:
        if not p["planR"]:
            continue
        R, ty, nty = p["R"], p["ty"], p["nty"]
        for last in (T, 5):  # the last tile row: full, or shorter than the ghost depth
            h = (nty - 1) * T + last
            own = [segments(ty[r] * T, min(ty[r + 1] * T, h), h) for r in range(R)]
            # the rows a region's stored cells depend on: its own and M ghost rows at each end, periodic
            win = [segments(ty[r] * T - M, min(ty[r + 1] * T, h) + M, h) for r in range(R)]
            for a, b, same in free[R]:
                where = f"nty {nty} B {p['B']} R {R} last {last}: regions {a}, {b} parity {same}"
                if same:  # both write the same buffer (and read the other)
                    assert not meet(own[a], own[b]), where
                else:  # each writes the buffer the other reads
                    assert not meet(own[a], win[b]) and not meet(own[b], win[a]), where
                checked += 1
    assert checked > 100000
