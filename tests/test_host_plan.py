"""Host-only planning arithmetic of the runtime (csrc/life_plan.cpp), checked
on the CPU: a small C++ harness is linked against life_plan.cpp alone with
g++ (no HIP) and prints the plans.

* life::gather_plan -- the rank-mode fan-in of life_collect
  (6-cartesian/life_cart.c:281-305, 5-gather/life_mpi.c:177-179): which
  rank's block arrives in which staging slot and where it lands in the
  frame.  For world 1..8 and every partition shape, every rank appears once,
  the two receive slots alternate and hold the largest block, and placing the
  pieces (OR-ing the shared LIFEBITS bytes) rebuilds the frame exactly.
* life::flow_chunk_passes -- the dataflow launch's 32-bit queue head never
  wraps: passes x tiles + resident workgroups stays within 2^31.
* life::next_pass -- which passes a step call of the temporal tiles runs and
  which of them exchange (every rank must compute this identically): driven
  as step_body drives it, over call sequences and every single call.
* life::halo_match_send / halo_wait_peers / halo_op_slot -- the LOCAL
  transport's pairing of receives with the peers' sends, resolved once per
  halo plan.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "life_host.h"
int main(int argc, char **argv) {
    if (!strcmp(argv[1], "chunk")) {
        printf("%lld\n", (long long)life::flow_chunk_passes(atoll(argv[2]), atoll(argv[3]), atoll(argv[4])));
        return 0;
    }
    if (!strcmp(argv[1], "pass")) {
        // pass K bmax since (deep generations)...: the passes of each call, driven as step_body drives
        // them; one line per pass: call m refill_first extend ext since_before since_after
        const int K = atoi(argv[2]), bmax = atoi(argv[3]);
        int since = atoi(argv[4]);
        auto drive = [&](int call, bool deep, long long gens) {
            for (long long g = 0; g < gens;) {
                const life::PassPlan p = life::next_pass(K, bmax, deep, since, gens - g);
                const int before = since;
                if (p.m < 1) exit(2);  // no progress
                if (p.refill_first) since = 0;
                since = p.extend ? since + p.m : 0;  // every other pass ends with the exchange
                printf("%d %d %d %d %d %d %d\n", call, p.m, (int)p.refill_first, (int)p.extend, p.ext, before, since);
                g += p.m;
            }
        };
        if (argc == 7 && !strcmp(argv[5], "sweep")) {
            // every single call of 1..100 generations from every count 0..K: call = since0 * 100 + generations - 1
            for (int since0 = 0; since0 <= K; since0++)
                for (int gens = 1; gens <= 100; gens++) {
                    since = since0;
                    drive(since0 * 100 + gens - 1, atoi(argv[6]) != 0, gens);
                }
            return 0;
        }
        for (int a = 5, call = 0; a + 1 < argc; a += 2, ++call) drive(call, atoi(argv[a]) != 0, atoll(argv[a + 1]));
        return 0;
    }
    const long long nx = atoll(argv[2]), ny = atoll(argv[3]);
    const int d0 = atoi(argv[4]), d1 = atoi(argv[5]), kernel = atoi(argv[6]), fmt = atoi(argv[7]);
    if (!strcmp(argv[1], "match")) {
        // match nx ny d0 d1 kernel loop: per rank "R rank nops", its ops "O phase kind peer what index
        // width first count slot match" (match: the peer's send index of a receive, else -2), and
        // its wait lists "W phase kind peers..."
        const int world = d0 * d1, loop = fmt;
        life_halo_op ops[8][16];
        int n[8];
        for (int r = 0; r < world; r++)
            if ((n[r] = life::halo_plan(nx, ny, d0, d1, r, kernel, loop, ops[r], 16)) < 0) return 3;
        for (int r = 0; r < world; r++) {
            printf("R %d %d\n", r, n[r]);
            for (int i = 0; i < n[r]; i++) {
                const life_halo_op &o = ops[r][i];
                const int m = o.kind == LIFE_HALO_RECV
                                  ? life::halo_match_send(ops[r], i, r, ops[o.peer], n[o.peer]) : -2;
                printf("O %d %d %d %d %lld %lld %lld %lld %d %d\n", o.phase, o.kind, o.peer, o.what, (long long)o.index,
                       (long long)o.width, (long long)o.first, (long long)o.count, life::halo_op_slot(ops[r], i), m);
            }
            for (int phase = 0; phase < 2; phase++)
                for (int kind = 0; kind < 2; kind++) {
                    int peers[16];
                    const int np = life::halo_wait_peers(ops[r], n[r], r, phase, kind, peers);
                    printf("W %d %d", phase, kind);
                    for (int k = 0; k < np; k++) printf(" %d", peers[k]);
                    printf("\n");
                }
        }
        return 0;
    }
    life::GatherPiece p[64];
    int64_t slot = 0;
    const int n = life::gather_plan(nx, ny, d0, d1, kernel, fmt, p, 64, &slot);
    printf("%d %lld %lld\n", n, (long long)slot, (long long)life::gather_frame_row_bytes(nx, fmt));
    for (int k = 0; k < n; k++)
        printf("%d %d %lld %lld %lld %lld %d %d\n", p[k].rank, p[k].slot, (long long)p[k].bytes,
               (long long)p[k].row_bytes, (long long)p[k].rows, (long long)p[k].dst, p[k].shared_first,
               p[k].shared_last);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    (d / "h.cpp").write_text(HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    str(d / "h.cpp"), os.path.join(CSRC, "life_plan.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.split("\n")


def gather_plan(exe, nx, ny, d0, d1, kernel, fmt):
    lines = run(exe, "gather", nx, ny, d0, d1, kernel, fmt)
    n, slot, frb = map(int, lines[0].split())
    pieces = [tuple(map(int, ln.split())) for ln in lines[1:1 + n]]
    return n, slot, frb, pieces


SHAPES = [(64, 48), (1000, 37), (257, 131), (4096, 1024), (13, 9), (8192, 100)]


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["dense", "vtk", "bits"])
@pytest.mark.parametrize("world", [1, 2, 3, 4, 5, 6, 7, 8])
def test_gather_plan_rebuilds_frame(plan_exe, lm, world, fmt):
    for nx, ny in SHAPES:
        for policy in ("cart", "rows", "cols"):
            try:
                d0, d1 = lm.dims_choose(nx, ny, world, policy)
            except RuntimeError:
                continue  # a shape with empty blocks
            n, slot, frb, pieces = gather_plan(plan_exe, nx, ny, d0, d1, 1, fmt)
            assert n == world
            root = world - 1
            assert pieces[0][0] == root and pieces[0][1] == -1  # the root's own block first
            assert [p[0] for p in pieces[1:]] == list(range(world - 1))  # fan-in in rank order
            assert [p[1] for p in pieces[1:]] == [k % 2 for k in range(world - 1)]  # alternating slots
            assert slot == max(p[2] for p in pieces)
            # rebuild the frame from per-rank exports of a known grid
            rng = np.random.default_rng(nx * 131 + ny + world)
            grid = (rng.random((ny, nx)) < 0.5).astype(np.uint8)
            if fmt == 0:
                want = grid.reshape(-1)
            elif fmt == 1:
                want = np.stack([grid + ord("0"), np.full_like(grid, ord("\n"))], axis=2).reshape(-1)
            else:
                want = np.packbits(grid, axis=1, bitorder="little").reshape(-1)
            frame = np.full(ny * frb, 0xAA, dtype=np.uint8)
            for p in pieces:
                if p[6]:
                    frame[p[5] + np.arange(p[4]) * frb] = 0  # shared first bytes start at 0
            for rank, _slot, nbytes, rb, rows, dst, sf, sl in pieces:
                L = lm.layout_query(nx, ny, (d0, d1), rank, "bit")
                blk = grid[L.y0:L.y0 + L.h, L.x0:L.x0 + L.w]
                if fmt == 0:
                    exp = blk
                elif fmt == 1:
                    exp = np.stack([blk + ord("0"), np.full_like(blk, ord("\n"))], axis=2).reshape(L.h, -1)
                else:  # the bits kernel: block cells from bit x0 & 7 of the first byte
                    s = L.x0 & 7
                    pad = np.zeros((L.h, s + L.w), dtype=np.uint8)
                    pad[:, s:] = blk
                    exp = np.packbits(pad, axis=1, bitorder="little")
                assert exp.shape == (rows, rb) and nbytes == rows * rb
                for y in range(rows):
                    o = dst + y * frb
                    row = exp[y]
                    a, b = (1 if sf else 0), (rb - 1 if sl else rb)
                    frame[o + a:o + b] = row[a:b]
                    if sf:
                        frame[o] |= row[0]
                    if sl and (rb > 1 or not sf):
                        frame[o + rb - 1] |= row[rb - 1]
            np.testing.assert_array_equal(frame, want, err_msg=f"{nx}x{ny} dims {d0}x{d1} fmt {fmt}")


def test_gather_plan_rejects(plan_exe):
    assert run(plan_exe, "gather", 64, 64, 2, 2, 1, 3)[0].split()[0] == "-1"  # unknown format


@pytest.mark.parametrize("tiles,grid", [(1, 0), (6494, 768), (34 * 191, 768), (1 << 20, 1024), (3, 5),
                                        ((1 << 31) - 10, 768), ((1 << 31) + 1, 1)])
def test_flow_chunk_passes(plan_exe, tiles, grid):
    limit = 1 << 31
    n = int(run(plan_exe, "chunk", tiles, grid, 0)[0])
    if tiles + grid > limit:
        assert n == 0
        return
    assert n >= 1 and n * tiles + grid <= limit < (n + 1) * tiles + grid
    # a cap below the bound wins; a cap above it does not
    assert int(run(plan_exe, "chunk", tiles, grid, 3)[0]) == min(3, n)
    assert int(run(plan_exe, "chunk", tiles, grid, n + 5)[0]) == n


# ---- life::next_pass

def passes(exe, K, bmax, since, calls):
    """Drives next_pass over `calls` = [(deep, generations), ...] from the deep-halo count `since`.
    Returns per call its passes as dicts."""
    flat = [v for deep, g in calls for v in (int(deep), g)]
    return parse_passes(run(exe, "pass", K, bmax, since, *flat), len(calls))


def parse_passes(lines, ncalls):
    out = [[] for _ in range(ncalls)]
    for ln in lines:
        if ln:
            call, m, refill, extend, ext, before, after = map(int, ln.split())
            out[call].append(dict(m=m, refill=bool(refill), extend=bool(extend), ext=ext, before=before, after=after))
    return out


def check_calls(K, bmax, calls, got):
    for (deep, gens), ps in zip(calls, got):
        where = f"K {K} bmax {bmax} deep {deep} generations {gens}: {ps}"
        assert sum(p["m"] for p in ps) == gens, where
        segment = []  # pass lengths since the last exchange boundary
        for p in ps:
            since = 0 if p["refill"] else p["before"]
            assert 1 <= p["m"] <= bmax, where
            assert p["refill"] == (p["before"] + p["m"] > K), where
            assert since + p["m"] <= K, where
            assert p["ext"] == K - since - p["m"], where
            if p["extend"]:
                assert deep and since + p["m"] < K and p["ext"] >= 1, where
            assert p["after"] == (since + p["m"] if p["extend"] else 0), where
            # equal passes within one K segment.  A pass that refills first was sized against the
            # uncut rest of the call (the count had reached K, or the deep halo is off), not against
            # the K - since generations its successors are cut to: a segment of its own
            if p["refill"]:
                segment = []
            segment.append(p["m"])
            assert max(segment) - min(segment) <= 1, where
            if not p["extend"] or p["refill"]:
                segment = []
        if not deep:  # no K boundary cuts the call: all its passes are equal
            assert max(p["m"] for p in ps) - min(p["m"] for p in ps) <= 1, where
        if deep:  # the next call's first pass fits the aprons, or they were refilled
            assert ps[-1]["after"] == 0 or ps[-1]["after"] + bmax <= K, where


# the step calls of test_deep_halo: (deep, generations, bmax)
DEEP_HALO_CALLS = [(1, 5, 12), (1, 20, 12), (1, 7, 12), (1, 31, 32), (1, 12, 12), (0, 9, 12), (0, 33, 12), (1, 1, 12),
                   (1, 24, 12)]


@pytest.mark.parametrize("K", [32, 1])
def test_next_pass_call_sequence(plan_exe, K):
    """test_deep_halo's sequence of calls, the block size changing between them (so one harness run
    per call, the deep-halo count carried over), and the same sequence at every fixed block size."""
    since = 0
    for deep, gens, bmax in DEEP_HALO_CALLS:
        bmax = min(bmax, K)
        got = passes(plan_exe, K, bmax, since, [(deep, gens)])
        check_calls(K, bmax, [(deep, gens)], got)
        since = got[0][-1]["after"]
    for bmax in (5, 10, 12, 16, 32):
        bmax = min(bmax, K)
        for flip in (0, 1):  # as recorded, and with deep on / off swapped
            calls = [(deep ^ flip, gens) for deep, gens, _ in DEEP_HALO_CALLS]
            check_calls(K, bmax, calls, passes(plan_exe, K, bmax, 0, calls))


@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("bmax", [5, 10, 12, 16, 32])
@pytest.mark.parametrize("K", [32, 1])
def test_next_pass_every_single_call(plan_exe, K, bmax, deep):
    bmax = min(bmax, K)
    calls = [(deep, gens) for _since in range(K + 1) for gens in range(1, 101)]
    got = parse_passes(run(plan_exe, "pass", K, bmax, 0, "sweep", deep), len(calls))
    for since in range(K + 1):
        assert all(ps[0]["before"] == since for ps in got[since * 100:since * 100 + 100])
    check_calls(K, bmax, calls, got)


def exchanges(ps):
    return sum(p["refill"] + (not p["extend"]) for p in ps)


def test_next_pass_pinned(plan_exe):
    def ms(ps):
        return [(p["m"], p["extend"]) for p in ps]
    # K 32, at most 12 per pass: 20 generations are 10 (extend) + 10 (exchange) -- behind a
    # 5-generation call, as the benchmark's warm-up leaves it: the next call's first pass of up to 12
    # would not fit behind 25.  From freshly filled aprons neither pass exchanges (20 + 12 <= 32).
    assert ms(passes(plan_exe, 32, 12, 5, [(1, 20)])[0]) == [(10, True), (10, False)]
    assert ms(passes(plan_exe, 32, 12, 0, [(1, 20)])[0]) == [(10, True), (10, True)]
    # 32 generations are 11 + 11 + 10 with one exchange, on the last
    assert ms(passes(plan_exe, 32, 12, 0, [(1, 32)])[0]) == [(11, True), (11, True), (10, False)]
    # calls of 5 then 20: one exchange with the deep halo, three without
    # (the counts test_deep_halo_exchange_count asserts on the device)
    assert sum(map(exchanges, passes(plan_exe, 32, 12, 0, [(1, 5), (1, 20)]))) == 1
    assert sum(map(exchanges, passes(plan_exe, 32, 12, 0, [(0, 5), (0, 20)]))) == 3
    # at most 5 per pass: 20 generations are 4 x 5 with no exchange
    assert ms(passes(plan_exe, 32, 5, 0, [(1, 20)])[0]) == [(5, True)] * 4
    # a pass the aprons no longer cover refills first: the deep halo switched off at since = 30
    p = passes(plan_exe, 32, 12, 30, [(0, 9)])[0][0]
    assert p["before"] + p["m"] > 32 and p["refill"] and not p["extend"] and p["after"] == 0


# ---- the LOCAL transport's send / receive matcher

SEND, RECV, FILL = 0, 1, 2


def halo_match(exe, nx, ny, d0, d1, kernel, loop):
    ranks, waits = {}, {}
    for ln in run(exe, "match", nx, ny, d0, d1, kernel, loop):
        f = ln.split()
        if not f:
            continue
        if f[0] == "R":
            r = int(f[1])
            ranks[r], waits[r] = [], {}
        elif f[0] == "O":
            phase, kind, peer, what, index, width, first, count, slot, match = map(int, f[1:])
            ranks[r].append(dict(phase=phase, kind=kind, peer=peer, what=what, width=width, count=count, slot=slot,
                                 match=match))
        else:
            waits[r][(int(f[1]), int(f[2]))] = list(map(int, f[3:]))
    return ranks, waits


def check_match(ranks, waits, where):
    used = {r: [] for r in ranks}  # per rank: its sends that a receive paired with
    for r, ops in ranks.items():
        for i, o in enumerate(ops):
            # the staging slot: earlier ops of the phase with the same kind and what
            assert o["slot"] == sum(q["phase"] == o["phase"] and q["kind"] == o["kind"] and q["what"] == o["what"]
                                    for q in ops[:i]), where
            if o["kind"] != RECV:
                continue
            assert o["match"] >= 0, f"{where}: rank {r} receive {i} has no send"
            q = ranks[o["peer"]][o["match"]]
            assert q["kind"] == SEND and q["peer"] == r and q["phase"] == o["phase"], where
            assert (q["what"], q["count"], q["width"]) == (o["what"], o["count"], o["width"]), where
            used[o["peer"]].append(o["match"])
    for r, ops in ranks.items():  # every send is paired exactly once
        assert sorted(used[r]) == [i for i, o in enumerate(ops) if o["kind"] == SEND], where
    for r, ops in ranks.items():
        for (phase, kind), peers in waits[r].items():
            want = {o["peer"] for o in ops if o["phase"] == phase and o["kind"] == kind and o["peer"] != r}
            assert len(peers) == len(set(peers)) and set(peers) == want, where


@pytest.mark.parametrize("kernel", [0, 1], ids=["byte", "bit"])
@pytest.mark.parametrize("world", [1, 2, 3, 4, 5, 6, 7, 8])
def test_halo_match(plan_exe, lm, world, kernel):
    done = 0
    for nx, ny in SHAPES:
        for d0 in range(1, world + 1):
            if world % d0:
                continue
            d1 = world // d0
            if nx < d0 or ny < d1:
                continue  # a shape with empty blocks
            for loop in ((0, 1, 2, 3) if world == 1 else (0,)):
                where = f"{nx}x{ny} dims {d0}x{d1} kernel {kernel} loop {loop}"
                ranks, waits = halo_match(plan_exe, nx, ny, d0, d1, kernel, loop)
                assert sorted(ranks) == list(range(world)), where
                check_match(ranks, waits, where)
                done += 1
    assert done >= len(SHAPES)
