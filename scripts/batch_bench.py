#!/usr/bin/env python3
"""Throughput of life_batch against the host loop it replaces (DESIGN.md §5.11,
profiles/batch/README.md).

Batch: LifeBatch.step(n) between two syncs, 50 % soups, settle off.  Baseline:
one Life(nx, ny) object per universe on the small-grid path, the same soups
(fill_random(seed + u)) and generations, one step(n) each and a sync of all at
the end, timed at a count small enough to finish in seconds and scaled per
universe.  Every timing is the median of --reps runs after one warm-up run of
the same shape; before timing, the first universes' checksums of both paths
are compared after the warm-up run.  One JSON line per row on stdout (and in
--out), a markdown table on stderr.

The survey lines, reported and not gated.  Per-universe
rules: 262144 universes of 64 x 64, 50 % soups, step(1024), HighLife for every
universe through set_rules against the same batch under the uniform
set_rule("B36/S23") -- the uniform table kernel is the yardstick, the
difference is the price of a rule per universe.  Cycle detection: the settle
line's batch (16384 soups of 32 x 32 at 35 %, step(4096)) with detection off,
settle on and cycle on, and the share of universes each detector found.

    python scripts/batch_bench.py --out profiles/batch/batch_bench.jsonl
The Generations lines, reported and not gated: 262144
universes of 64 x 64, 50 % soups (fill_random: nothing dying at the start),
step(1024) under Brian's Brain (one decay plane), Star Wars (two), a rule of 16
states (four) and, in the same run, uniform HighLife on the two-state table
kernel as the yardstick; then one line with a (rule, C) per universe, the four
rules in turn.

The population lines, reported and not gated: 64 x 64 and
128 x 64 at 16384 and 262144 universes and 500 x 500 at 4096, 50 % soups,
step(1024), each measured three ways in one process, alternating within every
repetition: (a) LIFE_BATCH_OPT_POPULATION off, (b) on, (c) the host loop the
option replaces, step(1) + live_counts() per generation on the batch of (a),
over --loop-gens generations and scaled to 1024 by 1024 / loop-gens (every
generation of the loop costs the same launches and readbacks).  Before any
timing the trace of (b) over loop-gens generations is compared with the counts
of (c).  read_s is life_batch_population of the whole trace, after the call.

The onset lines, reported and not gated, one beside the
cycle line and two more: 16384 soups of 32 x 32 at 35 % with step(4096) (the
cycle line's batch), 262144 soups of 64 x 64 at 50 % with step(1024), and the
same under Star Wars (B2/S345/C4).  Each measured two ways in one process,
alternating within every repetition: LIFE_BATCH_OPT_CYCLE alone, and with
LIFE_BATCH_OPT_ONSET beside it; the checksums and the cycle pairs of the two
are compared.  Under LIFE_MI355X_LIB with a build that predates the option the
lines hold the cycle-only figures alone (the A/B run against a parent build).

    python scripts/batch_bench.py --out profiles/batch/batch_bench.jsonl
    python scripts/batch_bench.py --only onset --out profiles/batch/onset_bench.jsonl
    python scripts/batch_bench.py --only survey --out profiles/batch/survey_bench.jsonl
    python scripts/batch_bench.py --only gen --out profiles/batch/gen_bench.jsonl
    python scripts/batch_bench.py --only population --out profiles/batch/population_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-and-open-mp_amd"))

import numpy as np  # noqa: E402

import life_mi355x as lm  # noqa: E402

ROWS = [((32, 32), (1024, 16384, 262144)), ((64, 64), (1024, 16384, 262144)), ((128, 64), (1024, 16384, 262144)),
        ((500, 500), (256, 4096))]
ONSET_ROWS = [((32, 32), 16384, 4096, 0.35, None), ((64, 64), 262144, 1024, 0.5, None),
              ((64, 64), 262144, 1024, 0.5, "B2/S345/C4")]  # shape, count, generations, density, rule
POPULATION_ROWS = [((64, 64), (16384, 262144)), ((128, 64), (16384, 262144)), ((500, 500), (4096,))]
SEED = 1234


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def batch_time(nx, ny, count, gens, reps, density=0.5, settle=False, rule=None, rules=None, cycle=False):
    """(median s, min s, max s, share of universes the detector found, checksums)
    of LifeBatch.step(gens); rules: one rule for every universe, through set_rules,
    or a list of rules taken in turn.  Checksums: over the whole state."""
    with lm.LifeBatch(nx, ny, count, settle=settle, rule=rule, cycle=cycle) as b:
        if isinstance(rules, (list, tuple)):
            triples = [lm.parse_rule_gen(r) for r in rules]
            b.set_rules([triples[u % len(triples)] for u in range(count)])
        elif rules is not None:
            b.set_rules([lm.parse_rule(rules)] * count)
        times = []
        for rep in range(reps + 1):  # the first is the warm-up
            b.fill_random(SEED, density)
            times.append(timed(lambda: b.step(gens), b.sync))
        share = float((b.settled() >= 0).mean()) if settle else float((b.cycles()[0] > 0).mean()) if cycle else 0.0
        sums = b.state_checksums() if (b.states > 2).any() else b.checksums()
    t = times[1:]
    return statistics.median(t), min(t), max(t), share, sums


def baseline_time(nx, ny, count, gens, reps, density=0.5):
    """The same for a host loop over `count` Life objects."""
    lives = [lm.Life(nx, ny) for _ in range(count)]
    try:
        def fill():
            for u, life in enumerate(lives):
                life.fill_random(SEED + u, density)

        def sync():
            for life in lives:
                life.sync()

        def run():
            for life in lives:
                life.step(gens)

        times = []
        for rep in range(reps + 1):
            fill()
            times.append(timed(run, sync))
        paths = {life.last_path() for life in lives}
        sums = [life.checksum() for life in lives]
    finally:
        for life in lives:
            life.close()
    t = times[1:]
    return statistics.median(t), min(t), max(t), sorted(paths), sums


def spread(times):
    return {"s": statistics.median(times), "min_s": min(times), "max_s": max(times)}


def population_row(nx, ny, count, gens, loop_gens, reps):
    """One population line: (a) option off, (b) option on, (c) the host loop, alternating."""
    with lm.LifeBatch(nx, ny, count) as off, lm.LifeBatch(nx, ny, count, population=True) as on:
        def loop():
            return np.stack([(off.step(1), off.live_counts())[1] for _ in range(loop_gens)], axis=1)

        # the traces of (b) and (c) first
        for b in (off, on):
            b.fill_random(SEED, 0.5)
        on.step(loop_gens)
        if not np.array_equal(on.population(), loop()):
            raise SystemExit(f"{nx}x{ny} x {count}: the trace and the host loop disagree")
        a_t, b_t, c_t, read_t = [], [], [], []
        for rep in range(reps + 1):  # the first is the warm-up
            off.fill_random(SEED, 0.5)
            a_t.append(timed(lambda: off.step(gens), off.sync))
            on.fill_random(SEED, 0.5)
            b_t.append(timed(lambda: on.step(gens), on.sync))
            read_t.append(timed(on.population, on.sync))
            off.fill_random(SEED, 0.5)
            c_t.append(timed(loop, off.sync))
        # the host loop ran last on the plain batch: the recording one to the same generation
        on.fill_random(SEED, 0.5)
        on.step(loop_gens)
        if list(off.checksums()) != list(on.checksums()):
            raise SystemExit(f"{nx}x{ny} x {count}: option on and off disagree")
    scale = gens / loop_gens
    a, b, c, read = (spread(t[1:]) for t in (a_t, b_t, c_t, read_t))
    row = {"population": True, "shape": [nx, ny], "count": count, "gens": gens, "tier": lm.batch_query(nx, ny)[0],
           "loop_gens": loop_gens, "loop_scale": scale}
    for name, t in (("off", a), ("on", b), ("read", read), ("loop", c)):
        row.update({f"{name}_{k}": v for k, v in t.items()})
    row.update({"loop_scaled_s": c["s"] * scale, "on_over_off": b["s"] / a["s"],
                "loop_over_on": c["s"] * scale / b["s"], "loop_over_on_and_read": c["s"] * scale / (b["s"] + read["s"]),
                "off_tcups": nx * ny * count * gens / a["s"] / 1e12, "on_tcups": nx * ny * count * gens / b["s"] / 1e12})
    return row


def onset_row(nx, ny, count, gens, density, rule, reps):
    """One onset line: cycle detection alone and with LIFE_BATCH_OPT_ONSET, alternating."""
    has = hasattr(lm._lib(), "life_batch_onsets")
    row = {"onset": True, "shape": [nx, ny], "count": count, "gens": gens, "density": density,
           "rule": rule or "B3/S23", "option_in_build": has}
    with lm.LifeBatch(nx, ny, count, rule=rule, cycle=True) as cyc:
        ons = lm.LifeBatch(nx, ny, count, rule=rule, cycle=True, onset=True) if has else None
        try:
            c_t, o_t = [], []
            for rep in range(reps + 1):  # the first is the warm-up
                cyc.fill_random(SEED, density)
                c_t.append(timed(lambda: cyc.step(gens), cyc.sync))
                if ons:
                    ons.fill_random(SEED, density)
                    o_t.append(timed(lambda: ons.step(gens), ons.sync))
            period = cyc.cycles()[0]
            row.update({f"cycle_{k}": v for k, v in spread(c_t[1:]).items()})
            row["cycle_share"] = float((period > 0).mean())
            if ons:
                sums = (lambda b: b.state_checksums() if (b.states > 2).any() else b.checksums())
                if list(sums(cyc)) != list(sums(ons)) or any((x != y).any() for x, y in zip(cyc.cycles(), ons.cycles())):
                    raise SystemExit(f"{nx}x{ny} x {count}: onset on and off disagree")
                onsets = ons.onsets()
                if ((onsets >= 0) != (period > 0)).any():
                    raise SystemExit(f"{nx}x{ny} x {count}: an onset without a period, or a period without an onset")
                row.update({f"onset_{k}": v for k, v in spread(o_t[1:]).items()})
                row.update({"onset_over_cycle": row["onset_s"] / row["cycle_s"],
                            "mean_onset": float(onsets[onsets >= 0].mean()), "max_onset": int(onsets.max())})
        finally:
            if ons:
                ons.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gens", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-count", type=int, default=32, help="Life objects of the baseline's host loop")
    ap.add_argument("--settle-gens", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the smallest count of every shape only")
    ap.add_argument("--loop-gens", type=int, default=32, help="generations of the population lines' host loop")
    ap.add_argument("--only", choices=("all", "table", "settle", "survey", "gen", "population", "onset"),
                    default="all",
                    help="the shape table, the settle line, the survey lines, the Generations lines, the "
                         "population lines or the onset lines alone")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    table = []
    for (nx, ny), counts in ROWS if a.only in ("all", "table") else []:
        k = min(a.baseline_count, counts[0])
        bt, bmin, bmax, paths, bsums = baseline_time(nx, ny, k, a.gens, a.reps)
        per_universe = bt / k
        for count in counts[:1] if a.quick else counts:
            t, tmin, tmax, _, sums = batch_time(nx, ny, count, a.gens, a.reps)
            if [int(s) for s in sums[:k]] != bsums:
                raise SystemExit(f"{nx}x{ny}: the batch and the host loop disagree after {a.gens} generations")
            updates = nx * ny * count * a.gens
            row = {"shape": [nx, ny], "count": count, "gens": a.gens, "tier": lm.batch_query(nx, ny)[0],
                   "batch_s": t, "batch_min_s": tmin, "batch_max_s": tmax, "baseline_count": k,
                   "baseline_s_per_universe": per_universe, "baseline_min_s": bmin / k, "baseline_max_s": bmax / k,
                   "baseline_paths": paths, "baseline_s_scaled": per_universe * count,
                   "ratio": per_universe * count / t, "tcups": updates / t / 1e12,
                   "baseline_tcups": nx * ny * a.gens / per_universe / 1e12}
            emit(row)
            table.append(row)
    # the settle option: reported, not gated
    nx, ny, count, density = 32, 32, 1024 if a.quick else 16384, 0.35
    if a.only in ("all", "settle", "survey"):
        off = batch_time(nx, ny, count, a.settle_gens, a.reps, density, settle=False)
        on = batch_time(nx, ny, count, a.settle_gens, a.reps, density, settle=True)
        if list(off[4]) != list(on[4]):
            raise SystemExit("settle on and off disagree")
    if a.only in ("all", "settle"):
        emit({"settle": True, "shape": [nx, ny], "count": count, "gens": a.settle_gens, "density": density,
              "off_s": off[0], "off_min_s": off[1], "off_max_s": off[2], "on_s": on[0], "on_min_s": on[1],
              "on_max_s": on[2], "speedup": off[0] / on[0], "settled_share": on[3]})
    if a.only in ("all", "survey"):
        # cycle detection beside settle, on the settle line's batch
        cyc = batch_time(nx, ny, count, a.settle_gens, a.reps, density, cycle=True)
        if list(off[4]) != list(cyc[4]):
            raise SystemExit("cycle detection on and off disagree")
        emit({"cycle": True, "shape": [nx, ny], "count": count, "gens": a.settle_gens, "density": density,
              "off_s": off[0], "off_min_s": off[1], "off_max_s": off[2], "settle_s": on[0], "settle_min_s": on[1],
              "settle_max_s": on[2], "settled_share": on[3], "cycle_s": cyc[0], "cycle_min_s": cyc[1],
              "cycle_max_s": cyc[2], "cycle_share": cyc[3], "settle_speedup": off[0] / on[0],
              "cycle_speedup": off[0] / cyc[0]})
    for (nx, ny), count, gens, density, rule in ONSET_ROWS if a.only in ("all", "survey", "onset") else []:
        # the onset option beside cycle detection (the first line: on the cycle line's batch)
        emit(onset_row(nx, ny, min(count, 1024) if a.quick else count, gens, density, rule, a.reps))
    if a.only in ("all", "survey"):
        # the price of a rule per universe: the uniform table kernel is the yardstick
        nx, ny, count, rule = 64, 64, 1024 if a.quick else 262144, "B36/S23"
        uni = batch_time(nx, ny, count, a.gens, a.reps, rule=rule)
        per = batch_time(nx, ny, count, a.gens, a.reps, rules=rule)
        if list(uni[4]) != list(per[4]):
            raise SystemExit("uniform and per-universe HighLife disagree")
        emit({"per_universe_rules": True, "shape": [nx, ny], "count": count, "gens": a.gens, "rule": rule,
              "uniform_s": uni[0], "uniform_min_s": uni[1], "uniform_max_s": uni[2], "per_universe_s": per[0],
              "per_universe_min_s": per[1], "per_universe_max_s": per[2], "per_universe_over_uniform": per[0] / uni[0],
              "uniform_tcups": nx * ny * count * a.gens / uni[0] / 1e12,
              "per_universe_tcups": nx * ny * count * a.gens / per[0] / 1e12})
    if a.only in ("all", "gen"):
        # Generations: the uniform two-state table kernel of the same run is the yardstick
        nx, ny, count = 64, 64, 1024 if a.quick else 262144
        updates = nx * ny * count * a.gens
        yard = batch_time(nx, ny, count, a.gens, a.reps, rule="B36/S23")
        emit({"generations": True, "shape": [nx, ny], "count": count, "gens": a.gens, "rule": "B36/S23", "planes": 0,
              "s": yard[0], "min_s": yard[1], "max_s": yard[2], "tcups": updates / yard[0] / 1e12,
              "over_highlife": 1.0})
        named = [("B2/S/C3", 1), ("B2/S345/C4", 2), ("B2/S345/C16", 4)]
        for rule, planes in named:
            t = batch_time(nx, ny, count, a.gens, a.reps, rule=rule)
            emit({"generations": True, "shape": [nx, ny], "count": count, "gens": a.gens, "rule": rule,
                  "planes": planes, "s": t[0], "min_s": t[1], "max_s": t[2], "tcups": updates / t[0] / 1e12,
                  "over_highlife": t[0] / yard[0]})
        mix = [r for r, _ in named] + ["B36/S23"]
        t = batch_time(nx, ny, count, a.gens, a.reps, rules=mix)
        emit({"generations": True, "shape": [nx, ny], "count": count, "gens": a.gens, "rule": "per universe",
              "rules": mix, "planes": 4, "s": t[0], "min_s": t[1], "max_s": t[2], "tcups": updates / t[0] / 1e12,
              "over_highlife": t[0] / yard[0]})
    for (nx, ny), counts in POPULATION_ROWS if a.only in ("all", "population") else []:
        for count in counts[:1] if a.quick else counts:
            emit(population_row(nx, ny, min(count, 1024) if a.quick else count, a.gens, min(a.loop_gens, a.gens),
                                a.reps))
    print("| shape | count | batch ms | host loop ms (scaled) | ratio | Tcell-updates/s |", file=sys.stderr)
    print("|---|---|---|---|---|---|", file=sys.stderr)
    for r in table:
        print(f"| {r['shape'][0]}x{r['shape'][1]} | {r['count']} | {1e3 * r['batch_s']:.3f} | "
              f"{1e3 * r['baseline_s_scaled']:.1f} | {r['ratio']:.0f} | {r['tcups']:.2f} |", file=sys.stderr)


if __name__ == "__main__":
    main()
