#!/usr/bin/env python3
"""LIFE_OPT_SKIP_DEAD measured: blocking calls timed with the
host clock (step + sync), medians of `--reps` alternating on / off runs in one
process on one box, as scripts/sparse_io_rate.py times its calls.

  sparse   p46gun.cfg loaded by set_cells into size^2, step(960) with the
           option on (valid maps) and off, alternating: ms per pass, tiles
           run per pass; the map scan is reported on its own: a one-pass
           call right after the option is switched on (maps invalid) minus
           a one-pass call on valid maps
  dense    50 % soup at size^2, step(120) on and off: the overhead of the
           plan kernel, the map clear, the plain tile grid and the masks

One JSON line per part on stdout (and appended to --out).

  ab       five ABAB pairs of the default bench.py line, this tree's library
           against the parent commit's (LIFE_AB_PARENT_LIB, loaded through
           LIFE_MI355X_LIB), each run a fresh child process with its own
           time limit; the first failure stops the set.

usage: python profiles/skip_dead/measure.py sparse|dense|ab [--size N] [--reps K] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mpi-and-open-mp_amd"))


def timed_step(life, gens):
    t0 = time.perf_counter()
    life.step(gens)
    life.sync()
    return (time.perf_counter() - t0) * 1e3


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def part_sparse(lm, a):
    cells = lm.load_cfg_cells(os.path.join(ROOT, "tests", "golden", "cfg", "p46gun.cfg"))[4]
    gens, passes = 960, 80
    with lm.Life(a.size, a.size, small_grid=False) as life:
        life.clear()
        life.set_cells(cells)
        life.configure(lm.OPT_SKIP_DEAD, 1)
        first = timed_step(life, gens)  # pays the map scan (and the kernels' first launches)
        act = life.activity()
        on, off, scan1, warm1, run = [], [], [], [], []
        for _ in range(a.reps):
            life.configure(lm.OPT_SKIP_DEAD, 0)
            off.append(timed_step(life, gens))
            life.configure(lm.OPT_SKIP_DEAD, 1)
            scan1.append(timed_step(life, 12))  # one pass behind the scan (the option switched on: maps invalid)
            warm1.append(timed_step(life, 12))  # one pass on valid maps
            on.append(timed_step(life, gens))   # 80 passes on valid maps
            p, r, _, t = life.activity()
            run.append(r / p)
        live = life.live_count()
    m_on, m_off = statistics.median(on), statistics.median(off)
    emit(dict(part="sparse", size=a.size, generations=gens, passes=passes, live_cells_end=live,
              on_ms=round(m_on, 3), off_ms=round(m_off, 3), first_ms=round(first, 3),
              scan_ms=round(statistics.median(scan1) - statistics.median(warm1), 3),
              one_pass_ms=round(statistics.median(warm1), 4), on_ms_per_pass=round(m_on / passes, 5),
              off_ms_per_pass=round(m_off / passes, 5), speedup=round(m_off / m_on, 1),
              tiles_run_per_pass=[round(v, 1) for v in run], tiles_per_pass=t // p,
              first_call_activity=act, on_all=[round(v, 3) for v in on], off_all=[round(v, 3) for v in off],
              scan1_all=[round(v, 3) for v in scan1], warm1_all=[round(v, 3) for v in warm1]), a.out)


def part_dense(lm, a):
    gens, passes = 120, 10
    with lm.Life(a.size, a.size, small_grid=False) as life:
        life.fill_random(1, 0.5)
        life.configure(lm.OPT_SKIP_DEAD, 1)
        timed_step(life, gens)
        life.configure(lm.OPT_SKIP_DEAD, 0)
        timed_step(life, gens)  # warm-up of both forms
        on, off = [], []
        for _ in range(a.reps):
            life.configure(lm.OPT_SKIP_DEAD, 0)
            off.append(timed_step(life, gens))
            path_off = life.last_path()
            life.configure(lm.OPT_SKIP_DEAD, 1)
            timed_step(life, gens)  # rescans; the next call runs on valid maps
            on.append(timed_step(life, gens))
            act = life.activity()
    m_on, m_off = statistics.median(on), statistics.median(off)
    emit(dict(part="dense", size=a.size, generations=gens, passes=passes, off_path=path_off,
              on_ms_per_pass=round(m_on / passes, 4), off_ms_per_pass=round(m_off / passes, 4),
              overhead_pct=round(100.0 * (m_on / m_off - 1.0), 1), activity=act,
              on_all=[round(v, 2) for v in on], off_all=[round(v, 2) for v in off]), a.out)


def part_ab(a):
    parent = os.environ.get("LIFE_AB_PARENT_LIB", "")
    if not os.path.exists(parent):
        raise SystemExit("LIFE_AB_PARENT_LIB: the parent commit's liblife_mi355x.so")
    vals = {"parent": [], "this": []}
    for label, env in [("parent", {"LIFE_MI355X_LIB": parent}), ("this", {})] * a.reps:
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=dict(os.environ, **env),
                               capture_output=True, text=True, timeout=150, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"{label}: time limit, stopping", flush=True)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or len(lines) != 1:
            print(f"{label}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}", flush=True)
            return 1
        vals[label].append(json.loads(lines[0])["value"])
        print(f"{label:7s} {vals[label][-1]:10.3f} Gcell/s", flush=True)
    emit(dict(part="ab", parent=vals["parent"], this=vals["this"], parent_median=statistics.median(vals["parent"]),
              this_median=statistics.median(vals["this"]),
              ratio=round(statistics.median(vals["this"]) / statistics.median(vals["parent"]), 4)), a.out)
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("part", choices=["sparse", "dense", "ab"])
    p.add_argument("--size", type=int, default=65536)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = p.parse_args()
    if a.part == "ab":
        return part_ab(a)
    import life_mi355x as lm

    (part_sparse if a.part == "sparse" else part_dense)(lm, a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
