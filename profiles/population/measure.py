#!/usr/bin/env python3
"""What LIFE_OPT_POPULATION costs: wall time of step calls,
host clock around step(n) + sync(), one device per child process.

  measure.py [--out FILE] [--lib NAME=PATH ...] [--parent PATH]

Per shape (65536^2 and 16384 x 32768, bit, 50 % soup), in one process,
alternating A B A B ...:
  (a) step(n) with the option off            n = 32, 256, 1024
  (b) step(n) with the option on (and the trace read: population())
  (c) the host loop n x (step(1) + live_count())
then p46gun.cfg in 65536^2 under skip-dead, option off / on, and -- each
library in a process of its own (LIFE_MI355X_LIB), the processes alternating --
  --parent PATH     (a) on a build of the parent commit beside this build
  --lib NAME=PATH   (b) on builds with another stripe count or occupancy
                    (-DLIFE_POP_STRIPES=S, -DLIFE_POP_WPE=4)
Prints one JSON line per timing and a summary; --out also writes them there.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "mpi-and-open-mp_amd")
GUN = os.path.join(ROOT, "tests", "golden", "cfg", "p46gun.cfg")


def worker(args):
    sys.path.insert(0, PKG)
    import life_mi355x as lm

    has_pop = hasattr(lm._lib(), "life_dev_population")
    nx, ny = args.nx, args.ny

    def timed(life, n, mode):
        life.sync()
        t0 = time.perf_counter()
        if mode == "loop":
            for _ in range(n):
                life.step(1)
                life.live_count()
        else:
            life.step(n)
            life.sync()
        t1 = time.perf_counter()
        read = 0.0
        if mode == "on":
            trace = life.population()
            read = time.perf_counter() - t1
            assert trace.size == n and trace[-1] == life.live_count()
        print(json.dumps({"tag": args.tag, "what": args.what, "nx": nx, "ny": ny, "mode": mode, "gens": n,
                          "ms": 1e3 * (t1 - t0), "read_ms": 1e3 * read, "path": life.last_path()}), flush=True)

    def set_mode(life, mode):
        if has_pop:
            life.configure(lm.OPT_POPULATION, 1 if mode == "on" else 0)

    with lm.Life(nx, ny, kernel="bit", small_grid=False, skip_dead=args.what == "gun") as life:
        if args.what == "gun":
            _, _, _, _, cells = lm.load_cfg_cells(GUN)
            life.clear()
            life.set_cells(cells + (nx // 2, ny // 2))
        else:
            life.fill_random(7, 0.5)
        modes = args.modes.split(",")
        for mode in modes:  # warm-up: every kernel of the timed window, and the trace buffer at its largest
            if mode != "loop":
                set_mode(life, mode)
                life.step(max(args.gens))
            else:
                life.step(1)
                life.live_count()
        for n in args.gens:
            for _ in range(args.reps):
                for mode in modes:  # A B (C) A B (C) ...
                    if mode == "loop" and n > args.loop_max:
                        continue
                    set_mode(life, mode)
                    timed(life, n, mode)


def child(out, tag, what, nx, ny, modes, gens, reps, lib=None, loop_max=1024):
    env = dict(os.environ)
    if lib:
        env["LIFE_MI355X_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tag", tag, "--what", what, "--nx", str(nx), "--ny",
           str(ny), "--modes", modes, "--gens", *map(str, gens), "--reps", str(reps), "--loop-max", str(loop_max)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{tag}: worker failed ({r.returncode})\n{r.stdout}\n{r.stderr}")
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    for row in rows:
        out(json.dumps(row))
    return rows


def summarise(out, rows):
    keys = sorted({(r["tag"], r["what"], r["nx"], r["ny"], r["mode"], r["gens"]) for r in rows})
    med = {}
    out("# tag what shape mode gens: median ms [min .. max] over n runs (read_ms median)")
    for k in keys:
        ms = [r["ms"] for r in rows if (r["tag"], r["what"], r["nx"], r["ny"], r["mode"], r["gens"]) == k]
        rd = [r["read_ms"] for r in rows if (r["tag"], r["what"], r["nx"], r["ny"], r["mode"], r["gens"]) == k]
        med[k] = statistics.median(ms)
        out(f"# {k[0]:8s} {k[1]:5s} {k[2]}x{k[3]} {k[4]:4s} {k[5]:5d}: {med[k]:10.3f} [{min(ms):.3f} .. {max(ms):.3f}] "
            f"n={len(ms)} read {statistics.median(rd):.3f}")
    out("# ratios of medians")
    for (tag, what, nx, ny, mode, gens), v in sorted(med.items()):
        base = med.get((tag, what, nx, ny, "off", gens))
        if mode == "on" and base:
            out(f"# {tag} {what} {nx}x{ny} n={gens}: (b)/(a) = {v / base:.4f}")
        on = med.get((tag, what, nx, ny, "on", gens))
        if mode == "loop" and on:
            out(f"# {tag} {what} {nx}x{ny} n={gens}: (c)/(b) = {v / on:.2f}   (c)/(a) = {v / base:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--what", default="soup")
    ap.add_argument("--nx", type=int, default=65536)
    ap.add_argument("--ny", type=int, default=65536)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--gens", type=int, nargs="+", default=[32, 256, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-max", type=int, default=1024)
    ap.add_argument("--out")
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--parent")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    f = open(args.out, "w") if args.out else None

    def out(line):
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()

    rows = []
    for nx, ny in ((65536, 65536), (16384, 32768)):
        rows += child(out, "this", "soup", nx, ny, "off,on,loop", args.gens, args.reps, loop_max=args.loop_max)
    rows += child(out, "this", "gun", 65536, 65536, "off,on", [1024], 5)
    if args.parent:  # the plain step, parent build and this build, processes alternating
        for _ in range(2):
            rows += child(out, "parent", "soup", 65536, 65536, "off", [1024], 4, lib=args.parent)
            rows += child(out, "this-a", "soup", 65536, 65536, "off", [1024], 4)
    libs = [("S64", None)] + [tuple(v.split("=", 1)) for v in args.lib]
    if args.lib:
        for _ in range(2):
            for name, path in libs:
                rows += child(out, name, "soup", 65536, 65536, "off,on", [1024], 3, lib=path)
    summarise(out, rows)


if __name__ == "__main__":
    main()
