"""Throughput of the bit tiles under a Life-like rule (life_dev_set_rule): generations 32..1024 of a
50 % soup, as bench.py times B3/S23 -- one untimed call of 32 generations, then 992 timed by the
host clock around step + sync.  bench.py itself stays the B3/S23 yardstick.  Every run is a fresh
child process with its own time limit; the first failure stops the set.

usage: python profiles/rule/rate.py OUT.jsonl [RUNS]      (results: *.jsonl and README.md beside this file)
       python profiles/rule/rate.py --one RULE NX NY      (one measurement, one JSON line; what the set starts)
VALU fraction: the algorithmic lane-operations of the formulation (RULE_VALU_PER_PAIR_ROW per 64-cell pair
row and generation under a table rule, 22 under B3/S23) over the call time, against bench.py's issue peak.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mpi-and-open-mp_amd"))
VALU_PEAK = 256 * 4 * 32 * 2.4e9  # lane-ops/s, as bench.py
WARMUP, STEPS = 32, 992
CASES = [("B3/S23", 65536, 65536), ("B36/S23", 65536, 65536), ("B3678/S34678", 65536, 65536),
         ("B3/S23", 16384, 32768), ("B36/S23", 16384, 32768), ("B3678/S34678", 16384, 32768)]


def one(rule, nx, ny):
    import life_mi355x as lm

    conway = lm.parse_rule(rule) == lm.RULE_CONWAY
    with lm.Life(nx, ny, kernel="bit", rule=rule) as life:
        life.fill_random(1, 0.5)
        life.step(WARMUP)
        life.sync()
        t0 = time.perf_counter()
        life.step(STEPS)
        life.sync()
        dt = time.perf_counter() - t0
        per_row = lm.CONWAY_VALU_PER_PAIR_ROW if conway else lm.RULE_VALU_PER_PAIR_ROW
        updates = float(nx) * ny * STEPS
        print(json.dumps(dict(rule=life.rule, nx=nx, ny=ny, path=life.last_path(), tcell=round(updates / dt / 1e12, 3),
                              valu_frac=round(updates * per_row / 64.0 / dt / VALU_PEAK, 4), live=life.live_count(),
                              checksum=life.checksum())), flush=True)


def main():
    if sys.argv[1] == "--one":
        return one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    with open(sys.argv[1], "a") as out:
        for rule, nx, ny in CASES * runs:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", rule, str(nx), str(ny)],
                                   capture_output=True, text=True, timeout=120, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(f"{rule} {nx}x{ny}: time limit, stopping", flush=True)
                return 1
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or len(lines) != 1:
                print(f"{rule} {nx}x{ny}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}", flush=True)
                return 1
            out.write(lines[0] + "\n")
            out.flush()
            print(lines[0], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
