"""Same-box ABAB of bench.py lines for the band split of the last tile column: the parent commit's
library (built from its own tree, given as LIFE_AB_PARENT_LIB and loaded through LIFE_MI355X_LIB)
against this tree's, the arms alternating.  Every run is a fresh child process with its own time
limit; the first failure stops the set.

usage: LIFE_AB_PARENT_LIB=/path/to/parent/liblife_mi355x.so python profiles/bandsplit/ab.py SET OUT.jsonl [RUNS]
sets: default driver half_flow0 half n8 byte   (results: *.jsonl and README.md beside this file)
arms: parent; split = this tree; one = this tree with LIFE_BAND_SPLIT=0 (must sit with the parent)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
P = {"LIFE_MI355X_LIB": os.environ.get("LIFE_AB_PARENT_LIB", "")}
ONE = {"LIFE_BAND_SPLIT": "0"}

SETS = {
    "default": ([], {}, True),                                    # 65536^2, 992 generations: 83 passes of 11-12
    "driver": (["--steps", "20", "--warmup", "5"], {}, True),     # the driver-shaped call: 2 passes of 10
    "half_flow0": (["--shape", "32768x65536"], {"LIFE_FLOW": "0"}, False),  # o = 16: {14, 2}, pipelined tiles
    "half": (["--shape", "32768x65536"], {}, True),               # the dataflow form: one band, unchanged
    "n8": (["--shape", "16384x32768"], {}, False),                # o = 8: {6, 2}, one round + half-height tail
    "byte": (["--kernel", "byte"], {}, False),                    # byte tiles have no bands
}


def main():
    name, path = sys.argv[1], sys.argv[2]
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    if not os.path.exists(P["LIFE_MI355X_LIB"]):
        raise SystemExit("LIFE_AB_PARENT_LIB: the parent commit's liblife_mi355x.so")
    args, env, with_one = SETS[name]
    arms = [("parent", dict(env, **P)), ("split", env)] + ([("one", dict(env, **ONE))] if with_one else [])
    with open(path, "a") as out:
        for label, e in arms * runs:
            t0 = time.time()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                                   env=dict(os.environ, **e), capture_output=True, text=True, timeout=150, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(f"{label}: time limit, stopping", flush=True)
                return 1
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or len(lines) != 1:
                print(f"{label}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}", flush=True)
                return 1
            j = json.loads(lines[0])
            roof = j.get("roofline", {})
            rec = dict(set=name, arm=label, value=j["value"], live=j.get("config", {}).get("live_cells_end"),
                       ms_per_step=j.get("ms_per_step"), call=j.get("call"), frac=roof.get("frac"),
                       issued_frac=roof.get("issued", {}).get("frac"), wall_s=round(time.time() - t0, 1))
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(f"{name:10s} {label:8s} {j['value']:10.3f} Gcell/s  frac {rec['frac']} issued {rec['issued_frac']}  "
                  f"live {rec['live']}  wall {rec['wall_s']} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
