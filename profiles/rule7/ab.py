"""Same-box ABAB of bench.py lines for the 7-gate B3/S23 rule of the bit tiles (LIFE_OPT_RULE7): the
parent commit's library (built from its own tree, given as LIFE_AB_PARENT_LIB and loaded through
LIFE_MI355X_LIB) against this tree's, the arms alternating.  Every run is a fresh child process with
its own time limit; the first failure stops the set.

usage: LIFE_AB_PARENT_LIB=/path/to/parent/liblife_mi355x.so python profiles/rule7/ab.py SET OUT.jsonl [RUNS]
sets: default driver s32k n8 byte   (results: *.jsonl and README.md beside this file)
arms: parent; rule7 = this tree; off = this tree with LIFE_RULE7=0 (must sit with the parent)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
P = {"LIFE_MI355X_LIB": os.environ.get("LIFE_AB_PARENT_LIB", "")}
OFF = {"LIFE_RULE7": "0"}

SETS = {
    "default": ([], True),                               # 65536^2, 992 generations: 83 pipelined passes of 11-12
    "driver": (["--steps", "20", "--warmup", "5"], True),  # the driver-shaped call: 2 passes of 10
    "s32k": (["--shape", "32768x32768"], True),          # the dataflow form
    "n8": (["--shape", "16384x32768"], True),            # one round + half-height tail per pass
    "byte": (["--kernel", "byte"], True),                # the untouched control
}


def main():
    name, path = sys.argv[1], sys.argv[2]
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    if not os.path.exists(P["LIFE_MI355X_LIB"]):
        raise SystemExit("LIFE_AB_PARENT_LIB: the parent commit's liblife_mi355x.so")
    args, with_off = SETS[name]
    arms = [("parent", P), ("rule7", {})] + ([("off", OFF)] if with_off else [])
    base = {k: v for k, v in os.environ.items() if k != "LIFE_RULE7"}
    with open(path, "a") as out:
        for label, e in arms * runs:
            t0 = time.time()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                                   env=dict(base, **e), capture_output=True, text=True, timeout=150, cwd=ROOT)
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
            print(f"{name:10s} {label:8s} {j['value']:10.3f}  frac {rec['frac']} issued {rec['issued_frac']}  "
                  f"live {rec['live']}  wall {rec['wall_s']} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
