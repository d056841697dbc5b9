"""Same-box ABAB of the default bench.py line: the parent commit's library (built from its own tree,
given as LIFE_AB_PARENT_LIB and loaded through LIFE_MI355X_LIB) against this tree's, the arms
alternating.  Every run is a fresh child process with its own time limit; the first failure stops.

usage: LIFE_AB_PARENT_LIB=/path/to/parent/liblife_mi355x.so python profiles/rule/ab.py OUT.jsonl [RUNS]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    path = sys.argv[1]
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    parent = os.environ.get("LIFE_AB_PARENT_LIB", "")
    if not os.path.exists(parent):
        raise SystemExit("LIFE_AB_PARENT_LIB: the parent commit's liblife_mi355x.so")
    with open(path, "a") as out:
        for label, e in [("parent", {"LIFE_MI355X_LIB": parent}), ("rule", {})] * runs:
            t0 = time.time()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"],
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
            rec = dict(arm=label, value=j["value"], live=j.get("config", {}).get("live_cells_end"),
                       frac=roof.get("frac"), issued_frac=roof.get("issued", {}).get("frac"),
                       wall_s=round(time.time() - t0, 1))
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(f"{label:8s} {j['value']:10.3f} Gcell/s  frac {rec['frac']} issued {rec['issued_frac']}  "
                  f"live {rec['live']}  wall {rec['wall_s']} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
