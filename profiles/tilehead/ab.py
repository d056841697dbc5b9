"""Same-box ABAB of bench.py lines for the bit tiles' trimmed head and tail (32-bit item decode, straight-
line window load and store): the parent commit's library (built from its own tree, given as
LIFE_AB_PARENT_LIB and loaded through LIFE_MI355X_LIB) against this tree's, the arms alternating.  Every
run is a fresh child process with its own time limit; the first failure stops the set.

usage: LIFE_AB_PARENT_LIB=/path/to/parent/liblife_mi355x.so python profiles/tilehead/ab.py SET OUT.jsonl [RUNS]
sets: default driver s32k n8 tall byte; m: this tree at LIFE_BLOCK_GENS = 10, 11, 12 (the default line)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
P = {"LIFE_MI355X_LIB": os.environ.get("LIFE_AB_PARENT_LIB", "")}

SETS = {
    "default": [],                             # 65536^2, 992 generations: 83 pipelined passes of 11-12
    "driver": ["--steps", "20", "--warmup", "5"],  # the driver-shaped call: 2 passes of 10
    "s32k": ["--shape", "32768x32768"],        # the dataflow form
    "n8": ["--shape", "16384x32768"],          # one round + half-height tail per pass
    "tall": ["--shape", "32768x65536"],
    "byte": ["--kernel", "byte"],              # the untouched control
    "m": [],
}


def main():
    name, path = sys.argv[1], sys.argv[2]
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    if name == "m":
        arms = [(f"m{m}", {"LIFE_BLOCK_GENS": str(m)}) for m in (10, 11, 12)]
    else:
        if not os.path.exists(P["LIFE_MI355X_LIB"]):
            raise SystemExit("LIFE_AB_PARENT_LIB: the parent commit's liblife_mi355x.so")
        arms = [("parent", P), ("new", {})]
    base = {k: v for k, v in os.environ.items() if k not in ("LIFE_BLOCK_GENS", "LIFE_MI355X_LIB")}
    with open(path, "a") as out:
        for label, e in arms * runs:
            t0 = time.time()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SETS[name]],
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
            print(f"{name:8s} {label:7s} {j['value']:10.3f}  frac {rec['frac']} issued {rec['issued_frac']}  "
                  f"live {rec['live']}  wall {rec['wall_s']} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
