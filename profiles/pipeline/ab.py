"""Same-box ABAB of bench.py lines: the parent commit's library (built from its own tree, given as
LIFE_AB_PARENT_LIB and loaded through LIFE_MI355X_LIB) against this tree's, the arms alternating.
Every run is a fresh child process with its own time limit; the first failure stops the set.

usage: LIFE_AB_PARENT_LIB=/path/to/parent/liblife_mi355x.so python profiles/pipeline/ab.py SET OUT.jsonl
sets: default m10 driver half byte final passes lasttail   (results of this change: *.jsonl and README.md beside
this file); lasttail also wants LIFE_AB_VARIANT_LIB, a build of this tree whose last launch splits its tail
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
P = {"LIFE_MI355X_LIB": os.environ.get("LIFE_AB_PARENT_LIB", "")}


def arms(name):
    if name == "default":  # 65536^2, 992 generations: 83 passes of 11-12
        one = [("parent", P, []), ("R4", {"LIFE_PIPELINE": "4"}, []), ("off", {"LIFE_PIPELINE": "0"}, []),
               ("R6", {"LIFE_PIPELINE": "6"}, []), ("R3", {"LIFE_PIPELINE": "3"}, []),
               ("R8", {"LIFE_PIPELINE": "8"}, [])]
        return one * 4
    if name == "m10":  # 10 generations per pass: the tail model's pick once tails are free
        one = [("parent_m10", dict(P, LIFE_BLOCK_GENS="10"), []),
               ("R4_m10", {"LIFE_PIPELINE": "4", "LIFE_BLOCK_GENS": "10"}, []),
               ("R6_m10", {"LIFE_PIPELINE": "6", "LIFE_BLOCK_GENS": "10"}, []),
               ("parent", P, []), ("auto", {}, [])]
        return one * 3
    if name == "driver":  # the driver-shaped call: 2 passes of 10
        a = ["--steps", "20", "--warmup", "5"]
        return [("parent", P, a), ("R4", {"LIFE_PIPELINE": "4"}, a), ("auto", {}, a)] * 4
    if name == "half":  # 32768 x 65536: 4.3 rounds per pass, the dataflow form by default
        a = ["--shape", "32768x65536"]
        return [("parent", P, a), ("auto", {}, a), ("parent_flow0", dict(P, LIFE_FLOW="0"), a),
                ("R4_flow0", {"LIFE_PIPELINE": "4", "LIFE_FLOW": "0"}, a)] * 4
    if name == "byte":
        a = ["--kernel", "byte"]
        return [("parent", P, a), ("R4", {"LIFE_PIPELINE": "4"}, a), ("auto", {}, a),
                ("R3", {"LIFE_PIPELINE": "3"}, a)] * 3
    if name == "lasttail":  # LIFE_PIPE_LAST_TAIL=1 build: the call's very last launch splits its tail
        V = {"LIFE_MI355X_LIB": os.environ.get("LIFE_AB_VARIANT_LIB", "")}
        s4, d = ["--steps", "48"], ["--steps", "20", "--warmup", "5"]
        return ([("whole_4pass", {}, s4), ("split_4pass", V, s4)] * 4 +
                [("whole_R4_driver", {"LIFE_PIPELINE": "4"}, d), ("split_R4_driver", dict(V, LIFE_PIPELINE="4"), d)] * 4 +
                [("whole", {}, []), ("split", V, [])] * 3)
    if name == "passes":  # shorter calls: 4, 8 and 16 passes of 12
        out = []
        for n in (4, 8, 16):
            a = ["--steps", str(12 * n)]
            out += [(f"parent_{n}pass", P, a), (f"auto_{n}pass", {}, a)] * 4
        return out
    if name == "final":  # the automatic rule as committed against the parent
        b, h, s4 = ["--kernel", "byte"], ["--kernel", "byte", "--shape", "32768x65536"], ["--steps", "48"]
        d = ["--steps", "20", "--warmup", "5"]
        return ([("parent", P, []), ("auto", {}, [])] * 4 + [("parent_byte", P, b), ("auto_byte", {}, b)] * 4 +
                [("parent_byte_half", P, h), ("auto_byte_half", {}, h)] * 4 +
                [("parent_4pass", P, s4), ("auto_4pass", {}, s4)] * 4 +
                [("parent_driver", P, d), ("auto_driver", {}, d)] * 4)
    raise SystemExit(f"unknown set {name}")


def main():
    name, path = sys.argv[1], sys.argv[2]
    if not os.path.exists(P["LIFE_MI355X_LIB"]):
        raise SystemExit("LIFE_AB_PARENT_LIB: the parent commit's liblife_mi355x.so")
    with open(path, "a") as out:
        for label, env, args in arms(name):
            t0 = time.time()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                                   env=dict(os.environ, **env), capture_output=True, text=True, timeout=150, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(f"{label}: time limit, stopping", flush=True)
                return 1
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or len(lines) != 1:
                print(f"{label}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}", flush=True)
                return 1
            j = json.loads(lines[0])
            rec = dict(set=name, arm=label, value=j["value"], live=j.get("config", {}).get("live_cells_end"),
                       ms_per_step=j.get("ms_per_step"), call=j.get("call"), wall_s=round(time.time() - t0, 1))
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(f"{label:16s} {j['value']:10.3f} Gcell/s  span {j.get('call', {}).get('device_span_ms')} ms", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
