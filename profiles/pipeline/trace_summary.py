"""Summary of a rocprofv3 --kernel-trace CSV of `bench.py --steps 96 --warmup 32`: the tile kernels
of the timed call (its last 8 passes), which of them overlap the launch before, and the time per
pass (first start to last end over the passes).
usage: python trace_summary.py trace_kernel_trace.csv PASSES"""
import csv
import sys


def main(path, passes):
    rows = [r for r in csv.DictReader(open(path)) if "tstep" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = 1
    # the timed call is the last `passes` passes: its launches are the trailing ones of equal grid size
    k = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]),
          r["Queue_Id"]) for r in rows]
    whole = max(g for _, _, g, _ in k)
    tail = [x for x in k if x[2] < whole / 2]
    if tail:  # region launches: the call's launches are the trailing run of them
        n = 0
        while n < len(k) and k[-1 - n][2] < whole / 2:
            n += 1
        call, per = k[-n:], n // passes
    else:
        call = k[-passes:]
    t0 = call[0][0]
    print(f"{len(call)} launches, {per} per pass, queues {sorted(set(q for *_, q in call))}")
    for i, (a, b, g, q) in enumerate(call):
        prev_end = call[i - 1][1] if i else a
        print(f"{i:3d} queue {q} items {g:5d} start {(a - t0) / 1e3:9.1f} us  dur {(b - a) / 1e3:7.1f} us  "
              f"starts {(prev_end - a) / 1e3:7.1f} us before the previous launch ends")
    span = (call[-1][1] - t0) / 1e3
    print(f"span {span:.1f} us, {span / passes:.1f} us per pass")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
