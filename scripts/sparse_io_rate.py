#!/usr/bin/env python3
"""Rate of the density map against the census (measurement tool): one
process, a size^2 bit grid of 50 % random soup, alternating timed
live_count() and gather_density(256) calls -- both blocking, both one pass
over the same owned words (size^2 / 8 bytes), each timed with the host clock
around the call (it ends in a device synchronise and a small copy).  Prints
one JSON line: both medians, the HBM read rate each stands for, its ratio to
the copy ceiling of the same run (life_measure_copy counts read + write
bytes), and the time of a 50-cell set_cells (halo refill and syncs
included), of a 512 x 512 gather_rect and of a 512 x 512 set_rect across
the periodic corner.

The way in is measured in the same process: upload_bits(packed) against
upload(dense) of the same state, alternating, host clock around each blocking
call (pageable host memory, the staging copy, the unpack / import kernel, the
halo refill and the syncs included); and the unbits kernel alone under HIP
events (set_timing(2): upload_bits' unpack launch takes an event pair of its
own), as read + written bytes over its time against the copy ceiling.  The
dense baseline needs the size^2-byte host grid this call exists to avoid."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-and-open-mp_amd"))
import life_mi355x as lm  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    v = fn()
    return (time.perf_counter() - t0) * 1e3, v


p = argparse.ArgumentParser()
p.add_argument("--size", type=int, default=65536)
p.add_argument("--factor", type=int, default=256)
p.add_argument("--reps", type=int, default=5)
p.add_argument("--kernel", default="bit")
p.add_argument("--out", default=None, help="also write the JSON line to this file")
a = p.parse_args()
copy = lm.measure_copy(0, 2 << 30, 5)
cfg = os.path.join(ROOT, "tests", "golden", "cfg", "p46gun.cfg")
cells = lm.load_cfg_cells(cfg)[4]
with lm.Life(a.size, a.size, kernel=a.kernel) as life:
    life.fill_random(1, 0.5)
    live = life.live_count()  # warm-up of both kernels
    assert int(life.gather_density(a.factor).sum(dtype="uint64")) == live
    census_ms, density_ms = [], []
    for _ in range(a.reps):
        ms, n = timed(life.live_count)
        assert n == live
        census_ms.append(ms)
        ms, d = timed(lambda: life.gather_density(a.factor))
        assert int(d.sum(dtype="uint64")) == live
        density_ms.append(ms)
    life.set_cells(cells)  # warm-up
    set_ms = [timed(lambda: life.set_cells(cells))[0] for _ in range(a.reps)]
    life.gather_rect(0, 0, 512, 512)
    rect_ms = [timed(lambda: life.gather_rect(-256, -256, 512, 512))[0] for _ in range(a.reps)]
    win = (np.random.default_rng(1).random((512, 512)) < 0.5).astype(np.uint8)
    life.set_rect(-256, -256, win)  # warm-up
    paste_ms = [timed(lambda: life.set_rect(-256, -256, win))[0] for _ in range(a.reps)]
    life.fill_random(1, 0.5)
    packed, dense = life.gather_bits(), life.gather()
    life.upload_bits(packed)  # warm-up of both paths (code objects, the staging buffer)
    life.upload(dense)
    bits_ms, dense_ms, unbits_ms = [], [], []
    for _ in range(a.reps):
        bits_ms.append(timed(lambda: life.upload_bits(packed))[0])
        assert life.live_count() == live
        dense_ms.append(timed(lambda: life.upload(dense))[0])
        assert life.live_count() == live
    for _ in range(a.reps):  # the kernel alone: one timed launch per call
        life.set_timing(2)
        life.upload_bits(packed)
        ms, n, _ = life.kernel_stats()
        assert n == 1
        unbits_ms.append(ms)
    life.set_timing(False)
    assert life.live_count() == live
    ub, ud, uk = statistics.median(bits_ms), statistics.median(dense_ms), statistics.median(unbits_ms)
    unbits_bytes = float(packed.nbytes) + float(a.size) ** 2 * (0.125 if a.kernel == "bit" else 1.0)
    nbytes = float(a.size) ** 2 * (0.125 if a.kernel == "bit" else 1.0)
    c, dm = statistics.median(census_ms), statistics.median(density_ms)
    line = json.dumps({
        "size": a.size, "kernel": a.kernel, "factor": a.factor, "reps": a.reps, "live_cells": live,
        "live_count_ms": round(c, 4), "gather_density_ms": round(dm, 4),
        "live_count_ms_all": [round(v, 4) for v in census_ms],
        "gather_density_ms_all": [round(v, 4) for v in density_ms],
        "density_over_census": round(dm / c, 4), "read_bytes": nbytes,
        "live_count_read_GBps": round(nbytes / (c * 1e-3) / 1e9, 1),
        "gather_density_read_GBps": round(nbytes / (dm * 1e-3) / 1e9, 1),
        "copy_ceiling_GBps": round(copy, 1),
        "live_count_frac_of_copy_ceiling": round(nbytes / (c * 1e-3) / 1e9 / copy, 4),
        "gather_density_frac_of_copy_ceiling": round(nbytes / (dm * 1e-3) / 1e9 / copy, 4),
        "set_cells_50_ms": round(statistics.median(set_ms), 4),
        "gather_rect_512_ms": round(statistics.median(rect_ms), 4),
        "set_cells_50_ms_all": [round(v, 4) for v in set_ms],
        "gather_rect_512_ms_all": [round(v, 4) for v in rect_ms],
        "set_rect_512_ms": round(statistics.median(paste_ms), 4),
        "set_rect_512_ms_all": [round(v, 4) for v in paste_ms],
        "upload_bits_ms": round(ub, 3), "upload_ms": round(ud, 3), "upload_over_upload_bits": round(ud / ub, 3),
        "upload_bits_ms_all": [round(v, 3) for v in bits_ms], "upload_ms_all": [round(v, 3) for v in dense_ms],
        "upload_bits_host_bytes": packed.nbytes, "upload_host_bytes": dense.nbytes,
        "upload_bits_host_GBps": round(packed.nbytes / (ub * 1e-3) / 1e9, 2),
        "upload_host_GBps": round(dense.nbytes / (ud * 1e-3) / 1e9, 2),
        "unbits_kernel_ms": round(uk, 4), "unbits_kernel_ms_all": [round(v, 4) for v in unbits_ms],
        "unbits_kernel_bytes": unbits_bytes, "unbits_kernel_GBps": round(unbits_bytes / (uk * 1e-3) / 1e9, 1),
        "unbits_kernel_frac_of_copy_ceiling": round(unbits_bytes / (uk * 1e-3) / 1e9 / copy, 4),
        "unbits_kernel_share_of_upload_bits": round(uk / ub, 5)})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
