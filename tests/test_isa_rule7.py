"""Static guards on the 7-gate arm of the B3/S23 bit tiles in the shipped
gfx950 code object (CPU only, no GPU; skipped like tests/test_isa.py when the
object is not built).

ConwayRule7 (csrc/life_bitops.h) takes 7 v_bitop3 per dword instead of 8: a
pair row of tstep_bit7_kernel is 2 v_alignbit + 18 v_bitop3, 24 pair rows 432
v_bitop3 per generation against tstep_bit_kernel's 480.  The op-count model
(tstep_valu_per_tile_lane) prices both arms at 22 per pair row, so these
counts, not the model, say what really issues.  The gain is only worth having
if the compiler keeps the schedule of the 8-gate loop: the permutes well ahead
of their waits (the threshold of tests/test_isa.py) inside the 80 VGPRs of 3
tiles per CU.
"""
import re
import subprocess

import pytest

from test_isa import generation_loops, isa, kernel_lines  # noqa: F401  (isa: the module's fixture)

KERNEL7 = "tstep_bit7_kernel<24, true, true, 8>"  # the 65536^2 single-GPU instance, 7-gate arm
FLOW7 = "tflow7_kernel<24, true, true, 1, 8, false>"  # the dataflow form (write-through hand-off), 7-gate arm
BITOPS = 24 * 18  # pair rows x (2 full adders + 2 x 7)


def barrier_loops(lines):
    """Op lists of every backward-branch loop of the kernel that holds a barrier."""
    out = []
    for addr, _, text in lines:
        m = re.match(r"s_cbranch_\w+ (\d+)$", text)
        if not m or int(m.group(1)) < 0x8000:
            continue
        target = addr + 4 + 4 * (int(m.group(1)) - 0x10000)
        body = [t for a, _, t in lines if target <= a <= addr]
        if any(t.startswith("s_barrier") for t in body):
            out.append(body)
    return out


def resources(notes, kernel):
    names = re.findall(r"\.name:\s+(\S+)", notes)
    vgprs = re.findall(r"\.vgpr_count:\s+(\d+)", notes)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [(int(v), int(s)) for n, v, s in zip(dem, vgprs, spills) if kernel in n]


def test_the_8_gate_finder_sees_no_loop_here(isa):
    """tests/test_isa.py finds its loops by 480 v_bitop3: none in this arm."""
    assert generation_loops(kernel_lines(isa[0], KERNEL7)) == []


def shape(body):
    ops = [t.split()[0] for t in body]
    return (ops.count("v_bitop3_b32"), ops.count("v_alignbit_b32"), ops.count("ds_bpermute_b32"),
            ops.count("s_barrier"))


FULL = (BITOPS, 48, 48, 1)  # 24 pair rows x (18 v_bitop3 + 2 v_alignbit + 2 ds_bpermute), one barrier
HALF = (BITOPS // 2, 24, 24, 1)  # the launch tail's half-height tiles (tail_item: R / 2 = 12 rows per wave)


def test_generation_loop_counts(isa):
    """Every loop with a barrier is a generation loop at 18 v_bitop3 per pair
    row: the full-height tiles' (plain and banded), or the same loop over the
    12 rows of the launch tail's half-height tiles, which the kernel holds as
    tstep_bit_kernel does (tests/test_isa.py passes them by: it keeps the loops
    of 480).  A backward branch whose span holds several barriers encloses
    several such loops (the code after the last one branches back to a store
    block laid out before the first): its loops are counted one by one."""
    loops = barrier_loops(kernel_lines(isa[0], KERNEL7))
    print([shape(b) for b in loops])
    single = [b for b in loops if shape(b)[3] == 1]
    assert [b for b in single if shape(b) == FULL], "no full-height generation loop found"
    for body in single:
        assert shape(body) in (FULL, HALF), shape(body)


def test_bpermute_issued_ahead_of_use(isa):
    loops = [b for b in barrier_loops(kernel_lines(isa[0], KERNEL7)) if shape(b) == FULL]
    assert loops
    for body in loops:
        ops = [t.split()[0] for t in body]
        gaps = [next(k for k in range(i, len(ops)) if ops[k] == "s_waitcnt") - i
                for i, o in enumerate(ops) if o == "ds_bpermute_b32"]
        mean = sum(gaps) / len(gaps)
        print(f"ds_bpermute -> s_waitcnt mean {mean:.2f}")
        assert mean >= 5.0, f"ds_bpermute -> s_waitcnt mean {mean:.2f}"


@pytest.mark.parametrize("kernel", [KERNEL7, FLOW7])
def test_vgpr_budget(isa, kernel):
    found = resources(isa[1], kernel)
    print(found)
    assert found and all(v <= 80 and s == 0 for v, s in found), found


def test_flow_permutes_issued_ahead(isa):
    """As tests/test_isa.py's for tflow_kernel: the waits of the dataflow
    twin's generation loop leave the next row's permutes in flight."""
    loops = [b for b in barrier_loops(kernel_lines(isa[0], FLOW7))
             if [t.split()[0] for t in b].count("v_bitop3_b32") == BITOPS]
    assert loops, "no dataflow generation loop found"
    for body in loops:
        ahead = sum(1 for t in body if t in ("s_waitcnt lgkmcnt(2)", "s_waitcnt lgkmcnt(3)"))
        print(f"{ahead} waits with permutes in flight")
        assert ahead >= 40, f"{ahead} waits with permutes of the next row in flight"
