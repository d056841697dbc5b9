"""Static guards on the table-rule bit tiles of the shipped gfx950 code object
(CPU only; skips like tests/test_isa.py when the object is missing): the
instance exists under its own name, fits 2 tiles per CU without spills, its
generation loop has the Conway tiles' shape (one barrier, two permutes and two
funnel shifts per pair row) and issues exactly the VALU instructions per pair
row that life_dev_kernel_work books (life_mi355x.RULE_VALU_PER_PAIR_ROW)."""
import re
import subprocess

from test_isa import isa, kernel_lines  # noqa: F401

KERNEL = "trule_bit_kernel<24, true, true, 8>"  # the single-GPU instance under a rule
ROWS = 24


def full_height_loops(lines):
    """Op sequences of the generation loops with a full-height window: the
    backward branches whose body holds a barrier and 2 permutes per pair row."""
    out = []
    for addr, op, text in lines:
        m = re.match(r"s_cbranch_\w+ (\d+)$", text)
        if not m or int(m.group(1)) < 0x8000:
            continue
        target = addr + 4 + 4 * (int(m.group(1)) - 0x10000)
        ops = [o for a, o, _ in lines if target <= a <= addr]
        if "s_barrier" in ops and ops.count("ds_bpermute_b32") == 2 * ROWS:
            out.append(ops)
    return out


def test_rule_tile_budget(isa):
    notes = isa[1]
    names = re.findall(r"\.name:\s+(\S+)", notes)
    vgprs = re.findall(r"\.vgpr_count:\s+(\d+)", notes)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    found = [(int(v), int(s)) for n, v, s in zip(dem, vgprs, spills) if KERNEL in n]
    assert found, "no table-rule tile instance"
    assert all(v <= 128 and s == 0 for v, s in found), found  # 2 tiles of 8 waves per CU: 4 waves per SIMD
    # its name must not be caught by the B3/S23 guards of tests/test_isa.py
    assert not any("tstep_bit_kernel<" in n for n in dem if "trule_bit_kernel" in n)


def test_rule_generation_loop(isa, lm):
    loops = full_height_loops(kernel_lines(isa[0], KERNEL))
    assert loops, "no full-height generation loop found"
    per_row = lm.RULE_VALU_PER_PAIR_ROW
    for ops in loops:
        assert ops.count("s_barrier") == 1
        assert ops.count("ds_bpermute_b32") == 2 * ROWS and ops.count("v_alignbit_b32") == 2 * ROWS
        valu = [o for o in ops if o.startswith("v_")]
        # the rows' work is funnel shifts and 3-input bit operations ...
        assert ops.count("v_alignbit_b32") + ops.count("v_bitop3_b32") == per_row * ROWS
        # ... and nothing else per row (the loop's own bookkeeping: under one instruction per row)
        assert len(valu) // ROWS == per_row, (len(valu), per_row)
