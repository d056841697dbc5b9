"""Static guards on the Generations kernels of the batch's wave tier (CPU only;
DESIGN.md §5.13), the sibling of test_isa_batch_survey.py: the instances that
are built, no scratch, LDS allocation or AGPRs, generation loops of lane moves
and VALU alone, and -- the claim that the decay planes cost no lane traffic --
the 4 ds_bpermute and 2 v_alignbit per word of the two-state kernels whatever
the number of planes."""
import re

import pytest

from test_isa import kernel_lines
from test_isa_batch import isa, kernel_notes  # noqa: F401 (isa: the fixture)

NONE, SETTLE, CYCLE = 0, 1, 2  # Detector of csrc/life_batch_kernels.hip
INSTANCES = [(w, p, det) for w in (1, 2, 3, 4) for p in (1, 2, 4) for det in (NONE, SETTLE, CYCLE)]
VGPR_CAP = 128  # four waves per SIMD, the waves of one workgroup: the hard limit
# v_bitop3 of a generation per word: the 28 of the table rule's and the decay step's 2, 6 (P = 2: and a v_xor
# beside them) and 12 (P = 4: and a v_xor and a v_and)
BITOP3_PER_WORD = {1: 30, 2: 34, 4: 40}
# Waves per SIMD, min(8, 512 // allocation) with registers allocated in eights, as found when the kernels were
# written (DESIGN.md §5.13 lists the counts): a change of step in either direction is worth a look.
WAVES = {
    (1, 1): (8, 8, 8), (1, 2): (8, 8, 8), (1, 4): (8, 8, 8),
    (2, 1): (8, 8, 8), (2, 2): (8, 8, 8), (2, 4): (8, 5, 6),
    (3, 1): (8, 8, 8), (3, 2): (8, 6, 7), (3, 4): (7, 4, 5),
    (4, 1): (8, 7, 8), (4, 2): (8, 5, 7), (4, 4): (7, 4, 5),
}  # [W, P] -> (no detector, settle, cycle)


def instance(w, p, det):
    return f"batch_gen_kernel<{w}, {p}, {det}>"


def lines_of(dis, name):
    return kernel_lines(dis + "\n0 <end>:\n", name)  # (the kernel may be the last of the code object)


def generation_loops(lines):
    """Op lists of the innermost loops that hold the stencil.  A loop is the
    span from the target of a backward branch (conditional or not: a loop left
    by a break in its middle closes with s_branch) to the nearest such branch;
    spans that enclose another target are outer loops or jumps back into
    out-of-line blocks and are not looked at."""
    back = {}
    for addr, _, text in lines:
        m = re.match(r"s_c?branch\w* (\d+)$", text)
        if m and int(m.group(1)) >= 0x8000:
            back.setdefault(addr + 4 + 4 * (int(m.group(1)) - 0x10000), []).append(addr)
    spans = [(t, min(a)) for t, a in back.items()]
    inner = [(t, e) for t, e in spans if not any(t <= t2 <= e for t2, e2 in spans if (t2, e2) != (t, e))]
    loops = [[op for a, op, _ in lines if t <= a <= e] for t, e in inner]
    return [ops for ops in loops if "v_bitop3_b32" in ops]


def test_every_instance_is_built_and_no_other(isa):
    names = [n for n in kernel_notes(isa[1]) if "batch_gen_kernel" in n]
    for inst in INSTANCES:
        assert sum(instance(*inst) in n for n in names) == 1, instance(*inst)
    assert len(names) == len(INSTANCES) == 36
    assert not any("batch_wave_kernel" in n or "batch_survey_kernel" in n for n in names)


def test_registers_and_no_lds_or_scratch(isa):
    notes = kernel_notes(isa[1])
    for w, p, det in INSTANCES:
        name, f = next((n, f) for n, f in notes.items() if instance(w, p, det) in n)
        assert f["vgpr_count"] <= VGPR_CAP and f["agpr_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] == 0, (name, f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert f.get("sgpr_spill_count", 0) == 0, (name, f)
        waves = min(8, 512 // (8 * ((f["vgpr_count"] + 7) // 8)))
        assert waves == WAVES[w, p][det], (name, f["vgpr_count"], waves)
    for name, f in notes.items():  # the data movement of the states spills nothing either
        if "batch_" in name and "states_kernel" in name:
            assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)


@pytest.mark.parametrize("w,p,det", INSTANCES)
def test_generation_loop_is_lane_moves_and_valu(isa, w, p, det):
    lines = lines_of(isa[0], instance(w, p, det))
    ops_all = [op for _, op, _ in lines]
    assert "s_barrier" not in ops_all
    assert not any(op.startswith(("ds_read", "ds_write", "scratch_", "buffer_")) for op in ops_all)
    loops = generation_loops(lines)
    # the cycle forms hold two loops, the detecting generations and the rest
    assert len(loops) >= (2 if det == CYCLE else 1), "generation loops not found"
    for ops in loops:
        assert not any(op.startswith("ds_") and op != "ds_bpermute_b32" for op in ops)
        # no memory traffic per generation: the universe's masks and state count are read before the loop
        assert not any(op.startswith(("global_", "flat_", "s_load", "s_buffer_load")) for op in ops)
        # whole generations: the lane moves and funnel shifts of the two-state kernels, whatever P is
        assert ops.count("ds_bpermute_b32") == 4 * w
        assert ops.count("v_alignbit_b32") == 2 * w
        assert ops.count("v_bitop3_b32") <= BITOP3_PER_WORD[p] * w + w  # (the compiler folds an op here and there)
        assert ops.count("v_bitop3_b32") >= BITOP3_PER_WORD[p] * w - w
