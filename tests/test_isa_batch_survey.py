"""Static guards on the survey forms of the batch's wave tier (CPU only;
DESIGN.md §5.12): a rule per universe under every detector and cycle detection
under the uniform rules are kernels of their own, and each keeps what §5.11
claims of the wave tier -- registers for 8 waves per SIMD, no LDS allocation,
no scratch, and a generation loop of lane moves and VALU alone: the universe's
masks are read before it."""
import re

import pytest

from test_isa import kernel_lines
from test_isa_batch import VGPR_BUDGET, generation_loops, isa, kernel_notes  # noqa: F401 (isa: the fixture)

CONWAY, TABLE, PER_UNIVERSE = 0, 1, 2  # SurveyRule of csrc/life_batch_kernels.hip
NONE, SETTLE, CYCLE = 0, 1, 2  # Detector
INSTANCES = [(w, PER_UNIVERSE, det) for w in (1, 2, 3, 4) for det in (NONE, SETTLE, CYCLE)]
INSTANCES += [(w, rule, CYCLE) for w in (1, 2, 3, 4) for rule in (CONWAY, TABLE)]


def all_generation_loops(lines):
    """generation_loops of test_isa_batch.py, and the loops it does not see: a
    loop that leaves by a break in its middle (the detecting loop of the cycle
    forms) closes with an unconditional s_branch.  A backward branch over the
    kernel's end is a jump to the epilogue and no loop."""
    out = list(generation_loops(lines))
    for addr, op, text in lines:
        m = re.match(r"s_branch (\d+)$", text)
        if not m or int(m.group(1)) < 0x8000:
            continue
        target = addr + 4 + 4 * (int(m.group(1)) - 0x10000)
        ops = [o for a, o, _ in lines if target <= a <= addr]
        if "v_bitop3_b32" in ops:
            out.append(ops)
    return [ops for ops in out if "s_endpgm" not in ops]


def instance(w, rule, det):
    return f"batch_survey_kernel<{w}, {rule}, {det}>"


def test_every_instance_is_built_and_no_other(isa):
    names = [n for n in kernel_notes(isa[1]) if "batch_survey_kernel" in n]
    for inst in INSTANCES:
        assert sum(instance(*inst) in n for n in names) == 1, instance(*inst)
    assert len(names) == len(INSTANCES) == 20
    assert not any("batch_wave_kernel" in n for n in names)


def test_registers_for_eight_waves_and_no_lds_or_scratch(isa):
    notes = kernel_notes(isa[1])
    for inst in INSTANCES:
        name, f = next((n, f) for n, f in notes.items() if instance(*inst) in n)
        assert f["vgpr_count"] <= VGPR_BUDGET and f["agpr_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] == 0, (name, f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert f.get("sgpr_spill_count", 0) == 0, (name, f)


@pytest.mark.parametrize("w,rule,det", INSTANCES)
def test_generation_loop_is_lane_moves_and_valu(isa, w, rule, det):
    lines = kernel_lines(isa[0], instance(w, rule, det))
    ops_all = [op for _, op, _ in lines]
    assert "s_barrier" not in ops_all
    assert not any(op.startswith(("ds_read", "ds_write", "scratch_", "buffer_")) for op in ops_all)
    # The cycle forms hold two loops, the detecting generations and the rest, with what is recorded written
    # between them.  The settle forms are held to what test_isa_batch.py holds the uniform settle kernels to:
    # they record their flag in a block placed out of line that branches back in, which is no part of a
    # generation.
    loops = all_generation_loops(lines) if det == CYCLE else generation_loops(lines)
    assert len(loops) >= (2 if det == CYCLE else 1), "generation loops not found"
    for ops in loops:
        assert not any(op.startswith("ds_") and op != "ds_bpermute_b32" for op in ops)
        # no memory traffic per generation: the rule table is read before the loop
        assert not any(op.startswith(("global_", "flat_", "s_load", "s_buffer_load")) for op in ops)
    for full in loops:  # each a loop of whole generations: 4 lane moves and 2 funnel shifts per word
        assert full.count("ds_bpermute_b32") == 4 * w
        assert full.count("v_alignbit_b32") == 2 * w
