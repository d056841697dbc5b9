"""Static guards on the recording kernels of the batch unit (CPU only;
DESIGN.md §5.14), in the manner of test_isa_batch.py: every instance is built
under a name of its own, none has scratch or spills, the wave tier still has
no barrier and no LDS exchange, the group tier still has one barrier per
generation, and the registers stay within the budgets the tiers need."""
import re

import pytest

from test_isa import kernel_lines
from test_isa_batch import INSTANCES as WAVE_INSTANCES
from test_isa_batch import VGPR_BUDGET, generation_loops, isa, kernel_notes  # noqa: F401 (isa: the fixture)
from test_isa_batch import instance as wave_instance
from test_isa_batch_gen import INSTANCES as GEN_INSTANCES
from test_isa_batch_gen import instance as gen_instance
from test_isa_batch_survey import INSTANCES as SURVEY_INSTANCES
from test_isa_batch_survey import instance as survey_instance

CONWAY, TABLE, PER_UNIVERSE = 0, 1, 2  # SurveyRule of csrc/life_batch_kernels.hip
NONE, SETTLE, CYCLE = 0, 1, 2  # Detector
TRACE = [(w, rule, det) for w in (1, 2, 3, 4) for rule in (CONWAY, TABLE, PER_UNIVERSE) for det in (NONE, SETTLE, CYCLE)]
ROWS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 25, 32)  # the strip heights of the group tier
VGPR_CAP = 128  # a workgroup of 1024 threads: the hard limit


def trace_instance(w, rule, det):
    return f"batch_trace_kernel<{w}, {rule}, {det}>"


def group_instance(rows):
    return f"batch_trace_group_kernel<{rows}>"


def lines_of(dis, name):
    return kernel_lines(dis + "\n0 <end>:\n", name)  # (the kernel may be the last of the code object)


def fields(notes, name):
    found = [(n, f) for n, f in notes.items() if name in n]
    assert len(found) == 1, (name, [n for n, _ in found])
    return found[0]


def test_every_recording_instance_is_built(isa):
    notes = kernel_notes(isa[1])
    for inst in TRACE:
        fields(notes, trace_instance(*inst))
    for rows in ROWS:
        fields(notes, group_instance(rows))
    assert sum("batch_trace_kernel" in n for n in notes) == len(TRACE) == 36
    assert sum("batch_trace_group_kernel" in n for n in notes) == len(ROWS) == 13
    # no recording kernel is counted among the others
    for n in notes:
        if "batch_trace" in n:
            assert not any(old in n for old in ("batch_wave_kernel", "batch_survey_kernel", "batch_gen_kernel",
                                                "batch_group_kernel")), n


def test_the_existing_instances_keep_their_names(isa):
    notes = kernel_notes(isa[1])
    for inst in WAVE_INSTANCES:
        assert any(wave_instance(*inst) in n for n in notes), wave_instance(*inst)
    for inst in SURVEY_INSTANCES:
        fields(notes, survey_instance(*inst))
    for inst in GEN_INSTANCES:
        fields(notes, gen_instance(*inst))
    for rows in ROWS:
        fields(notes, f"batch_group_kernel<{rows}>")


def test_no_scratch_no_spills_and_registers(isa):
    notes = kernel_notes(isa[1])
    for w, rule, det in TRACE:
        name, f = fields(notes, trace_instance(w, rule, det))
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert f.get("sgpr_spill_count", 0) == 0 and f["agpr_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] == 0, (name, f)  # no LDS allocation
        survey = rule == PER_UNIVERSE or det == CYCLE
        print(name, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"])
        assert f["vgpr_count"] <= (VGPR_CAP if survey else VGPR_BUDGET), (name, f)
    for rows in ROWS:
        name, f = fields(notes, group_instance(rows))
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert f.get("sgpr_spill_count", 0) == 0, (name, f)
        print(name, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "lds", f["group_segment_fixed_size"])
        assert f["vgpr_count"] + f["agpr_count"] <= VGPR_CAP, (name, f)


@pytest.mark.parametrize("w,rule,det", TRACE)
def test_wave_tier_has_no_barrier_and_no_lds_exchange(isa, w, rule, det):
    ops = [op for _, op, _ in lines_of(isa[0], trace_instance(w, rule, det))]
    assert "s_barrier" not in ops
    assert not any(op.startswith(("ds_read", "ds_write")) for op in ops)


def barrier_loops(lines):
    """Op lists of the bodies of backward branches that hold the stencil."""
    out = []
    for addr, _, text in lines:
        m = re.match(r"s_c?branch\w* (\d+)$", text)
        if not m or int(m.group(1)) < 0x8000:
            continue
        target = addr + 4 + 4 * (int(m.group(1)) - 0x10000)
        ops = [o for a, o, _ in lines if target <= a <= addr]
        if "v_bitop3_b32" in ops:
            out.append(ops)
    return out


@pytest.mark.parametrize("rows", ROWS)
def test_group_tier_keeps_one_barrier_per_generation(isa, rows):
    loops = barrier_loops(lines_of(isa[0], group_instance(rows)))
    assert loops, "no generation loop found"
    for ops in loops:
        assert ops.count("s_barrier") == 1
