"""Static guards on the onset kernels of the batch's wave tier (CPU only;
DESIGN.md §5.15), the sibling of test_isa_batch_survey.py and
test_isa_batch_gen.py: the instances that are built, no scratch, spills, AGPRs
or LDS allocation, the register budgets of the kernels they extend, and the
shape of their generation loops -- the detecting loop, the loop that advances
the copy, and the rest loop step one state (4 ds_bpermute and 2 v_alignbit per
word), the joint walk of the search steps two."""
import re

import pytest

from test_isa_batch import VGPR_BUDGET, isa, kernel_notes  # noqa: F401 (isa: the fixture)
from test_isa_batch_gen import VGPR_CAP, lines_of

CONWAY, TABLE, PER_UNIVERSE = 0, 1, 2  # SurveyRule of csrc/life_batch_kernels.hip
INSTANCES = [(w, rule, pop) for w in (1, 2, 3, 4) for rule in (CONWAY, TABLE, PER_UNIVERSE)
             for pop in ("false", "true")]
GEN_INSTANCES = [(w, p) for w in (1, 2, 3, 4) for p in (1, 2, 4)]


def instance(w, rule, pop):
    return f"batch_onset_kernel<{w}, {rule}, {pop}>"


def gen_instance(w, p):
    return f"batch_onset_gen_kernel<{w}, {p}>"


def fields(notes, name):
    found = [(n, f) for n, f in notes.items() if name in n]
    assert len(found) == 1, (name, [n for n, _ in found])
    return found[0]


def test_every_instance_is_built_and_no_other(isa):
    notes = kernel_notes(isa[1])
    for inst in INSTANCES:
        fields(notes, instance(*inst))
    for inst in GEN_INSTANCES:
        fields(notes, gen_instance(*inst))
    assert sum("batch_onset_kernel" in n for n in notes) == len(INSTANCES) == 24
    assert sum("batch_onset_gen_kernel" in n for n in notes) == len(GEN_INSTANCES) == 12
    for n in notes:  # no onset kernel is counted among the others
        if "batch_onset" in n:
            assert not any(old in n for old in ("batch_wave_kernel", "batch_survey_kernel", "batch_gen_kernel",
                                                "batch_trace_kernel", "group_kernel")), n


def test_registers_and_no_lds_scratch_or_spills(isa):
    notes = kernel_notes(isa[1])
    for name, cap in [(instance(*i), VGPR_BUDGET) for i in INSTANCES] + \
                     [(gen_instance(*i), VGPR_CAP) for i in GEN_INSTANCES]:
        name, f = fields(notes, name)
        print(name, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"])
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert f.get("sgpr_spill_count", 0) == 0 and f["agpr_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] == 0, (name, f)  # ds_bpermute needs no LDS allocation
        assert f["vgpr_count"] <= cap, (name, f)


def stencil_loops(lines):
    """Op lists of the innermost loops that hold the stencil: the span of every
    backward branch (conditional or not) that holds lane moves and encloses no
    other such span.  (generation_loops of test_isa_batch_gen.py drops a span
    that encloses any branch target at all; the joint walk, left by a break at
    its top, is laid out around the target of a small block without a stencil.)"""
    spans = []
    for addr, _, text in lines:
        m = re.match(r"s_c?branch\w* (\d+)$", text)
        if m and int(m.group(1)) >= 0x8000:
            target = addr + 4 + 4 * (int(m.group(1)) - 0x10000)
            if any(op == "ds_bpermute_b32" for a, op, _ in lines if target <= a <= addr):
                spans.append((target, addr))
    inner = [(t, e) for t, e in spans if not any(t <= t2 and e2 <= e for t2, e2 in spans if (t2, e2) != (t, e))]
    return [[op for a, op, _ in lines if t <= a <= e] for t, e in sorted(set(inner))]


def check_loops(lines, w):
    ops_all = [op for _, op, _ in lines]
    assert "s_barrier" not in ops_all
    assert not any(op.startswith(("ds_read", "ds_write", "scratch_", "buffer_")) for op in ops_all)
    assert "s_endpgm" not in [op for ops in stencil_loops(lines) for op in ops]
    loops = stencil_loops(lines)
    for ops in loops:
        assert not any(op.startswith("ds_") and op != "ds_bpermute_b32" for op in ops)
        assert not any(op.startswith(("global_load", "flat_load", "s_load", "s_buffer_load")) for op in ops)
    moves = sorted(ops.count("ds_bpermute_b32") for ops in loops)
    shifts = sorted(ops.count("v_alignbit_b32") for ops in loops)
    # loops of one chain (detecting, advancing the copy, the rest; the compiler lays a recording loop out in two
    # versions here and there) and the one joint walk of two
    assert len(loops) >= 4 and moves == [4 * w] * (len(loops) - 1) + [8 * w], moves
    assert shifts == [2 * w] * (len(loops) - 1) + [4 * w], shifts
    return loops


@pytest.mark.parametrize("w,rule,pop", INSTANCES)
def test_generation_loops_of_the_two_state_forms(isa, w, rule, pop):
    loops = check_loops(lines_of(isa[0], instance(w, rule, pop)), w)
    if pop == "false":  # (a recording loop flushes its trace: stores, and no other memory access)
        for ops in loops:
            assert not any(op.startswith(("global_", "flat_")) for op in ops)
    else:
        for ops in loops:  # the search records nothing: the loops without the count of a generation hold no store
            if "v_bcnt_u32_b32" not in ops:
                assert not any(op.startswith(("global_", "flat_")) for op in ops)


@pytest.mark.parametrize("w,p", GEN_INSTANCES)
def test_generation_loops_of_the_generations_forms(isa, w, p):
    for ops in check_loops(lines_of(isa[0], gen_instance(w, p)), w):
        assert not any(op.startswith(("global_", "flat_")) for op in ops)
