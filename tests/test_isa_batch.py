"""Static guards on the batch unit's gfx950 code object (CPU only): what
DESIGN.md §5.11 claims of the wave tier -- no scratch, a generation loop with
no barrier and no LDS traffic other than the lane moves, 4 ds_bpermute per
word, and registers for 8 waves per SIMD."""
import os
import re
import subprocess

import pytest

from test_isa import LLVM, ROOT, kernel_lines

OBJ = os.path.join(ROOT, "mpi-and-open-mp_amd", "build", "life_batch_kernels.hip.o")
INSTANCES = [(w, rule, settle) for w in (1, 2, 3, 4) for rule in ("ConwayRule", "TableRule")
             for settle in ("true", "false")]
VGPR_BUDGET = 64  # min(8, 512 // allocation) waves per SIMD: 8 up to 64 registers


def instance(w, rule, settle):
    return f"batch_wave_kernel<{w}, life::{rule}, {settle}>"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("built object or llvm-objdump missing")
    d = tmp_path_factory.mktemp("isa_batch")
    fat, co = str(d / "fat.bin"), str(d / "k.co")
    subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fat}", OBJ], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True,
                         check=True).stdout
    dis = subprocess.run(["c++filt"], input=dis, capture_output=True, text=True).stdout
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    return dis, notes


def kernel_notes(notes):
    """{demangled name: {field: int}} of every kernel of the code object."""
    out = {}
    for block in re.split(r"\n(?=\s+- \.agpr_count)", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        out[dem] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    return out


def generation_loops(lines):
    """Op lists of the loops (bodies of backward branches) that hold the stencil."""
    out = []
    for addr, op, text in lines:
        m = re.match(r"s_cbranch_\w+ (\d+)$", text)
        if not m or int(m.group(1)) < 0x8000:
            continue
        target = addr + 4 + 4 * (int(m.group(1)) - 0x10000)
        ops = [o for a, o, _ in lines if target <= a <= addr]
        if "v_bitop3_b32" in ops:
            out.append(ops)
    return out


def test_every_instance_is_built(isa):
    names = kernel_notes(isa[1])
    for inst in INSTANCES:
        assert any(instance(*inst) in n for n in names), instance(*inst)


def test_no_scratch_and_eight_waves_per_simd(isa):
    notes = kernel_notes(isa[1])
    seen = 0
    for name, f in notes.items():
        if "batch_" not in name:
            continue
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        if "batch_wave_kernel" in name:
            seen += 1
            assert f["vgpr_count"] <= VGPR_BUDGET and f["agpr_count"] == 0, (name, f)
            assert f["group_segment_fixed_size"] == 0, (name, f)  # ds_bpermute needs no LDS allocation
    assert seen == len(INSTANCES)


@pytest.mark.parametrize("w,rule,settle", INSTANCES)
def test_generation_loop_has_no_barrier_and_no_lds_exchange(isa, w, rule, settle):
    lines = kernel_lines(isa[0], instance(w, rule, settle))
    ops_all = [op for _, op, _ in lines]
    assert "s_barrier" not in ops_all  # the waves of a workgroup never meet
    assert not any(op.startswith(("ds_read", "ds_write", "scratch_", "buffer_")) for op in ops_all)
    loops = generation_loops(lines)
    assert loops, "no generation loop found"
    for ops in loops:
        assert not any(op.startswith("ds_") and op != "ds_bpermute_b32" for op in ops)
        assert not any(op.startswith(("global_", "flat_")) for op in ops)  # no memory traffic per generation
    # the loop of whole generations: 4 lane moves and 2 funnel shifts per word
    full = max(loops, key=len)
    assert full.count("ds_bpermute_b32") == 4 * w
    assert full.count("v_alignbit_b32") == 2 * w
