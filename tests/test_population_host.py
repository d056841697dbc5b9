"""LIFE_OPT_POPULATION, the parts that need no GPU: the header declares the
option and the reader, the binding lists and exports them, and the op-count
model of the census instances (csrc/life_kernels.h kPopValuPerPairRow; DESIGN.md
5.10: two v_bcnt_u32_b32 per pair row and generation) is what the binding and
the built code object say."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "life_mi355x.h")
KERNELS_H = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc", "life_kernels.h")
OBJ = os.path.join(ROOT, "mpi-and-open-mp_amd", "build", "life_kernels.hip.o")
LLVM = "/opt/rocm/lib/llvm/bin"


def test_header_declares_the_option_and_the_reader():
    text = open(HEADER).read()
    assert re.search(r"^#define LIFE_OPT_POPULATION 13$", text, re.M)
    assert re.search(r"^int life_dev_population\(life_dev \*d, int64_t \*counts, int64_t max, int64_t \*generations\);$",
                     text, re.M)


def test_binding_exports(lm):
    assert "life_dev_population" in lm.ABI_SYMBOLS
    assert lm.OPT_POPULATION == 13
    assert hasattr(lm._lib(), "life_dev_population")
    assert callable(lm.Life.population)


def test_census_op_model(lm):
    """tstep_valu_per_tile_lane(m, pop) - tstep_valu_per_tile_lane(m) = waves x rows x kPopValuPerPairRow x m:
    the constant is the binding's, and the header's."""
    text = open(KERNELS_H).read()
    assert int(re.search(r"constexpr int kPopValuPerPairRow = (\d+);", text).group(1)) == lm.POP_VALU_PER_PAIR_ROW == 2
    assert "bool pop = false" in re.search(r"double tstep_valu_per_tile_lane\([^;]*;", text).group(0)


def test_census_instance_counts_two_ops_per_pair_row():
    """The built census instance of the 65536^2 tile: its generation loop holds the plain tile's 480 v_bitop3
    and 48 more v_bcnt_u32_b32 (24 pair rows x 2), nothing spilled inside it."""
    if not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("built object or llvm-objdump missing")
    import tempfile

    import test_isa

    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fat}", OBJ], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True,
                             check=True).stdout
    dis = subprocess.run(["c++filt"], input=dis, capture_output=True, text=True).stdout
    lines = test_isa.kernel_lines(dis, "tpop_bit_kernel<24, true, true, 8>")
    loops = []
    for addr, op, text in lines:
        m = re.match(r"s_cbranch_\w+ (\d+)$", text)
        if not m or int(m.group(1)) < 0x8000:
            continue
        target = addr + 4 + 4 * (int(m.group(1)) - 0x10000)
        ops = [o for a, o, _ in lines if target <= a <= addr]
        if "s_barrier" in ops and ops.count("v_bitop3_b32") == 480:
            loops.append(ops)
    assert loops, "no full-height generation loop in the census instance"
    for ops in loops:
        assert ops.count("v_bcnt_u32_b32") == 48
        assert not any(o.startswith("scratch_") for o in ops)
