"""The bit tile's window load and store outside the generation loop (CPU only,
the built gfx950 code object; fixture and helpers of tests/test_isa.py).

A plain tile's wave decides once whether its 24 window rows cross the periodic
seam and whether it stores all 24 (LIFE_TILE_STRAIGHT, tile_body_bit): when
they do not / it does, the loads and the stores are 24 instructions in one
basic block each, the row base walked by the pitch in scalar registers.

Before (the per-row walk: a 64-bit compare-and-select for the y wrap between
the loads, two range branches around every store): in both kernels the plain
tile's 24 loads sat in one block among 210 other instructions (the banded
item's among 233), and no basic block held more than one store.  Now: the
straight block holds the 24 loads and 10 other instructions (the per-row walk
stays for the seam, 24 + 208), and one block of 51 instructions holds the 24
stores.  The whole kernel went from 6453 / 6593 instructions (7-gate /
8-gate) to 4857 / 4997.
"""
import re

import pytest

from test_isa import isa, kernel_lines  # noqa: F401  (the module-scoped fixture)

KERNELS = ["tstep_bit7_kernel<24, true, true, 8>", "tstep_bit_kernel<24, true, true, 8>"]
ROWS = 24


def basic_blocks(lines):
    """The kernel's instructions cut at every branch (a block ends with it)
    and at every branch target (a block starts there)."""
    targets = set()
    for addr, op, text in lines:
        m = re.match(r"s_cbranch_\w+ (\d+)$|s_branch (\d+)$", text)
        if m:
            simm = int(m.group(1) or m.group(2))
            targets.add(addr + 4 + 4 * (simm - 0x10000 if simm >= 0x8000 else simm))
    blocks, cur = [], []
    for addr, op, text in lines:
        if addr in targets and cur:
            blocks.append(cur)
            cur = []
        cur.append(op)
        if op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm", "s_setpc_b64"):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    return blocks


@pytest.mark.parametrize("kernel", KERNELS)
def test_window_load_is_one_block(isa, kernel):
    blocks = basic_blocks(kernel_lines(isa[0], kernel))
    found = [len(b) - ROWS for b in blocks if b.count("global_load_dwordx2") == ROWS]
    print(f"{kernel}: blocks with {ROWS} loads, other instructions in each: {found}")
    assert found, "no basic block holds the 24 window loads"
    assert min(found) <= 4 * ROWS, found


@pytest.mark.parametrize("kernel", KERNELS)
def test_window_store_is_one_block(isa, kernel):
    blocks = basic_blocks(kernel_lines(isa[0], kernel))
    found = [len(b) for b in blocks if b.count("global_store_dwordx2") == ROWS]
    print(f"{kernel}: blocks with {ROWS} stores, instructions in each: {found}")
    assert found, "no basic block holds the 24 row stores"
