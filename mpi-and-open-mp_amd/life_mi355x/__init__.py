"""life_mi355x -- Python binding of the MI355X Game-of-Life C ABI.

Mirrors the reference's per-rank interface (6-cartesian/life_cart.c:39-49):

=====================  ==============================================
reference              here
=====================  ==============================================
life_init (loader)     :func:`load_cfg` (cfg.py) + :class:`Life`
life_step              :meth:`Life.step`  (HIP kernels)
life_exchange          part of :meth:`Life.step` (RCCL / local halo)
life_collect           :meth:`Life.gather` (device-side gather)
life_save_vtk          :func:`save_vtk` (cfg.py)
decomposition          :func:`decomposition`
MPI_Dims_create        :func:`dims_create`
life_free              :meth:`Life.close`
=====================  ==============================================

The compute path is ``liblife_mi355x.so`` only: there is no CPU fallback.
Importing works without a GPU (host-only helpers such as
:func:`halo_plan` run anywhere); device calls raise :class:`LifeError` when
no HIP device is present.
"""
from __future__ import annotations

import collections
import ctypes
import importlib.abc
import os
import sys

import numpy as np

from .cfg import (bits_bytes, density_bytes, load_bits, load_bits_packed, load_cfg, load_cfg_cells,  # noqa: F401
                  load_density, save_vtk, vtk_bytes, vtk_header)

HERE = os.path.dirname(os.path.abspath(__file__))
# LIFE_MI355X_LIB: load another build of the same library (experiments only)
LIB_PATH = os.environ.get("LIFE_MI355X_LIB") or os.path.join(HERE, "liblife_mi355x.so")

KERNEL_BYTE = 0
KERNEL_BIT = 1
KERNELS = {"byte": KERNEL_BYTE, "bit": KERNEL_BIT}
XPORT_AUTO, XPORT_RCCL, XPORT_LOCAL = 0, 1, 2
HALO_SEND, HALO_RECV, HALO_FILL = 0, 1, 2
HALO_COLUMN, HALO_ROW, HALO_CORNER = 0, 1, 2
OPT_SMALL_GRID, OPT_OVERLAP, OPT_SMALL_WINDOW, OPT_BLOCK_GENS, OPT_LOOPBACK, OPT_FLOW = 1, 2, 4, 5, 6, 7
OPT_FLOW_CHUNK = 8
OPT_DEEP_HALO = 9
OPT_PIPELINE = 11  # 0 off, 1 automatic, 3..16 row regions per pass (LIFE_OPT_PIPELINE)
OPT_SKIP_DEAD = 12  # 0 off, 1 run only the tiles whose window may hold a live cell (LIFE_OPT_SKIP_DEAD)
OPT_POPULATION = 13  # 0 off, 1 record the population of every generation of a step call (LIFE_OPT_POPULATION)
OPT_RULE7 = 14  # B3/S23 in 7 gates per dword: RULE7_TILES | RULE7_FLOW, 0 the 8-gate kernels (LIFE_OPT_RULE7)
RULE7_TILES, RULE7_FLOW = 1, 2
# LIFE_TEMPORAL_DEPTH(_BYTE): generations per halo exchange of the temporal layouts
TEMPORAL_DEPTH = {"bit": 32, "byte": 32}
BLOCK_GENS = {"bit": 12, "byte": 32}  # tiles: default generations per launch at most (LIFE_OPT_BLOCK_GENS)
TEMPORAL_ROWS = {"bit": 24, "byte": 48}  # default register rows per wave (bit: 64-cell pair rows)
TILE_WAVES = {"bit": 8, "byte": 8}  # waves per tile workgroup (window = waves x rows)
TEMPORAL_XAPRON = {"bit": 64, "byte": 32}  # x-apron of the temporal layouts: one lane column
# VALU instructions per pair row and generation of the bit tiles under a rule other than B3/S23 (the table
# tail: 2 v_alignbit + 2 full adders + 2 x 25 v_bitop3; csrc/life_kernels.h kRuleValuPerPairRow) and under
# B3/S23; life_dev_kernel_work books them, tests/test_isa_rule.py and tests/test_isa.py pin them
RULE_VALU_PER_PAIR_ROW = 56
CONWAY_VALU_PER_PAIR_ROW = 22
# what the census instances of the bit tiles add per pair row and generation: two v_bcnt_u32_b32
# (csrc/life_kernels.h kPopValuPerPairRow, LIFE_OPT_POPULATION)
POP_VALU_PER_PAIR_ROW = 2
RULE_CONWAY = (1 << 3, (1 << 2) | (1 << 3))  # (birth, survive) masks of B3/S23

# Every symbol include/life_mi355x.h declares (checked by tests/test_abi.py).
ABI_SYMBOLS = (
    "life_decomposition", "life_dims_create", "life_dims_choose", "life_halo_plan", "life_layout_query",
    "life_strerror", "life_last_error", "life_dev_create", "life_dev_create_ex",
    "life_get_unique_id", "life_dev_create_rank", "life_dev_upload", "life_dev_fill_random",
    "life_dev_step", "life_dev_gather", "life_dev_live_count", "life_dev_sync",
    "life_dev_layout", "life_dev_world", "life_dev_set_timing", "life_dev_kernel_stats",
    "life_tune", "life_tune_temporal", "life_dev_configure", "life_dev_kernel_work", "life_dev_checksum",
    "life_dev_gather_vtk", "life_dev_gather_bits", "life_dev_destroy", "life_measure_copy", "life_dev_phase_stats",
    "life_dev_barrier", "life_device_count", "life_dev_last_path", "life_dev_call_stats",
    "life_dev_strerror", "life_dev_shard_info",
    "life_dev_clear", "life_dev_set_cells", "life_dev_gather_rect", "life_dev_gather_density",
    "life_dev_upload_bits", "life_dev_set_rect",
    "life_rule_parse", "life_rule_format", "life_dev_set_rule", "life_dev_get_rule",
    "life_dev_activity", "life_dev_population", "life_dev_last_rule_arm",
    "life_batch_query", "life_batch_create", "life_batch_destroy", "life_batch_upload", "life_batch_gather",
    "life_batch_fill_random", "life_batch_set_rule", "life_batch_get_rule", "life_batch_configure",
    "life_batch_step", "life_batch_census", "life_batch_settled", "life_batch_generation", "life_batch_sync",
    "life_batch_set_rules", "life_batch_get_rules", "life_batch_cycles",
    "life_rule_parse_gen", "life_rule_format_gen", "life_batch_set_rule_gen", "life_batch_get_rule_gen",
    "life_batch_set_rules_gen", "life_batch_get_rules_gen", "life_batch_upload_states", "life_batch_gather_states",
    "life_batch_census_gen", "life_batch_query_plan", "life_batch_population", "life_batch_onsets",
    "life_tile_decode_query",
)
GEN_MAX_STATES = 16  # LIFE_GEN_MAX_STATES
BATCH_TIER_WAVE, BATCH_TIER_GROUP = 1, 2  # LIFE_BATCH_TIER_*
BATCH_TIERS = {BATCH_TIER_WAVE: "wave", BATCH_TIER_GROUP: "group"}
BATCH_OPT_SETTLE = 1  # LIFE_BATCH_OPT_SETTLE
BATCH_OPT_CYCLE = 3  # LIFE_BATCH_OPT_CYCLE (2 is unassigned)
BATCH_OPT_POPULATION = 4  # LIFE_BATCH_OPT_POPULATION
BATCH_OPT_ONSET = 5  # LIFE_BATCH_OPT_ONSET
PATHS = {0: "none", 1: "onegen", 2: "tiles", 3: "flow", 5: "small", 6: "skip"}


class LifeError(RuntimeError):
    def __init__(self, rc: int, what: str):
        lib = _lib()
        detail = lib.life_last_error().decode(errors="replace")
        super().__init__(f"{what}: {lib.life_strerror(rc).decode()} ({rc}){': ' + detail if detail else ''}")
        self.rc = rc


class HaloOp(ctypes.Structure):
    _fields_ = [("phase", ctypes.c_int32), ("kind", ctypes.c_int32), ("peer", ctypes.c_int32),
                ("what", ctypes.c_int32), ("index", ctypes.c_int64), ("first", ctypes.c_int64),
                ("count", ctypes.c_int64), ("width", ctypes.c_int64)]

    def as_tuple(self):
        return (self.phase, self.kind, self.peer, self.what, self.index, self.first, self.count, self.width)


class Layout(ctypes.Structure):
    _fields_ = [("w", ctypes.c_int64), ("h", ctypes.c_int64), ("x0", ctypes.c_int64),
                ("y0", ctypes.c_int64), ("pitch", ctypes.c_int64), ("xoff", ctypes.c_int64),
                ("rows", ctypes.c_int64), ("units", ctypes.c_int64), ("xapron", ctypes.c_int64),
                ("yapron", ctypes.c_int64), ("kernel", ctypes.c_int32), ("coords", ctypes.c_int32 * 2),
                ("generations_per_exchange", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_LIB = None


class _TorchAfterLibraryGuard(importlib.abc.MetaPathFinder):
    """Refuses `import torch` once liblife_mi355x.so is loaded:
    the library binds /opt/rocm's libamdhip64.so.7; torch links its bundled HIP
    runtime by the unversioned name, so importing it afterwards maps a SECOND
    runtime into the process and it dies with a double free at exit.  With
    torch imported first, the library binds torch's runtime and all is well."""

    MESSAGE = ("life_mi355x: liblife_mi355x.so is already loaded with /opt/rocm's HIP runtime; importing torch now "
               "would map torch's bundled HIP runtime as a second copy (the process aborts with a double free at "
               "exit).  Import torch before the first life_mi355x device call, or not at all.")

    def find_spec(self, name, path, target=None):
        if name == "torch" or name.startswith("torch."):
            raise ImportError(self.MESSAGE)
        return None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is not built: run `make -C mpi-and-open-mp_amd` "
                              "or __graft_entry__.build()")
        if "torch" not in sys.modules and not any(isinstance(f, _TorchAfterLibraryGuard) for f in sys.meta_path):
            sys.meta_path.insert(0, _TorchAfterLibraryGuard())
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        i64, i32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
        P = ctypes.POINTER
        L.life_decomposition.argtypes = [i64, i32, i32, P(i64), P(i64)]
        L.life_decomposition.restype = None
        L.life_dims_create.argtypes = [i32, P(ctypes.c_int)]
        L.life_dims_create.restype = None
        L.life_dims_choose.argtypes = [i64, i64, i32, i32, P(ctypes.c_int)]
        L.life_halo_plan.argtypes = [i64, i64, i32, i32, i32, i32, P(HaloOp), i32]
        L.life_layout_query.argtypes = [i64, i64, i32, i32, i32, i32, P(Layout)]
        L.life_strerror.argtypes = [i32]
        L.life_strerror.restype = ctypes.c_char_p
        L.life_last_error.restype = ctypes.c_char_p
        L.life_dev_create.argtypes = [i64, i64, i32, i32, P(vp)]
        L.life_dev_create_ex.argtypes = [i64, i64, i32, i32, i32, i32, i32, P(vp)]
        L.life_get_unique_id.argtypes = [ctypes.c_char_p]
        L.life_dev_create_rank.argtypes = [i64, i64, i32, i32, i32, i32, i32, ctypes.c_char_p, i32, P(vp)]
        L.life_dev_upload.argtypes = [vp, P(ctypes.c_uint8)]
        L.life_dev_fill_random.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32]
        L.life_dev_step.argtypes = [vp, i64]
        L.life_dev_gather.argtypes = [vp, P(ctypes.c_uint8)]
        L.life_dev_gather_vtk.argtypes = [vp, ctypes.c_char_p]
        L.life_dev_gather_bits.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8)]
        L.life_dev_clear.argtypes = [vp]
        L.life_dev_set_cells.argtypes = [vp, P(i64), i64, i32]
        L.life_dev_gather_rect.argtypes = [vp, i64, i64, i64, i64, P(ctypes.c_uint8)]
        L.life_dev_gather_density.argtypes = [vp, i64, i64, P(ctypes.c_uint32)]
        L.life_dev_upload_bits.argtypes = [vp, P(ctypes.c_uint8)]
        L.life_dev_set_rect.argtypes = [vp, i64, i64, i64, i64, P(ctypes.c_uint8)]
        L.life_dev_live_count.argtypes = [vp]
        L.life_dev_live_count.restype = i64
        L.life_dev_sync.argtypes = [vp]
        L.life_dev_barrier.argtypes = [vp]
        L.life_device_count.argtypes = []
        L.life_dev_last_path.argtypes = [vp]
        L.life_dev_checksum.argtypes = [vp, P(ctypes.c_uint64)]
        L.life_dev_layout.argtypes = [vp, i32, P(Layout)]
        L.life_dev_world.argtypes = [vp] + [P(ctypes.c_int)] * 5
        L.life_dev_set_timing.argtypes = [vp, i32]
        L.life_dev_configure.argtypes = [vp, i32, i32]
        L.life_dev_kernel_stats.argtypes = [vp, P(ctypes.c_double), P(i64), P(ctypes.c_double)]
        L.life_dev_kernel_work.argtypes = [vp, P(ctypes.c_double), P(ctypes.c_double)]
        L.life_dev_phase_stats.argtypes = [vp] + [P(ctypes.c_double)] * 4 + [P(i64)]
        if hasattr(L, "life_dev_call_stats"):  # absent from pre-round-4 builds (LIFE_MI355X_LIB A/B runs)
            L.life_dev_call_stats.argtypes = [vp, P(ctypes.c_double), P(ctypes.c_double), P(i64), P(ctypes.c_double)]
        if hasattr(L, "life_dev_shard_info"):  # absent from pre-round-6 builds (LIFE_MI355X_LIB A/B runs)
            L.life_dev_shard_info.argtypes = [vp, i32, P(ctypes.c_int), ctypes.c_char_p, P(ctypes.c_int)]
        if hasattr(L, "life_dev_set_rule"):  # absent from builds that predate rules (LIFE_MI355X_LIB A/B runs)
            u32 = ctypes.c_uint32
            L.life_rule_parse.argtypes = [ctypes.c_char_p, P(u32), P(u32)]
            L.life_rule_format.argtypes = [u32, u32, ctypes.c_char_p]
            L.life_dev_set_rule.argtypes = [vp, u32, u32]
            L.life_dev_get_rule.argtypes = [vp, P(u32), P(u32)]
        if hasattr(L, "life_dev_activity"):  # absent from builds that predate LIFE_OPT_SKIP_DEAD (A/B runs)
            L.life_dev_activity.argtypes = [vp] + [P(i64)] * 4
        if hasattr(L, "life_dev_population"):  # absent from builds that predate LIFE_OPT_POPULATION (A/B runs)
            L.life_dev_population.argtypes = [vp, P(i64), i64, P(i64)]
        if hasattr(L, "life_dev_last_rule_arm"):  # absent from builds that predate LIFE_OPT_RULE7 (A/B runs)
            L.life_dev_last_rule_arm.argtypes = [vp]
        if hasattr(L, "life_batch_create"):  # absent from builds that predate batches (LIFE_MI355X_LIB A/B runs)
            u32, u64 = ctypes.c_uint32, ctypes.c_uint64
            L.life_batch_query.argtypes = [i64, i64, P(ctypes.c_int), P(i64)]
            L.life_batch_create.argtypes = [i64, i64, i64, i32, P(vp)]
            L.life_batch_destroy.argtypes = [vp]
            L.life_batch_destroy.restype = None
            L.life_batch_upload.argtypes = [vp, i64, i64, P(ctypes.c_uint8)]
            L.life_batch_gather.argtypes = [vp, i64, i64, P(ctypes.c_uint8)]
            L.life_batch_fill_random.argtypes = [vp, u64, u32]
            L.life_batch_set_rule.argtypes = [vp, u32, u32]
            L.life_batch_get_rule.argtypes = [vp, P(u32), P(u32)]
            L.life_batch_configure.argtypes = [vp, i32, i32]
            L.life_batch_step.argtypes = [vp, i64]
            L.life_batch_census.argtypes = [vp, P(i64), P(u64)]
            L.life_batch_settled.argtypes = [vp, P(i64)]
            L.life_batch_generation.argtypes = [vp, P(i64)]
            L.life_batch_sync.argtypes = [vp]
        if hasattr(L, "life_batch_set_rules"):  # absent from builds that predate per-universe rules
            L.life_batch_set_rules.argtypes = [vp, i64, i64, P(u32), P(u32)]
            L.life_batch_get_rules.argtypes = [vp, i64, i64, P(u32), P(u32)]
            L.life_batch_cycles.argtypes = [vp, P(i64), P(i64)]
        if hasattr(L, "life_batch_set_rule_gen"):  # absent from builds that predate Generations rules
            u8 = ctypes.c_uint8
            L.life_rule_parse_gen.argtypes = [ctypes.c_char_p, P(u32), P(u32), P(u32)]
            L.life_rule_format_gen.argtypes = [u32, u32, u32, ctypes.c_char_p]
            L.life_batch_set_rule_gen.argtypes = [vp, u32, u32, u32]
            L.life_batch_get_rule_gen.argtypes = [vp, P(u32), P(u32), P(u32)]
            L.life_batch_set_rules_gen.argtypes = [vp, i64, i64, P(u32), P(u32), P(u32)]
            L.life_batch_get_rules_gen.argtypes = [vp, i64, i64, P(u32), P(u32), P(u32)]
            L.life_batch_upload_states.argtypes = [vp, i64, i64, P(u8)]
            L.life_batch_gather_states.argtypes = [vp, i64, i64, P(u8)]
            L.life_batch_census_gen.argtypes = [vp, P(i64), P(i64), P(u64)]
        if hasattr(L, "life_batch_population"):  # absent from builds that predate population traces
            L.life_batch_population.argtypes = [vp, i64, i64, P(u32), P(i64)]
        if hasattr(L, "life_batch_onsets"):  # absent from builds that predate cycle onsets
            L.life_batch_onsets.argtypes = [vp, P(i64)]
        if hasattr(L, "life_batch_query_plan"):  # absent from builds that predate it
            L.life_batch_query_plan.argtypes = [i64, i64] + [P(ctypes.c_int)] * 6
        L.life_tune.argtypes = [i32, i32, i32]
        L.life_tune_temporal.argtypes = [i32, i32]
        L.life_measure_copy.argtypes = [i32, i64, i32, P(ctypes.c_double)]
        L.life_dev_destroy.argtypes = [vp]
        L.life_dev_destroy.restype = None
        _LIB = L
    return _LIB


# Test hook: a byte value that fresh gather destinations are filled with
# before the device copy (None: np.empty).  tests/conftest.py sets 0xA5, so a
# copy that did not land shows up as poison instead of as a plausible grid.
GATHER_FILL = None


def _host_buffer(shape) -> np.ndarray:
    if GATHER_FILL is None:
        return np.empty(shape, dtype=np.uint8)
    return np.full(shape, GATHER_FILL, dtype=np.uint8)


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise LifeError(rc, what)
    return rc


def kernel_id(kernel) -> int:
    if isinstance(kernel, str):
        return KERNELS[kernel]
    return int(kernel)


# ---------------------------------------------------------------- host only
def decomposition(n: int, p: int, k: int):
    """life_cart.c:217-223 -> (start, stop)."""
    s, e = ctypes.c_int64(), ctypes.c_int64()
    _lib().life_decomposition(n, p, k, ctypes.byref(s), ctypes.byref(e))
    return s.value, e.value


def dims_create(n: int):
    """MPI_Dims_create(n, 2, {0,0}) (life_cart.c:117-118)."""
    d = (ctypes.c_int * 2)()
    _lib().life_dims_create(n, d)
    return d[0], d[1]


PARTITIONS = {"cart": 0, "rows": 1, "cols": 2, "auto": 3}  # LIFE_PARTITION_*


def dims_choose(nx: int, ny: int, n: int, policy="auto"):
    """Partition shape for n shards (life_dims_choose): "cart" =
    MPI_Dims_create, "rows" = {1, n} strips, "cols" = {n, 1}, "auto"."""
    d = (ctypes.c_int * 2)()
    pol = PARTITIONS[policy] if isinstance(policy, str) else int(policy)
    _check(_lib().life_dims_choose(nx, ny, n, pol, d), "life_dims_choose")
    return d[0], d[1]


def halo_plan(nx: int, ny: int, dims, rank: int, kernel="byte"):
    """The per-exchange halo ops of shard `rank` (see life_halo_plan)."""
    ops = (HaloOp * 16)()
    n = _check(_lib().life_halo_plan(nx, ny, dims[0], dims[1], rank, kernel_id(kernel), ops, 16),
               "life_halo_plan")
    return [ops[i].as_tuple() for i in range(n)]


def layout_query(nx: int, ny: int, dims, rank: int, kernel="byte") -> Layout:
    L = Layout()
    _check(_lib().life_layout_query(nx, ny, dims[0], dims[1], rank, kernel_id(kernel), ctypes.byref(L)),
           "life_layout_query")
    return L


def parse_rule(text: str):
    """(birth, survive) masks of a rulestring (life_rule_parse): "B36/S23" in
    either letter case, or Golly's "23/3" (S/B).  Bit k of birth: a dead cell
    with k live neighbours is born; of survive: a live one stays alive."""
    b, s = ctypes.c_uint32(), ctypes.c_uint32()
    _check(_lib().life_rule_parse(str(text).encode(), ctypes.byref(b), ctypes.byref(s)), "life_rule_parse")
    return b.value, s.value


def format_rule(birth: int, survive: int) -> str:
    """The canonical "B.../S..." of two 9-bit masks (life_rule_format)."""
    if not (0 <= int(birth) < 2**32 and 0 <= int(survive) < 2**32):
        raise ValueError(f"rule masks {birth}, {survive} are not 32-bit")
    out = ctypes.create_string_buffer(24)
    _check(_lib().life_rule_format(int(birth), int(survive), out), "life_rule_format")
    return out.value.decode()


def _rule_masks(rule):
    """A rulestring or a (birth, survive) pair -> the pair."""
    if isinstance(rule, str):
        try:
            return parse_rule(rule)
        except LifeError as e:
            try:
                states = parse_rule_gen(rule)[2]
            except LifeError:
                raise e from None
            raise LifeError(e.rc, f"rule {rule!r} is a Generations rule of {states} states: those run on wave-tier "
                                  "batches only (LifeBatch), not on Life") from None
    birth, survive = rule
    return int(birth), int(survive)


def parse_rule_gen(text: str):
    """(birth, survive, states) of a Generations rulestring (life_rule_parse_gen):
    what :func:`parse_rule` accepts (states = 2), "B2/S345/C4" (G for C, either
    letter case) and Golly's "345/2/4" (S/B/C), 2 <= states <= 16."""
    b, s, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(_lib().life_rule_parse_gen(str(text).encode(), ctypes.byref(b), ctypes.byref(s), ctypes.byref(c)),
           "life_rule_parse_gen")
    return b.value, s.value, c.value


def format_rule_gen(birth: int, survive: int, states: int = 2) -> str:
    """The canonical "B.../S.../Cn" (life_rule_format_gen); for two states
    what :func:`format_rule` gives."""
    if not all(0 <= int(v) < 2**32 for v in (birth, survive, states)):
        raise ValueError(f"rule masks {birth}, {survive} or state count {states} are not 32-bit")
    out = ctypes.create_string_buffer(32)
    _check(_lib().life_rule_format_gen(int(birth), int(survive), int(states), out), "life_rule_format_gen")
    return out.value.decode()


def _rule_triple(rule):
    """A rulestring, a (birth, survive) pair or a (birth, survive, states)
    triple -> the triple (a pair has two states)."""
    if isinstance(rule, str):
        return parse_rule_gen(rule)
    rule = tuple(int(v) for v in rule)
    if len(rule) == 2:
        return rule + (2,)
    birth, survive, states = rule
    return birth, survive, states


def batch_query(nx: int, ny: int):
    """(tier, bytes per universe) of a batch of nx x ny universes
    (life_batch_query, no GPU needed): tier "wave" (one universe per wave, 1 <=
    nx <= 128, 1 <= ny <= 64) or "group" (one per workgroup, the shapes of the
    small-grid register kernel); LifeError for a shape in neither."""
    tier, nbytes = ctypes.c_int(), ctypes.c_int64()
    _check(_lib().life_batch_query(int(nx), int(ny), ctypes.byref(tier), ctypes.byref(nbytes)), "life_batch_query")
    return BATCH_TIERS[tier.value], nbytes.value


BatchPlan = collections.namedtuple("BatchPlan", "tier words lanes_per_strip rows strips threads")


def batch_plan(nx: int, ny: int) -> BatchPlan:
    """The kernel instance and launch of a batch of nx x ny universes
    (life_batch_query_plan, no GPU needed): ``tier`` as :func:`batch_query`,
    ``words`` per row, ``threads`` of a workgroup, and on the group tier the
    ``lanes_per_strip`` (``words`` rounded up to a power of two), the strip
    height ``rows`` and the ``strips`` = ny / rows of a universe (0 on the wave
    tier); LifeError for a shape in neither."""
    out = [ctypes.c_int() for _ in range(6)]
    _check(_lib().life_batch_query_plan(int(nx), int(ny), *map(ctypes.byref, out)), "life_batch_query_plan")
    return BatchPlan(BATCH_TIERS[out[0].value], *(v.value for v in out[1:]))


def density_to_thr(density: float) -> int:
    return min(int(density * 2.0**32), 0xFFFFFFFF)


def tune_temporal(rows: int = 0, kernel=-1) -> None:
    """Temporal tile height: register rows per wave of one encoding (bit:
    16/24 pair rows; byte: 32/48 word rows), or of both
    (kernel -1: each takes the value if valid for it)."""
    _check(_lib().life_tune_temporal(kernel_id(kernel), rows), "life_tune_temporal")


def tune(rows: int = 0, depth: int = 0, kernel=-1) -> None:
    """Stencil rows-per-lane / prefetch depth for this process (life_tune)."""
    _check(_lib().life_tune(kernel_id(kernel), rows, depth), "life_tune")


def measure_copy(device: int = 0, nbytes: int = 2 << 30, reps: int = 5) -> float:
    """Measured HBM copy ceiling in GB/s (read + write bytes / best time)."""
    g = ctypes.c_double()
    _check(_lib().life_measure_copy(device, nbytes, reps, ctypes.byref(g)), "life_measure_copy")
    return g.value


def unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(_lib().life_get_unique_id(buf), "life_get_unique_id")
    return buf.raw


# ---------------------------------------------------------------- device
class Life:
    """A periodic nx x ny Game of Life resident in MI355X HBM.

    ``Life(nx, ny, shards=1, kernel="bit")`` drives ``shards`` Cartesian
    blocks from this process (one per GPU, or several logical shards on one
    GPU with the LOCAL transport).  :meth:`for_rank` is the
    one-process-per-GPU form (torchrun), with RCCL between ranks.
    """

    def __init__(self, nx: int, ny: int, shards: int = 1, kernel="bit", dims=(0, 0),
                 transport: int = XPORT_AUTO, small_grid: bool = True, overlap: bool = True, flow=None,
                 window=None, rule=None, skip_dead: bool = False, population: bool = False, _handle=None):
        self.nx, self.ny = int(nx), int(ny)
        self.kernel = kernel_id(kernel)
        self._h = ctypes.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _check(_lib().life_dev_create_ex(self.nx, self.ny, shards, dims[0], dims[1], self.kernel,
                                             transport, ctypes.byref(self._h)), "life_dev_create")
        # small_grid: True/"auto" (VGPR kernel when the shape allows, else LDS),
        # "lds" (LDS kernel only), "window" (the VGPR kernel windowed over
        # several CUs where the shape allows, else as True; True windows only
        # shapes whose one-workgroup strips would be >= 4 rows tall), "vgpr1"
        # (as True, never windowed), False (the streaming kernels);
        # window=(R, K): the windowed kernel's strip height and halo rows
        mode = {True: 1, "auto": 1, "lds": 2, "window": 3, "vgpr1": 4, False: 0}[small_grid]
        if mode != 1:
            self.configure(OPT_SMALL_GRID, mode)
        if window is not None:
            self.configure(OPT_SMALL_WINDOW, int(window[0]) * 256 + int(window[1]))
        if not overlap:
            self.configure(OPT_OVERLAP, 0)
        # flow: None (library default 3: the dataflow tiles where a pass is
        # only a few rounds of workgroups), or a LIFE_OPT_FLOW value (0: one
        # launch per pass)
        if flow is not None:
            self.configure(OPT_FLOW, int(flow))
        # rule: None (B3/S23), a rulestring or a (birth, survive) pair (set_rule)
        if rule is not None:
            self.set_rule(rule)
        # skip_dead: run only the tiles whose window may hold a live cell
        # (LIFE_OPT_SKIP_DEAD; no effect on devices that do not qualify)
        if skip_dead:
            self.configure(OPT_SKIP_DEAD, 1)
        # population: every step call records the live cells after each of its
        # generations (LIFE_OPT_POPULATION; population() reads them)
        if population:
            self.configure(OPT_POPULATION, 1)

    def configure(self, option: int, value: int) -> None:
        _check(_lib().life_dev_configure(self._h, option, value), "configure")

    def set_rule(self, rule) -> None:
        """life_dev_set_rule: the Life-like rule of the following steps, a
        rulestring ("B36/S23", "23/36") or a (birth, survive) pair of 9-bit
        masks.  Bit encoding only (the byte encoding runs B3/S23), no B0
        rules; the state is untouched.  Under a rule other than B3/S23 the
        per-launch tiles and the one-generation kernel run (no dataflow or
        small-grid kernels)."""
        birth, survive = _rule_masks(rule)
        if not (0 <= birth < 2**32 and 0 <= survive < 2**32):
            raise ValueError(f"rule masks {birth}, {survive} are not 32-bit")
        _check(_lib().life_dev_set_rule(self._h, birth, survive), "set_rule")

    @property
    def rule(self) -> str:
        """The current rule's canonical string (life_dev_get_rule)."""
        b, s = ctypes.c_uint32(), ctypes.c_uint32()
        _check(_lib().life_dev_get_rule(self._h, ctypes.byref(b), ctypes.byref(s)), "get_rule")
        return format_rule(b.value, s.value)

    @classmethod
    def for_rank(cls, nx, ny, rank, world, uid: bytes, device: int, kernel="bit", dims=(0, 0)):
        h = ctypes.c_void_p()
        _check(_lib().life_dev_create_rank(nx, ny, kernel_id(kernel), rank, world, dims[0], dims[1],
                                           uid, device, ctypes.byref(h)), "life_dev_create_rank")
        return cls(nx, ny, kernel=kernel, _handle=h)

    # life_init's cell loading (life_cart.c:104-109)
    def upload(self, grid: np.ndarray) -> None:
        g = np.ascontiguousarray(grid, dtype=np.uint8)
        if g.shape != (self.ny, self.nx):
            raise ValueError(f"grid shape {g.shape} != ({self.ny}, {self.nx})")
        _check(_lib().life_dev_upload(self._h, g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "upload")

    def fill_random(self, seed: int, density: float = 0.5) -> None:
        _check(_lib().life_dev_fill_random(self._h, seed, density_to_thr(density)), "fill_random")

    # sparse I/O: no nx*ny host grid (life_dev_clear / set_cells / gather_rect / gather_density)
    def clear(self) -> None:
        """Every cell dead (== upload of an all-zero grid)."""
        _check(_lib().life_dev_clear(self._h), "clear")

    def set_cells(self, cells, alive: bool = True) -> None:
        """The listed (x, y) cells become alive (or dead); coordinates wrap
        periodically, duplicates are allowed, other cells are untouched."""
        c = np.ascontiguousarray(np.asarray(cells, dtype=np.int64))
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError(f"set_cells: cells must have shape (n, 2), not {c.shape}")
        _check(_lib().life_dev_set_cells(self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), c.shape[0],
                                         1 if alive else 0), "set_cells")

    def upload_bits(self, packed: np.ndarray) -> None:
        """life_dev_upload_bits, the inverse of :meth:`gather_bits`: the whole
        state from packed rows, a uint8 (ny, ceil(nx/8)) array with cell x at
        bit x & 7 of byte x >> 3 (np.packbits(grid, axis=1,
        bitorder="little")); a row's bits at and beyond nx are ignored."""
        p = np.asarray(packed)
        if p.dtype != np.uint8 or p.shape != (self.ny, (self.nx + 7) // 8):
            raise ValueError(f"upload_bits: packed must be uint8 of shape ({self.ny}, {(self.nx + 7) // 8}), "
                             f"not {p.dtype} {p.shape}")
        p = np.ascontiguousarray(p)
        _check(_lib().life_dev_upload_bits(self._h, p.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "upload_bits")

    def set_rect(self, x0: int, y0: int, cells) -> None:
        """life_dev_set_rect, the inverse of :meth:`gather_rect`: cell
        ((x0 + i) mod nx, (y0 + j) mod ny) becomes cells[j, i] != 0 for the
        (h, w) integer or bool array `cells`; other cells are untouched."""
        c = np.asarray(cells)
        if c.ndim != 2 or not (np.issubdtype(c.dtype, np.integer) or c.dtype == np.bool_):
            raise ValueError(f"set_rect: cells must be a 2-D integer or bool array, not {c.dtype} {c.shape}")
        # uint8 goes as it is (the library takes any nonzero byte as alive); wider values must not be cut to 8 bits
        c = np.ascontiguousarray(c if c.dtype == np.uint8 else c != 0, dtype=np.uint8)
        _check(_lib().life_dev_set_rect(self._h, int(x0), int(y0), c.shape[1], c.shape[0],
                                        c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "set_rect")

    def gather_rect(self, x0: int, y0: int, w: int, h: int, out: np.ndarray | None = None) -> np.ndarray:
        """The periodic w x h window at (x0, y0) as an (h, w) uint8 array:
        out[j, i] is cell ((x0 + i) mod nx, (y0 + j) mod ny)."""
        w, h = int(w), int(h)
        if out is None:
            out = _host_buffer((max(h, 0), max(w, 0)))
        if out.shape != (max(h, 0), max(w, 0)) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("gather_rect: out must be a C-contiguous uint8 (h, w) array")
        _check(_lib().life_dev_gather_rect(self._h, int(x0), int(y0), w, h,
                                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "gather_rect")
        return out

    def gather_density(self, fx: int, fy: int | None = None) -> np.ndarray:
        """Block-summed live counts: a (ceil(ny/fy), ceil(nx/fx)) uint32 array,
        bin [by, bx] counting the live cells with x // fx == bx, y // fy == by."""
        fx = int(fx)
        fy = fx if fy is None else int(fy)
        # factors the library rejects (LIFE_EINVAL) have no map shape: it never writes
        shape = (-(-self.ny // fy), -(-self.nx // fx)) if fx >= 1 and fy >= 1 else (1, 1)
        out = _host_buffer(shape + (4,)).view(np.uint32).reshape(shape)
        _check(_lib().life_dev_gather_density(self._h, fx, fy, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
               "gather_density")
        return out

    def step(self, generations: int = 1) -> None:
        _check(_lib().life_dev_step(self._h, generations), "step")

    def gather(self, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = _host_buffer((self.ny, self.nx))
        _check(_lib().life_dev_gather(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "gather")
        return out

    def gather_vtk(self) -> bytes:
        """life_dev_gather_vtk: the whole VTK file of the current grid, with
        the cell text formatted on the device (== save_vtk of gather())."""
        body = ctypes.create_string_buffer(2 * self.nx * self.ny)
        _check(_lib().life_dev_gather_vtk(self._h, body), "gather_vtk")
        return vtk_header(self.nx, self.ny) + body.raw

    def gather_bits(self, out: np.ndarray | None = None) -> np.ndarray:
        """life_dev_gather_bits: packed rows (ny x ceil(nx/8) bytes, cell x at
        bit x & 7 of byte x >> 3; == np.packbits(gather(), axis=1,
        bitorder="little")), packed on the device."""
        if out is None:
            out = _host_buffer((self.ny, (self.nx + 7) // 8))
        if out.shape != (self.ny, (self.nx + 7) // 8) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("gather_bits: out must be a C-contiguous uint8 (ny, ceil(nx/8)) array")
        _check(_lib().life_dev_gather_bits(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "gather_bits")
        return out

    def live_count(self) -> int:
        return _check(_lib().life_dev_live_count(self._h), "live_count")

    def checksum(self) -> int:
        """life_dev_checksum: encoding- and partition-independent grid hash."""
        v = ctypes.c_uint64()
        _check(_lib().life_dev_checksum(self._h, ctypes.byref(v)), "checksum")
        return v.value

    def sync(self) -> None:
        _check(_lib().life_dev_sync(self._h), "sync")

    def barrier(self) -> None:
        """life_dev_barrier: sync, then (rank mode) an all-reduce every rank joins."""
        _check(_lib().life_dev_barrier(self._h), "barrier")

    def layout(self, local_shard: int = 0) -> Layout:
        L = Layout()
        _check(_lib().life_dev_layout(self._h, local_shard, ctypes.byref(L)), "layout")
        return L

    def world(self):
        v = [ctypes.c_int() for _ in range(5)]
        _check(_lib().life_dev_world(self._h, *[ctypes.byref(x) for x in v]), "world")
        return dict(zip(("world", "dims0", "dims1", "nlocal", "transport"), (x.value for x in v)))

    def shard_info(self, local_shard: int = 0):
        """life_dev_shard_info: {"device", "pci_bus_id", "rccl_nranks"} of a
        local shard (rccl_nranks 0: no communicator); None from builds that
        predate it."""
        if not hasattr(_lib(), "life_dev_shard_info"):
            return None
        dev, n = ctypes.c_int(), ctypes.c_int()
        bus = ctypes.create_string_buffer(64)
        _check(_lib().life_dev_shard_info(self._h, local_shard, ctypes.byref(dev), bus, ctypes.byref(n)),
               "shard_info")
        return {"device": dev.value, "pci_bus_id": bus.value.decode(errors="replace"), "rccl_nranks": n.value}

    def set_timing(self, on) -> None:
        """life_dev_set_timing: False off, True launch timing + phase events,
        2 launch timing only (no event packets inside a partitioned step)."""
        _check(_lib().life_dev_set_timing(self._h, int(on)), "set_timing")

    def last_path(self) -> str:
        """Kernel family of the last step call (life_dev_last_path)."""
        return PATHS[_check(_lib().life_dev_last_path(self._h), "last_path")]

    def last_rule7(self) -> int:
        """The forms (RULE7_TILES | RULE7_FLOW) of which a launch of the last step call ran the 7-gate
        arm of the B3/S23 bit tiles (life_dev_last_rule_arm); 0: every launch ran the 8-gate kernels."""
        return _check(_lib().life_dev_last_rule_arm(self._h), "last_rule7")

    def activity(self):
        """(passes, tiles_run, tiles_cleared, tiles_total) summed over the
        skip-dead passes of the last step call (life_dev_activity; blocking);
        zeros when it ran none."""
        v = [ctypes.c_int64() for _ in range(4)]
        _check(_lib().life_dev_activity(self._h, *[ctypes.byref(x) for x in v]), "activity")
        return tuple(x.value for x in v)

    def population(self) -> np.ndarray:
        """The live cells of the whole grid after each generation of the last
        step call (life_dev_population; blocking): an int64 array, empty when
        that call recorded nothing (LIFE_OPT_POPULATION off, step(0), no call)."""
        n = ctypes.c_int64()
        _check(_lib().life_dev_population(self._h, None, 0, ctypes.byref(n)), "population")
        out = np.zeros(n.value, dtype=np.int64)
        if n.value:
            _check(_lib().life_dev_population(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n.value,
                                              None), "population")
        return out

    def flow_active(self) -> bool:
        return self.last_path() == "flow"

    def kernel_stats(self):
        ms, n, b = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _check(_lib().life_dev_kernel_stats(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(b)),
               "kernel_stats")
        return ms.value, n.value, b.value

    def kernel_work(self):
        """(cell-updates, VALU lane-ops) per timed launch (life_dev_kernel_work)."""
        u, v = ctypes.c_double(), ctypes.c_double()
        _check(_lib().life_dev_kernel_work(self._h, ctypes.byref(u), ctypes.byref(v)), "kernel_work")
        return u.value, v.value

    def phase_stats(self):
        """Mean ms per overlapped block of the ring, interior, halo exchange
        and whole block, and the number of blocks (life_dev_phase_stats)."""
        v = [ctypes.c_double() for _ in range(4)]
        n = ctypes.c_int64()
        _check(_lib().life_dev_phase_stats(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(n)), "phase_stats")
        return dict(zip(("ring_ms", "interior_ms", "halo_ms", "block_ms"), (x.value for x in v)), blocks=n.value)

    def call_stats(self):
        """Where the last step call's time went (life_dev_call_stats, timing
        on): host enqueue ms (whole call, longest pass), passes, device span
        ms (first work start to last work end, max over local shards)."""
        h, pm, sp = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int64()
        if not hasattr(_lib(), "life_dev_call_stats"):
            return {"host_enqueue_ms": 0.0, "pass_enqueue_max_ms": 0.0, "passes": 0, "device_span_ms": 0.0}
        _check(_lib().life_dev_call_stats(self._h, ctypes.byref(h), ctypes.byref(pm), ctypes.byref(n),
                                          ctypes.byref(sp)), "call_stats")
        return {"host_enqueue_ms": h.value, "pass_enqueue_max_ms": pm.value, "passes": n.value,
                "device_span_ms": sp.value}

    def close(self) -> None:
        if self._h:
            _lib().life_dev_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LifeBatch:
    """``count`` independent periodic nx x ny universes on one GPU, advanced
    together by one launch per :meth:`step` (life_batch_*).

    Every call is ordered on the batch's one stream: ``step`` returns at once,
    and a following ``gather`` / ``live_counts`` / ``checksums`` / ``settled``
    waits for it.  ``rule``: None (B3/S23), a rulestring or a (birth, survive)
    pair (wave tier only); a Generations rule ("B2/S/C3", a (birth, survive,
    states) triple) gives every cell up to 16 states, moved by
    :meth:`upload_states` / :meth:`gather_states`.  ``rules``: one such rule per universe
    (:meth:`set_rules`; wave tier only).  ``settle``: stop a universe early once
    it repeats with period 1 or 2 (LIFE_BATCH_OPT_SETTLE; wave tier only).
    ``cycle``: find cycles of any period instead (LIFE_BATCH_OPT_CYCLE,
    :meth:`cycles`; wave tier only, not together with ``settle``).  ``onset``:
    with ``cycle``, also the exact generation at which each universe entered
    its cycle (LIFE_BATCH_OPT_ONSET, :meth:`onsets`).
    ``population``: record every universe's live cells after each generation
    of a :meth:`step` call (LIFE_BATCH_OPT_POPULATION, :meth:`population`;
    DESIGN.md §5.14; both tiers, two-state rules only)."""

    def __init__(self, nx: int, ny: int, count: int, device: int = 0, rule=None, settle: bool = False, rules=None,
                 cycle: bool = False, population: bool = False, onset: bool = False):
        self.nx, self.ny, self.count = int(nx), int(ny), int(count)
        self._h = ctypes.c_void_p()
        _check(_lib().life_batch_create(self.nx, self.ny, self.count, int(device), ctypes.byref(self._h)),
               "life_batch_create")
        self.tier = batch_query(self.nx, self.ny)[0]
        if rule is not None:
            self.set_rule(rule)
        if rules is not None:
            self.set_rules(rules)
        if settle:
            self.configure(BATCH_OPT_SETTLE, 1)
        if cycle:
            self.configure(BATCH_OPT_CYCLE, 1)
        if onset:
            self.configure(BATCH_OPT_ONSET, 1)
        if population:
            self.configure(BATCH_OPT_POPULATION, 1)

    def configure(self, option: int, value: int) -> None:
        _check(_lib().life_batch_configure(self._h, int(option), int(value)), "life_batch_configure")

    def set_rule(self, rule) -> None:
        """life_batch_set_rule: what :meth:`Life.set_rule` accepts, and
        Generations rules ("B2/S/C3", a (birth, survive, states) triple: life_
        batch_set_rule_gen); a rule other than B3/S23 needs a wave-tier batch.
        Clears every settled flag and resets every dying cell to dead."""
        birth, survive, states = _rule_triple(rule)
        if not all(0 <= v < 2**32 for v in (birth, survive, states)):
            raise ValueError(f"rule masks {birth}, {survive} or state count {states} are not 32-bit")
        if states > 2:
            _check(_lib().life_batch_set_rule_gen(self._h, birth, survive, states), "life_batch_set_rule_gen")
        else:
            _check(_lib().life_batch_set_rule(self._h, birth, survive), "life_batch_set_rule")

    @property
    def rule(self) -> str:
        """The one rule of a uniform batch, with /Cn where it has more than two
        states; LifeError (LIFE_ESTATE) once :meth:`set_rules` gave the
        universes rules of their own (see ``rules``)."""
        b, s, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(_lib().life_batch_get_rule_gen(self._h, ctypes.byref(b), ctypes.byref(s), ctypes.byref(c)),
               "life_batch_get_rule_gen")
        return format_rule_gen(b.value, s.value, c.value)

    def set_rules(self, rules, first: int = 0) -> None:
        """life_batch_set_rules: universes [first, first + len(rules)) take
        ``rules``, a sequence of rulestrings, (birth, survive) pairs or (birth,
        survive, states) triples; the others keep theirs.  Clears the settled and
        cycle flags of those universes and resets their dying cells to dead.
        The batch steps a rule per universe until :meth:`set_rule`.  Where an
        entry has more than two states the call is life_batch_set_rules_gen."""
        masks = [_rule_triple(r) for r in rules]
        for birth, survive, states in masks:
            if not all(0 <= v < 2**32 for v in (birth, survive, states)):
                raise ValueError(f"rule masks {birth}, {survive} or state count {states} are not 32-bit")
        birth = np.array([m[0] for m in masks], dtype=np.uint32)
        survive = np.array([m[1] for m in masks], dtype=np.uint32)
        states = np.array([m[2] for m in masks], dtype=np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if (states > 2).any():
            _check(_lib().life_batch_set_rules_gen(self._h, int(first), len(masks), birth.ctypes.data_as(u32p),
                                                   survive.ctypes.data_as(u32p), states.ctypes.data_as(u32p)),
                   "life_batch_set_rules_gen")
        else:
            _check(_lib().life_batch_set_rules(self._h, int(first), len(masks), birth.ctypes.data_as(u32p),
                                               survive.ctypes.data_as(u32p)), "life_batch_set_rules")

    def rule_masks(self, first: int = 0, n: int | None = None):
        """(birth, survive) uint32 arrays of universes [first, first + n)
        (life_batch_get_rules; n None: all from `first` on)."""
        first = int(first)
        n = self.count - first if n is None else int(n)
        birth, survive = np.zeros(max(n, 0), dtype=np.uint32), np.zeros(max(n, 0), dtype=np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        _check(_lib().life_batch_get_rules(self._h, first, n, birth.ctypes.data_as(u32p),
                                           survive.ctypes.data_as(u32p)), "life_batch_get_rules")
        return birth, survive

    def rule_triples(self, first: int = 0, n: int | None = None):
        """(birth, survive, states) uint32 arrays of universes [first, first +
        n) (life_batch_get_rules_gen; n None: all from `first` on)."""
        first = int(first)
        n = self.count - first if n is None else int(n)
        birth, survive, states = (np.zeros(max(n, 0), dtype=np.uint32) for _ in range(3))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        _check(_lib().life_batch_get_rules_gen(self._h, first, n, birth.ctypes.data_as(u32p),
                                               survive.ctypes.data_as(u32p), states.ctypes.data_as(u32p)),
               "life_batch_get_rules_gen")
        return birth, survive, states

    @property
    def rules(self) -> list:
        """The canonical rulestring of every universe (with /Cn where it has
        more than two states)."""
        return [format_rule_gen(int(b), int(s), int(c)) for b, s, c in zip(*self.rule_triples())]

    @property
    def states(self) -> np.ndarray:
        """The state count of every universe (uint32, count entries)."""
        return self.rule_triples()[2]

    @property
    def generation(self) -> int:
        """Generations stepped since the states were last written as a whole."""
        g = ctypes.c_int64()
        _check(_lib().life_batch_generation(self._h, ctypes.byref(g)), "life_batch_generation")
        return g.value

    def upload(self, grids, first: int = 0) -> None:
        """Universes [first, first + n) from an (n, ny, nx) array (nonzero = alive)."""
        g = np.asarray(grids)
        if g.ndim != 3 or g.shape[1:] != (self.ny, self.nx):
            raise ValueError(f"upload: grids shape {g.shape} != (n, {self.ny}, {self.nx})")
        g = np.ascontiguousarray(g if g.dtype == np.uint8 else g != 0, dtype=np.uint8)
        _check(_lib().life_batch_upload(self._h, int(first), g.shape[0],
                                        g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "life_batch_upload")

    def gather(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """Universes [first, first + n) as an (n, ny, nx) uint8 array of 0 / 1
        (n None: all from `first` on)."""
        first = int(first)
        n = self.count - first if n is None else int(n)
        out = _host_buffer((max(n, 0), self.ny, self.nx))
        _check(_lib().life_batch_gather(self._h, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
               "life_batch_gather")
        return out

    def upload_states(self, grids, first: int = 0) -> None:
        """Universes [first, first + n) from an (n, ny, nx) array of cell states
        (0 dead, 1 alive, 2 .. C - 1 dying; life_batch_upload_states): every value
        must be below the state count of its universe."""
        g = np.asarray(grids)
        if g.ndim != 3 or g.shape[1:] != (self.ny, self.nx):
            raise ValueError(f"upload_states: grids shape {g.shape} != (n, {self.ny}, {self.nx})")
        if g.size and (g.min() < 0 or g.max() > 255):
            raise ValueError("upload_states: cell states are 0 .. 255")
        g = np.ascontiguousarray(g, dtype=np.uint8)
        _check(_lib().life_batch_upload_states(self._h, int(first), g.shape[0],
                                               g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
               "life_batch_upload_states")

    def gather_states(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """Universes [first, first + n) as an (n, ny, nx) uint8 array of cell
        states (n None: all from `first` on)."""
        first = int(first)
        n = self.count - first if n is None else int(n)
        out = _host_buffer((max(n, 0), self.ny, self.nx))
        _check(_lib().life_batch_gather_states(self._h, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
               "life_batch_gather_states")
        return out

    def census_gen(self):
        """(live, dying, checksum) of every universe (life_batch_census_gen):
        the cells in state 1, the cells in states >= 2 (int64), and the sum of
        state x mix64(y nx + x + 1) over all cells modulo 2^64 (uint64)."""
        live, dying = np.zeros(self.count, dtype=np.int64), np.zeros(self.count, dtype=np.int64)
        sums = np.zeros(self.count, dtype=np.uint64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        _check(_lib().life_batch_census_gen(self._h, live.ctypes.data_as(i64p), dying.ctypes.data_as(i64p),
                                            sums.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
               "life_batch_census_gen")
        return live, dying, sums

    def dying_counts(self) -> np.ndarray:
        """The dying cells (state >= 2) of every universe (int64, count entries)."""
        return self.census_gen()[1]

    def state_checksums(self) -> np.ndarray:
        """The checksum over the whole state of every universe (uint64): equal
        to :meth:`checksums` where nothing is dying."""
        return self.census_gen()[2]

    def fill_random(self, seed: int, density: float = 0.5) -> None:
        """Universe u becomes what ``Life.fill_random(seed + u, density)`` gives
        an nx x ny grid (seed + u modulo 2^64); nothing is dying."""
        _check(_lib().life_batch_fill_random(self._h, int(seed) % 2**64, density_to_thr(density)),
               "life_batch_fill_random")

    def step(self, generations: int = 1) -> None:
        _check(_lib().life_batch_step(self._h, int(generations)), "life_batch_step")

    def live_counts(self) -> np.ndarray:
        """The live cells of every universe (int64, count entries)."""
        out = np.zeros(self.count, dtype=np.int64)
        _check(_lib().life_batch_census(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None),
               "life_batch_census")
        return out

    def checksums(self) -> np.ndarray:
        """``oracle.checksum`` of every universe (uint64, count entries)."""
        out = np.zeros(self.count, dtype=np.uint64)
        _check(_lib().life_batch_census(self._h, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
               "life_batch_census")
        return out

    def settled(self) -> np.ndarray:
        """Per universe the generation at which settle detection found it
        repeating with period 1 or 2, -1 where it has not (int64)."""
        out = np.zeros(self.count, dtype=np.int64)
        _check(_lib().life_batch_settled(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
               "life_batch_settled")
        return out

    def cycles(self):
        """(period, generation) int64 arrays of LIFE_BATCH_OPT_CYCLE: per
        universe the exact period it was found to repeat with and the generation
        it was found at; 0 and -1 where none was found."""
        period, found = np.zeros(self.count, dtype=np.int64), np.zeros(self.count, dtype=np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        _check(_lib().life_batch_cycles(self._h, period.ctypes.data_as(i64p), found.ctypes.data_as(i64p)),
               "life_batch_cycles")
        return period, found

    def onsets(self) -> np.ndarray:
        """Per universe the generation at which its orbit entered the cycle
        that :meth:`cycles` reports (LIFE_BATCH_OPT_ONSET, life_batch_onsets):
        max(true onset, the generation the finding :meth:`step` call began at);
        -1 where none was recorded (int64)."""
        out = np.zeros(self.count, dtype=np.int64)
        _check(_lib().life_batch_onsets(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
               "life_batch_onsets")
        return out

    def population(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """The population trace of the last :meth:`step` call with
        LIFE_BATCH_OPT_POPULATION on (life_batch_population): an (n, G) uint32
        array, entry [k, g] the live cells of universe first + k after
        generation g + 1 of that call (n None: all from `first` on).  G is the
        call's generation count; 0 with the option off, after ``step(0)`` and
        before any call."""
        first = int(first)
        n = self.count - first if n is None else int(n)
        gens = ctypes.c_int64()
        _check(_lib().life_batch_population(self._h, first, n, None, ctypes.byref(gens)), "life_batch_population")
        out = np.zeros((max(n, 0), gens.value), dtype=np.uint32)
        _check(_lib().life_batch_population(self._h, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                            None), "life_batch_population")
        return out

    def sync(self) -> None:
        _check(_lib().life_batch_sync(self._h), "life_batch_sync")

    def close(self) -> None:
        if self._h:
            _lib().life_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
