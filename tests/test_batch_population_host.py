"""Batch population traces, host side (no GPU): the option
and its readout are in the header and the binding, and the entry cap is
stated in the header once."""
import inspect
import os
import re

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "life_mi355x.h")


def test_header_and_binding_agree_on_the_option(lm):
    header = open(HEADER).read()
    assert re.search(r"#define LIFE_BATCH_OPT_POPULATION (\d+)", header).group(1) == str(lm.BATCH_OPT_POPULATION) == "4"
    options = re.findall(r"#define LIFE_BATCH_OPT_\w+ (\d+)", header)
    assert sorted(options) == ["1", "3", "4"]  # 2 stays unassigned, 0 invalid, and no number is used twice


def test_the_readout_is_exported_and_declared(lm):
    assert "life_batch_population" in declared_functions()
    assert "life_batch_population" in lm.ABI_SYMBOLS
    assert getattr(lm._lib(), "life_batch_population") is not None
    header = open(HEADER).read()
    assert re.search(r"int life_batch_population\(life_batch \*b, int64_t first, int64_t n, uint32_t \*counts,\s*"
                     r"int64_t \*generations\);", header)
    assert "population" in inspect.signature(lm.LifeBatch.__init__).parameters
    assert list(inspect.signature(lm.LifeBatch.population).parameters) == ["self", "first", "n"]


def test_the_entry_cap_is_stated_once():
    header = open(HEADER).read()
    assert header.count("2^30") == 1
    kernels = open(os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc", "life_batch_kernels.h")).read()
    assert re.search(r"kBatchTraceEntries = \(int64_t\)1 << 30;", kernels)
