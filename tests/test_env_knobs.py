"""The environment knobs of the runtime live in one table
(mpi-and-open-mp_amd/csrc/life_env.h), checked on the CPU:

* no other file under csrc/ calls getenv;
* INTEGRATION.md "Environment knobs" lists exactly the table's names, and the
  knobs that were settled and removed appear in neither;
* the three readers (a g++ harness including life_env.h, run as child
  processes): unset, valid, out of range and non-numeric values of one
  integer, one flag and one real knob; the value-set check life_plan.cpp
  keeps on top of the reader for LIFE_TEMPORAL_DEPTH(_BYTE), through
  life_layout_query.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")
REMOVED = {"LIFE_STREAM_PRIORITY", "LIFE_JOIN", "LIFE_TAIL_C", "LIFE_FLOW_AUTO_ROUNDS", "LIFE_FLOW_MIN_PASSES",
           "LIFE_TILE_WAVES"}


def table_names():
    """Names of the knob definitions in life_env.h: the quoted name that opens a Knob's braces."""
    src = open(os.path.join(CSRC, "life_env.h")).read()
    return re.findall(r'^constexpr \w+Knob \w+\{"(LIFE_[A-Z0-9_]+)"', src, re.M)


def test_getenv_only_in_life_env():
    hits = [f for f in sorted(os.listdir(CSRC)) if "getenv" in open(os.path.join(CSRC, f)).read()]
    assert hits == ["life_env.h"]


def test_table_matches_integration_md():
    names = table_names()
    assert len(names) == len(set(names)) and len(names) >= 20
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc[doc.index("Environment knobs"):]
    rows = re.findall(r"^\| `(LIFE_[A-Z0-9_]+)` \|", section, re.M)
    assert len(rows) == len(set(rows))
    assert set(rows) == set(names)
    assert not REMOVED & set(names) and not REMOVED & set(rows)
    # and no source file still reads a removed name
    for f in os.listdir(CSRC):
        text = open(os.path.join(CSRC, f)).read()
        assert not [n for n in REMOVED if re.search(rf"\b{n}\b", text)], f


HARNESS = r"""
#include <stdio.h>
#include "life_env.h"
#include "life_mi355x.h"
int main() {
    using namespace life::env;
    life_layout bit, byte;
    if (life_layout_query(256, 256, 1, 1, 0, LIFE_KERNEL_BIT, &bit) != LIFE_OK) return 1;
    if (life_layout_query(256, 256, 1, 1, 0, LIFE_KERNEL_BYTE, &byte) != LIFE_OK) return 1;
    printf("%d %d %g %d %d %d\n", read(kBlockGens), read(kBands), read(kCommTimeoutS), read(kXcdOrderOnegen),
           bit.generations_per_exchange, byte.generations_per_exchange);
    return 0;
}
"""


@pytest.fixture(scope="module")
def env_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("env")
    (d / "h.cpp").write_text(HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    str(d / "h.cpp"), os.path.join(CSRC, "life_plan.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def read(exe, **env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("LIFE_")}
    out = subprocess.run([exe], env=dict(base, **env), capture_output=True, text=True, check=True).stdout.split()
    return dict(block_gens=int(out[0]), bands=int(out[1]), timeout=float(out[2]), onegen=int(out[3]),
                depth=int(out[4]), depth_byte=int(out[5]))


def test_defaults(env_exe):
    assert read(env_exe) == dict(block_gens=0, bands=1, timeout=600.0, onegen=-1, depth=32, depth_byte=32)


@pytest.mark.parametrize("text,want", [("1", 1), ("12", 12), ("32", 32),  # the range's ends and inside
                                       ("0", 0), ("33", 0), ("-4", 0), ("many", 0), ("", 0)])
def test_int_knob(env_exe, text, want):
    assert read(env_exe, LIFE_BLOCK_GENS=text)["block_gens"] == want


@pytest.mark.parametrize("text,want", [("0", 0), ("1", 1), ("7", 1), ("-1", 1), ("off", 0), ("", 0)])
def test_flag_knob(env_exe, text, want):
    """A set flag is atoi(value) != 0: there is no out-of-range value, and text atoi cannot read is 0."""
    assert read(env_exe, LIFE_BANDS=text)["bands"] == want
    assert read(env_exe, LIFE_XCD_ORDER_ONEGEN=text)["onegen"] == want  # set: 0 / 1, never the unset -1


@pytest.mark.parametrize("text,want", [("2.5", 2.5), ("30", 30.0), ("0", 600.0), ("-3", 600.0), ("soon", 600.0)])
def test_real_knob(env_exe, text, want):
    assert read(env_exe, LIFE_COMM_TIMEOUT_S=text)["timeout"] == want


@pytest.mark.parametrize("text,want", [("12", 12), ("8", 8), ("1", 1), ("13", 32), ("64", 32), ("deep", 32)])
def test_temporal_depth_value_set(env_exe, text, want):
    got = read(env_exe, LIFE_TEMPORAL_DEPTH=text)
    assert got["depth"] == want and got["depth_byte"] == 32


@pytest.mark.parametrize("text,want", [("16", 16), ("1", 1), ("32", 32), ("8", 32), ("12", 32), ("24", 32), ("13", 32)])
def test_temporal_depth_byte_value_set(env_exe, text, want):
    got = read(env_exe, LIFE_TEMPORAL_DEPTH_BYTE=text)
    assert got["depth_byte"] == want and got["depth"] == 32
