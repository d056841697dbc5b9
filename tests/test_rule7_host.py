"""B3/S23 in 7 gates (ConwayRule7, csrc/life_bitops.h), host side (no GPU):
the host evaluator life::conway7_host (csrc/life_plan.cpp, linked alone with
g++ as tests/test_rule_host.py does) equals the rule's definition on all 128
inputs -- the two bits of each of three rows' horizontal sums and the cell --
and the immediates it runs on are the ones the header names, which the device
policy uses by those names."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")

HARNESS = r"""
#include <stdio.h>
#include "life_host.h"
int main() {
    // input k (0..127): bit 0 a0, 1 a1, 2 b0, 3 b1, 4 c0, 5 c1, 6 alive; lane j of word w is input 32 w + j
    for (int w = 0; w < 4; w++) {
        uint32_t in[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < 32; j++)
            for (int b = 0; b < 7; b++)
                if (((32 * w + j) >> b) & 1) in[b] |= 1u << j;
        printf("%u\n", life::conway7_host(in[0], in[1], in[2], in[3], in[4], in[5], in[6]));
    }
    printf("%u %u %u %u %u\n", life::kR7Par, life::kR7Nae, life::kR7G1, life::kR7G2, life::kR7Out);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("rule7")
    (d / "h.cpp").write_text(HARNESS)
    exe = str(d / "h")
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", str(d / "h.cpp"),
                    os.path.join(CSRC, "life_plan.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    return [int(v) for v in out[:4]], [int(v) for v in out[4:]]


def want(k):
    a, b, c, alive = k & 3, (k >> 2) & 3, (k >> 4) & 3, k >> 6
    n9 = a + b + c  # the three rows' 3-cell sums: the cell included
    return int(n9 == 3 or (alive and n9 == 4))


def test_host_evaluator_is_the_rule_on_all_128_inputs(harness):
    words, _ = harness
    got = [(words[k // 32] >> (k % 32)) & 1 for k in range(128)]
    assert got == [want(k) for k in range(128)]


def header_immediates():
    text = open(os.path.join(CSRC, "life_host.h")).read()
    return [int(re.search(rf"constexpr uint32_t {n} = (0x[0-9A-Fa-f]+);", text).group(1), 16)
            for n in ("kR7Par", "kR7Nae", "kR7G1", "kR7G2", "kR7Out")]


def b3(imm, a, b, c):
    """v_bitop3_b32 on one bit: the truth table indexed by (a, b, c), a the most significant."""
    return (imm >> ((a << 2) | (b << 1) | c)) & 1


def test_the_circuit_on_the_header_immediates(harness):
    """The circuit as csrc/life_bitops.h writes it, on the immediates read from
    the header's text: the rule on all 128 inputs, and the evaluator's own."""
    par, nae, g1i, g2i, outi = header_immediates()
    assert harness[1] == [par, nae, g1i, g2i, outi]
    for k in range(128):
        a0, a1, b0, b1, c0, c1, alive = ((k >> i) & 1 for i in range(7))
        p, n = b3(par, a0, b0, c0), b3(nae, a0, b0, c0)
        x, y = b3(par, a1, b1, c1), b3(nae, a1, b1, c1)
        g1 = b3(g1i, p, n, y)
        g2 = b3(g2i, n, x, g1)
        assert b3(outi, p, alive, g2) == want(k), k


def test_device_policy_uses_the_named_immediates():
    """ConwayRule7 spells no immediate of its own: each gate is one of the header's names."""
    text = open(os.path.join(CSRC, "life_bitops.h")).read()
    body = text[text.index("struct ConwayRule7"):]
    body = body[:body.index("};")]
    assert re.findall(r"b3<(\w+)>", body) == ["kR7Par", "kR7Nae", "kR7Par", "kR7Nae", "kR7G1", "kR7G2", "kR7Out"]
    src = open(os.path.join(CSRC, "life_plan.cpp")).read()
    host = src[src.index("life::conway7_host"):]
    host = host[:host.index("\n}")]
    assert re.findall(r"bitop3_host\((\w+),", host) == ["kR7Par", "kR7Nae", "kR7Par", "kR7Nae", "kR7G1", "kR7G2", "kR7Out"]
