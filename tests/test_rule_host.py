"""Life-like rules, host side (no GPU): the rulestring parser and formatter
(life_rule_parse / life_rule_format), the lane-uniform words the table-rule
kernels take (life::rule_words, csrc/life_plan.cpp, linked alone with g++ as
tests/test_host_plan.py does) checked by evaluating the kernel's boolean
construction (TableRule, csrc/life_bitops.h) in numpy over every adder
output, and the numpy reference the GPU rule tests lean on, pinned to the
oracle at B3/S23."""
import os
import re
import subprocess

import numpy as np
import pytest

import rule_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-and-open-mp_amd", "csrc")

NAMED_TEXT = ["B3/S23", "B36/S23", "B3678/S34678", "B2/S", "B1357/S1357", "B3/S012345678"]


@pytest.mark.parametrize("text", NAMED_TEXT)
def test_named_rules_round_trip(lm, text):
    birth, survive = lm.parse_rule(text)
    assert (birth, survive) == R.NAMED[text]
    assert lm.format_rule(birth, survive) == text
    assert lm.parse_rule(text.lower()) == (birth, survive)


def test_other_forms(lm):
    assert lm.parse_rule("23/3") == R.CONWAY  # Golly's S/B
    assert lm.parse_rule("23/36") == R.NAMED["B36/S23"]
    assert lm.parse_rule("/2") == R.NAMED["B2/S"]
    assert lm.parse_rule("b3/S23") == lm.parse_rule("B3/s23") == R.CONWAY
    assert lm.parse_rule("B63/S3322") == R.NAMED["B36/S23"]  # any order, repeats
    assert lm.format_rule(*lm.parse_rule("B63/S3322")) == "B36/S23"
    assert lm.parse_rule("B/S") == (0, 0) and lm.format_rule(0, 0) == "B/S"
    assert lm.format_rule(0x1FF, 0x1FF) == "B012345678/S012345678"
    assert lm.RULE_CONWAY == R.CONWAY


@pytest.mark.parametrize("text", ["B9/S2", "B3S23", "", "nonsense", "B3/S23 ", "3/2/1", "S23/B3x"])
def test_rejected_text(lm, text):
    with pytest.raises(lm.LifeError) as e:
        lm.parse_rule(text)
    assert e.value.rc == -1  # LIFE_EINVAL
    assert f'"{text}"' in str(e.value)  # the message quotes the text


def test_format_rejects_high_bits(lm):
    with pytest.raises(lm.LifeError) as e:
        lm.format_rule(1 << 9, 0)
    assert e.value.rc == -1


HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include "life_host.h"
int main(int argc, char **argv) {
    // rules as "birth survive" pairs: one line of the 20 words a[0][0..4] a[1][0..4] b[0][0..4] b[1][0..4]
    for (int k = 1; k + 1 < argc; k += 2) {
        const life::RuleWords w = life::rule_words((uint32_t)atoi(argv[k]), (uint32_t)atoi(argv[k + 1]));
        for (int q = 0; q < 10; q++) printf("%u ", w.a[q / 5][q % 5]);
        for (int q = 0; q < 10; q++) printf("%u ", w.b[q / 5][q % 5]);
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def words_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("rule_words")
    (d / "h.cpp").write_text(HARNESS)
    exe = str(d / "h")
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", str(d / "h.cpp"),
                    os.path.join(CSRC, "life_plan.cpp"), "-o", exe], check=True)

    def run(rules):
        args = [str(v) for r in rules for v in r]
        out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.splitlines()
        words = [np.array(ln.split(), dtype=np.uint64).astype(np.uint32) for ln in out]
        return [(w[:10].reshape(2, 5), w[10:].reshape(2, 5)) for w in words]

    return run


def sample_rules():
    rng = np.random.default_rng(20240)
    pairs = [(int(b) & ~1, int(s)) for b, s in rng.integers(0, 512, size=(64, 2))]
    return pairs + R.conway_flips()


def mux(a, b, c):
    return (a & b) | (~a & c)


def table_tail(A, B, a0, a1, b0, b1, c0, c1, alive):
    """TableRule::operator() of csrc/life_bitops.h, word for word."""
    u0, k0 = a0 ^ b0 ^ c0, (a0 & b0) | (a0 & c0) | (b0 & c0)
    v0, v1 = a1 ^ b1 ^ c1, (a1 & b1) | (a1 & c1) | (b1 & c1)
    L = [mux(alive, (u0 & A[1][s]) ^ B[1][s], (u0 & A[0][s]) ^ B[0][s]) for s in range(5)]
    x = v0 ^ k0
    lo = mux(x, L[1], mux(v0, L[2], L[0]))
    hi = mux(x, L[3], mux(v0, L[4], L[2]))
    return mux(v1, hi, lo)


def test_rule_words_give_the_table(words_of):
    """Every rule of the sample; every (alive, three row sums) case -- all
    2 x 9 (alive, neighbours) pairs through every adder output that makes
    them: lane k of the test words is one case, as a lane's bit is one cell."""
    cases = [(al, ra, rb, rc) for al in (0, 1) for ra in range(4) for rb in range(al, 4) for rc in range(4)]
    assert {(al, ra + rb + rc - al) for al, ra, rb, rc in cases} == R.ALL_PAIRS | {(0, 9)}

    def word(bits):  # bit k of the word = case k (several words: 112 cases)
        bits = np.array(bits, dtype=np.uint64)
        return np.array([sum(int(b) << i for i, b in enumerate(bits[j:j + 32])) for j in range(0, len(bits), 32)],
                        dtype=np.uint32)

    alive = word([c[0] for c in cases])
    rows = [(word([c[i] & 1 for c in cases]), word([c[i] >> 1 for c in cases])) for i in (1, 2, 3)]
    rules = sample_rules()
    assert len(rules) == 64 + 17 and all(not b & 1 for b, _ in rules)
    for (birth, survive), (A, B) in zip(rules, words_of(rules)):
        assert set(np.unique(np.concatenate([A.ravel(), B.ravel()]))) <= {0, 0xFFFFFFFF}
        got = table_tail(A, B, rows[0][0], rows[0][1], rows[1][0], rows[1][1], rows[2][0], rows[2][1], alive)
        for k, (al, ra, rb, rc) in enumerate(cases):
            n8 = ra + rb + rc - al
            if n8 > 8:
                continue  # a dead cell among 9 live ones of 9: cannot occur
            want = ((survive if al else birth) >> n8) & 1
            assert (int(got[k // 32]) >> (k % 32)) & 1 == want, (birth, survive, al, ra, rb, rc)


@pytest.mark.parametrize("nx,ny", [(17, 3), (65, 65), (200, 70)])
def test_numpy_reference_is_the_oracle_at_conway(oracle, nx, ny):
    grid = oracle.fill_random(nx, ny, 11, 0.5)
    np.testing.assert_array_equal(R.rule_run(grid, 7, R.CONWAY), oracle.life_run(grid, 7))


def test_valu_constant_is_the_kernels(lm):
    """The binding's RULE_VALU_PER_PAIR_ROW is the constant life_dev_kernel_work
    books (csrc/life_kernels.h); tests/test_isa_rule.py pins it to the code."""
    text = open(os.path.join(CSRC, "life_kernels.h")).read()
    assert int(re.search(r"kRuleValuPerPairRow = (\d+);", text).group(1)) == lm.RULE_VALU_PER_PAIR_ROW
