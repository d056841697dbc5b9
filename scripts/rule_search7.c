// rule_search7.c -- exhaustive search for the tail of the B3/S23 rule over EVERY 2-bit encoding of
// the two column sums, not only the full adder's.  Tool, not product code.
//   gcc -O2 -fopenmp scripts/rule_search7.c -o scripts/rule_search7 && scripts/rule_search7
//
// Three rows' horizontal sums (s0 + 2 s1 each) give W0 = a0 + b0 + c0 and W1 = a1 + b1 + c1, both
// 0..3, and n9 = W0 + 2 W1; alive' = (n9 == 3) | (alive & n9 == 4).  A v_bitop3 of (a, b, c) can
// give any symmetric bit of W: up to complement there are three that split 0..3 into two pairs --
//   P parity (0xF0 ^ 0xCC ^ 0xAA = 0x96): {1,3},  M majority (0xE8): {2,3},  N not-all-equal (0x7E): {1,2}
// -- and any two of them encode W injectively at the price of the full adder (P, M): two gates per
// group.  scripts/rule_search.c fixed (P, M) x (P, M) and found no 3-gate tail.  Here: all nine
// pairs of encodings, tails of three gates and of two, over the five signals (two bits of W0, two
// of W1, alive).  A tail's last gate is decided by its inputs (rows with equal inputs must agree
// on the target); its immediate is printed with unreachable input combinations as 0.
//
// Circuits are counted up to complement of the inner gates (an inner gate is 0 in row 0), with
// inner gates that really depend on their three operands, the last gate reading the gate before it
// and every gate being read.  Immediates as life_bitops.h b3<IMM>: IMM = f(0xF0, 0xCC, 0xAA), the
// first operand most significant.
#include <stdint.h>
#include <stdio.h>

static const char *kEncName[3] = {"P,N", "M,P", "N,M"};  // (first, second) signal of a group
static const char kBit[3][2] = {{'P', 'N'}, {'M', 'P'}, {'N', 'M'}};
static int bit_of(char k, int w) { return k == 'P' ? w & 1 : k == 'M' ? w >> 1 : (w == 1 || w == 2); }

static uint32_t sig0[5], tgt;
static char name[7][4];

// the 8 minterm masks of operands (x, y, z) over the 32 rows
static void minterms(uint32_t x, uint32_t y, uint32_t z, uint32_t m[8]) {
    for (int i = 0; i < 8; i++)
        m[i] = ((i & 4) ? x : ~x) & ((i & 2) ? y : ~y) & ((i & 1) ? z : ~z);
}
// every inner gate over (x, y, z), canonical: 0 in row 0, nothing on an empty minterm, depends on all three
static int gates(const uint32_t m[8], uint32_t out[256], int imm[256]) {
    int n = 0;
    for (int t = 0; t < 256; t++) {
        uint32_t g = 0;
        int ok = 1;
        for (int i = 0; i < 8 && ok; i++)
            if (t >> i & 1) {
                if (!m[i]) ok = 0;
                g |= m[i];
            }
        if (!ok || (g & 1u)) continue;
        int dep = 1;  // flipping each operand changes g somewhere on the reachable rows
        for (int b = 1; b <= 4 && dep; b <<= 1) {
            int d = 0;
            for (int i = 0; i < 8; i++)
                if (m[i] && m[i ^ b] && ((t >> i & 1) != (t >> (i ^ b) & 1))) d = 1;
            dep = d;
        }
        if (!dep) continue;
        out[n] = g;
        imm[n++] = t;
    }
    return n;
}
// the last gate over (x, y, z): its immediate, or -1 when two rows with equal inputs differ in the target
static int last_gate(uint32_t x, uint32_t y, uint32_t z) {
    uint32_t m[8];
    minterms(x, y, z, m);
    int imm = 0;
    for (int i = 0; i < 8; i++) {
        if ((m[i] & tgt) && (m[i] & ~tgt)) return -1;
        if (m[i] & tgt) imm |= 1 << i;
    }
    return imm;
}

static long search3(int print) {
    long found = 0;
    for (int a = 0; a < 5; a++) for (int b = a + 1; b < 5; b++) for (int c = b + 1; c < 5; c++) {
        uint32_t m1[8], g1s[256];
        int i1[256];
        minterms(sig0[a], sig0[b], sig0[c], m1);
        const int n1 = gates(m1, g1s, i1);
        for (int k1 = 0; k1 < n1; k1++) {
            uint32_t sig[7];
            for (int i = 0; i < 5; i++) sig[i] = sig0[i];
            sig[5] = g1s[k1];
            for (int d = 0; d < 6; d++) for (int e = d + 1; e < 6; e++) for (int f = e + 1; f < 6; f++) {
                uint32_t m2[8], g2s[256];
                int i2[256];
                minterms(sig[d], sig[e], sig[f], m2);
                const int n2 = gates(m2, g2s, i2);
                for (int k2 = 0; k2 < n2; k2++) {
                    sig[6] = g2s[k2];
                    for (int p = 0; p < 6; p++) for (int q = p + 1; q < 6; q++) {
                        if (f != 5 && q != 5) continue;  // the first gate is read
                        const int imm = last_gate(sig[p], sig[q], sig[6]);
                        if (imm < 0) continue;
                        found++;
                        if (print) {
                            snprintf(name[5], 4, "g1");
                            snprintf(name[6], 4, "g2");
                            printf("  g1=b3<0x%02X>(%s,%s,%s) g2=b3<0x%02X>(%s,%s,%s) out=b3<0x%02X>(%s,%s,g2)\n",
                                   i1[k1], name[a], name[b], name[c], i2[k2], name[d], name[e], name[f], imm,
                                   name[p], name[q]);
                        }
                    }
                }
            }
        }
    }
    return found;
}

static long search2(int print) {
    long found = 0;
    for (int a = 0; a < 5; a++) for (int b = a + 1; b < 5; b++) for (int c = b + 1; c < 5; c++) {
        uint32_t m1[8], g1s[256];
        int i1[256];
        minterms(sig0[a], sig0[b], sig0[c], m1);
        const int n1 = gates(m1, g1s, i1);
        for (int k1 = 0; k1 < n1; k1++)
            for (int p = 0; p < 5; p++) for (int q = p + 1; q < 5; q++) {
                const int imm = last_gate(sig0[p], sig0[q], g1s[k1]);
                if (imm < 0) continue;
                found++;
                if (print)
                    printf("  g1=b3<0x%02X>(%s,%s,%s) out=b3<0x%02X>(%s,%s,g1)\n", i1[k1], name[a], name[b], name[c],
                           imm, name[p], name[q]);
            }
    }
    return found;
}

int main(void) {
    tgt = 0;  // row r: W0 = r & 3, W1 = r >> 2 & 3, alive = r >> 4
    for (int r = 0; r < 32; r++) {
        const int n9 = (r & 3) + 2 * (r >> 2 & 3), al = r >> 4;
        if (n9 == 3 || (al && n9 == 4)) tgt |= 1u << r;
    }
    printf("target %08x\n", tgt);
    long total3 = 0, total2 = 0;
    for (int e0 = 0; e0 < 3; e0++) for (int e1 = 0; e1 < 3; e1++) {
        for (int i = 0; i < 5; i++) sig0[i] = 0;
        for (int r = 0; r < 32; r++) {
            if (bit_of(kBit[e0][0], r & 3)) sig0[0] |= 1u << r;
            if (bit_of(kBit[e0][1], r & 3)) sig0[1] |= 1u << r;
            if (bit_of(kBit[e1][0], r >> 2 & 3)) sig0[2] |= 1u << r;
            if (bit_of(kBit[e1][1], r >> 2 & 3)) sig0[3] |= 1u << r;
            if (r >> 4) sig0[4] |= 1u << r;
        }
        snprintf(name[0], 4, "%c0", kBit[e0][0]);
        snprintf(name[1], 4, "%c0", kBit[e0][1]);
        snprintf(name[2], 4, "%c1", kBit[e1][0]);
        snprintf(name[3], 4, "%c1", kBit[e1][1]);
        snprintf(name[4], 4, "al");
        printf("W0 as (%s), W1 as (%s):\n", kEncName[e0], kEncName[e1]);
        const long n2 = search2(1), n3 = search3(1);
        printf("  2-gate tails: %ld   3-gate tails: %ld\n", n2, n3);
        total2 += n2;
        total3 += n3;
    }
    printf("all nine encoding pairs: 2-gate tails %ld, 3-gate tails %ld\n", total2, total3);
    return 0;
}
