// life_host.h -- host-only planning helpers of the runtime (life_plan.cpp):
// no HIP types, so CPU tests compile life_plan.cpp with g++ alone and check
// them without a GPU (tests/test_host_plan.py).
#pragma once
#include <stdint.h>

#include "life_mi355x.h"

namespace life {

// life_halo_plan with `loop` (bit 0: x, bit 1: y): that axis, with dims == 1,
// is exchanged too, the shard being its own neighbour (LIFE_OPT_LOOPBACK).
int halo_plan(int64_t nx, int64_t ny, int dims0, int dims1, int rank, int kernel, int loop, life_halo_op *ops,
              int max_ops);

#pragma GCC visibility push(hidden)  // the runtime's own: not among the library's dynamic symbols
// The LOCAL transport's pairing of a halo plan's messages, and the staging
// slots both transports use (pure: life_halo.hip resolves them once per plan).
// halo_op_slot: staging slot of op i = earlier ops of its phase with the same
// kind and what.
int halo_op_slot(const life_halo_op *ops, int i);
// halo_match_send: the send in `peer_ops` (the plan of rank mine[recv].peer)
// that receive `recv` of rank `rank`'s plan `mine` copies from: within a
// phase, the k-th receive from a peer pairs with the peer's k-th send to
// `rank`.  Returns its index, -1 when there is none.
int halo_match_send(const life_halo_op *mine, int recv, int rank, const life_halo_op *peer_ops, int npeer);
// halo_wait_peers: the peers other than `rank` itself named by the ops of
// `phase` and `kind`, each once, in plan order; returns their number (<= n).
int halo_wait_peers(const life_halo_op *ops, int n, int rank, int phase, int kind, int *peers);

// The next pass of a step call of the temporal tiles with `remaining` > 0
// generations left: K generations per exchange, at most bmax per pass, `since`
// generations advanced since the aprons were last filled (deep halo).  Every
// rank must compute this identically, or their send / receive groups stop
// pairing.
//  * deep: the call is cut at the K boundary (K - since generations; 32 =
//    11 + 11 + 10 at 12 generations per pass at most);
//  * the segment is split into ceil(seg / bmax) passes of nearly equal size
//    (a 20-generation call runs 10 + 10, not 16 + 4);
//  * refill_first: the aprons no longer cover the pass (since + m > K: a
//    longer pass than planned for, or the deep halo switched off while they
//    were part-used) -- exchange before it, since' = 0;
//  * extend: (deep) the aprons still hold the next pass's ghost cells, so
//    this pass skips the exchange and also advances the `ext` apron rows the
//    next one reads; not on the call's last pass (remaining == m) when the
//    next call's first pass could not fit (since' + m + bmax > K);
//  * otherwise the pass ends with the K-deep exchange.
struct PassPlan { int m; bool refill_first; bool extend; int ext; };  // ext = K - since' - m, since' after the refill
PassPlan next_pass(int K, int bmax, bool deep, int since, int64_t remaining);

// Pipelined passes of a single wrapped shard (LIFE_OPT_PIPELINE): a pass of
// nty tile rows is cut into R regions of whole tile rows, each its own
// launch, dealt over S streams, so that the first region of pass p + 1 may
// start in the launch tail of the last region of pass p.
//  * Regions: R contiguous groups of nearly equal size covering [0, nty),
//    each at least 2 tile rows (a last tile row shorter than the ghost depth
//    lets tile row 0's window reach two tile rows up: still the neighbouring
//    region).  With a banded last tile column (B > 1 tile rows per banded
//    item) the boundaries fall on multiples of B when every region can hold
//    a whole band (nty / B >= R: `aligned`); else they ignore B, and a
//    region's bands, which start at its first tile row, take a few more items.
//  * Order: pass p launches region (p + j) % R at position j = 0 .. R - 1;
//    launch i = p R + j runs on stream i % S.
//  * Dependencies: launch (p, r) reads what pass p - 1 wrote in regions r - 1,
//    r, r + 1 (cyclic) and overwrites the rows those same three launches
//    read.  They sit at positions (j + dr + 1) % R of pass p - 1, dr = -1, 0,
//    1: R + j - that position launches back.
//  * wait[j][0 .. nwait[j]): the launches, as distances back from i, that the
//    launch at position j of a pass p >= 1 waits for by event -- the required
//    ones that neither stream order nor a wait of an earlier launch of its
//    stream implies, worked out over passes 0 and 1 (later passes only know
//    more).  R = 4, S = 2: one wait, 3 back, at j = 0 .. 2.  The launches of
//    pass 0 depend on the fence before them only.  record[j]: some launch
//    waits for the one at position j.
// R == 0: no plan (R < 3, nty < 2 R, or more regions / streams than kPipeMax*).
constexpr int kPipeMaxRegions = 16, kPipeMaxStreams = 4;
struct PipePlan {
    int R = 0, S = 0;
    bool aligned = false;
    int64_t ty[kPipeMaxRegions + 1] = {};  // region r = tile rows [ty[r], ty[r + 1])
    int nwait[kPipeMaxRegions] = {};
    int wait[kPipeMaxRegions][kPipeMaxStreams] = {};
    bool record[kPipeMaxRegions] = {};
};
PipePlan pipe_plan(int64_t nty, int64_t B, int R, int S);

// The banded last tile column of the bit tiles.  A tile column that owns o
// < 62 pairs runs as up to kMaxBands contiguous sub-columns, each in groups
// of G = 2^gsh lanes (1 ghost + own owned + ghost pairs, own <= G - 2, 2 <=
// gsh <= 5), 64 / G tile rows per workgroup.  band_split(o) minimises the
// lanes a tile row of the column takes, the sum of G over its sub-columns: one
// sub-column at the smallest G that holds o when no pair of sub-columns takes
// fewer lanes (ties keep one), else the pair with the widest first part
// (o = 32: {30, G 32} + {2, G 4}, 36 lanes); n == 0, a whole 64-lane tile,
// when nothing takes fewer than 64 (o >= 45).
constexpr int kMaxBands = 2;
struct BandCol { int first, own, gsh; };  // first pair within the column, owned pairs, log2 of the group
struct BandSplit {
    int n = 0;
    BandCol b[kMaxBands] = {};
};
BandSplit band_split(int64_t o, int max_parts = kMaxBands);  // max_parts 1: one sub-column (o <= 30) or none
// Tile rows per banded item of each sub-column (64 >> gsh, powers of two).
struct BandRows {
    int n = 0;
    int64_t B[kMaxBands] = {};
    int64_t largest() const {  // a multiple of every other
        int64_t m = 1;
        for (int i = 0; i < n; i++) m = B[i] > m ? B[i] : m;
        return m;
    }
};
// pipe_plan with the regions aligned on the largest band (whole banded items
// of every sub-column)
inline PipePlan pipe_plan(int64_t nty, const BandRows &bands, int R, int S) {
    return pipe_plan(nty, bands.largest(), R, S);
}
#pragma GCC visibility pop

// Life-like rules (life_rule_parse, life_dev_set_rule): `birth` bit k = a dead
// cell with k live neighbours of 8 is born, `survive` bit k = a live cell
// with k stays alive.  B3/S23 runs the hand-searched tail (BitEnc::rule1);
// every other rule the table tail (TableRule, life_bitops.h), whose lane-
// uniform words rule_words derives: with n9 the live cells of the 3 x 3 block,
// the cell included, t(alive, n9) = birth bit n9 (dead; n9 = 9 cannot occur)
// or survive bit n9 - 1 (alive; n9 = 0 cannot occur); for alive = 0 / 1 and S
// = 0 .. 4 the leaf over n9 = 2 S + u0 is (u0 & a) ^ b with b = t(alive, 2 S)
// and a = b ^ t(alive, 2 S + 1), each all-ones or zero.
constexpr uint32_t kRuleMask = 0x1FFu, kConwayBirth = 1u << 3, kConwaySurvive = (1u << 2) | (1u << 3);
struct RuleWords {
    uint32_t a[2][5], b[2][5];  // [alive][S]
};
RuleWords rule_words(uint32_t birth, uint32_t survive);
// The one definition of a leaf, for rule_words and for the batch kernels that
// expand a universe's own masks on the device (life_batch_kernels.hip).
#ifdef __HIP__
#define LIFE_HOST_DEVICE __host__ __device__
#else
#define LIFE_HOST_DEVICE
#endif
struct RuleLeaf { uint32_t a, b; };
LIFE_HOST_DEVICE inline RuleLeaf rule_leaf(uint32_t birth, uint32_t survive, int alive, int s) {
    const uint32_t mask = alive ? survive : birth;
    // next state of a cell whose 3 x 3 block holds n9 live cells; n8 = n9 - alive outside 0 .. 8 cannot occur
    const int n8 = 2 * s - alive;
    const uint32_t t0 = n8 >= 0 && n8 <= 8 && ((mask >> n8) & 1u) ? 0xFFFFFFFFu : 0u;
    const uint32_t t1 = n8 + 1 <= 8 && ((mask >> (n8 + 1)) & 1u) ? 0xFFFFFFFFu : 0u;
    return RuleLeaf{t0 ^ t1, t0};
}
// B3/S23 in 7 gates per dword (ConwayRule7, life_bitops.h; the search: scripts/rule_search7.c,
// profiles/rule7/rule_search7.txt).  The column sums W0 = a0 + b0 + c0 and W1 = a1 + b1 + c1 are
// kept as (parity, not all equal) instead of the full adder's (parity, majority): p, n of W0 and
// x, y of W1, then g1 = b3<kR7G1>(p, n, y), g2 = b3<kR7G2>(n, x, g1), out = b3<kR7Out>(p, alive, g2).
// Immediates as b3<IMM>: IMM = f(0xF0, 0xCC, 0xAA), the first operand most significant.
constexpr uint32_t kR7Par = 0x96;  // a ^ b ^ c: W odd
constexpr uint32_t kR7Nae = 0x7E;  // not all equal: W is 1 or 2
constexpr uint32_t kR7G1 = 0x56;   // c ^ (a | b)
constexpr uint32_t kR7G2 = 0x42;   // (a ^ c) & ~(a ^ b)
constexpr uint32_t kR7Out = 0xA8;  // c & (a | b)
// v_bitop3_b32 on the host: bit i of the result is bit (a_i, b_i, c_i) of imm
inline uint32_t bitop3_host(uint32_t imm, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
    for (int k = 0; k < 8; k++)
        if ((imm >> k) & 1u) r |= ((k & 4) ? a : ~a) & ((k & 2) ? b : ~b) & ((k & 1) ? c : ~c);
    return r;
}
// ConwayRule7 word for word on the host (life_plan.cpp): 32 cells per call, checked against the
// definition over all 128 inputs by tests/test_rule7_host.py
uint32_t conway7_host(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0, uint32_t c1, uint32_t alive);
// The text forms: B36/S23 (either letter case) and Golly's 23/3 (S/B);
// digits 0-8 in any order, repeats and empty lists allowed.  false: not a
// rulestring.  rule_format writes the canonical B.../S... with ascending digits
// (at most 22 characters and the NUL).
bool rule_parse(const char *text, uint32_t *birth, uint32_t *survive);
void rule_format(uint32_t birth, uint32_t survive, char out[24]);
// Generations rules (life_rule_parse_gen): the forms above
// (states = 2), B2/S345/C4 (G for C, either letter case) and Golly's 345/2/4
// (S/B/C); 2 <= states <= kGenMaxStates.  rule_format_gen appends /Cn where
// states > 2 (at most 26 characters and the NUL).
constexpr uint32_t kGenMaxStates = 16;
bool rule_parse_gen(const char *text, uint32_t *birth, uint32_t *survive, uint32_t *states);
void rule_format_gen(uint32_t birth, uint32_t survive, uint32_t states, char out[32]);
// decay bit planes a universe of `states` states needs beside its alive plane:
// d = s - 1 of a dying cell, at most states - 2 (the kernels are built for 1, 2 and 4)
constexpr int gen_planes(uint32_t states) { return states <= 2 ? 0 : states <= 3 ? 1 : states <= 5 ? 2 : 4; }

// Batches (life_batch_*): how `count` universes of one shape
// are stored and launched.  Storage: natural 32-cell words, `words` per row,
// ny rows, universes `bytes` apart.  Wave tier (nx <= kBatchWaveMaxX, ny <=
// kBatchWaveMaxY): one universe per wave, one row per lane, kBatchWaves waves
// per workgroup.  Group tier: one universe per workgroup of lane groups of 2^
// lg_wp lanes, each a strip of `rows` rows -- the shapes of the small-grid
// register kernel (life_kernels.hip reg_small_rows: the same strip heights,
// threads and word limit, restated here so the plan needs no HIP).  tier 0:
// neither, `why` says so.
constexpr int64_t kBatchWaveMaxX = 128, kBatchWaveMaxY = 64, kBatchGroupMaxX = 2048;
constexpr int kBatchWaves = 4, kBatchGroupThreads = 1024;
struct BatchPlan {
    int tier = 0;
    int words = 0;           // per row
    int64_t bytes = 0;       // per universe
    int waves_per_group = 0; // waves of a workgroup
    int universes_per_group = 0;
    int rows = 0, lg_wp = 0, strips = 0;  // group tier: strip height R, log2 lanes per strip, ny / R
    char why[400] = {};
};
BatchPlan batch_plan(int64_t nx, int64_t ny);

// The dataflow queue head is 32-bit: one launch may hold at most
// kFlowMaxHead pulls (its items plus one extra pull per resident workgroup).
// flow_chunk_passes: passes of `tiles` items each one launch of `grid`
// resident workgroups may take (at most `cap` when cap > 0); 0 when not even
// one pass fits.  Host-only (life_plan.cpp).
constexpr int64_t kFlowMaxHead = (int64_t)1 << 31;
int64_t flow_chunk_passes(int64_t tiles, int64_t grid, int64_t cap);

// life_collect's fan-in (life_cart.c:281-305, 5-gather/life_mpi.c:177-179)
// as a plan: every rank exports its block in one of three frame formats
// (DENSE 1 B per cell, VTK 2 B, BITS = LIFEBITS packed rows), the root (rank
// world-1) places its own block first, then receives the others in rank order
// into two alternating staging slots (block k+1 arrives while block k is copied
// out).  Pure arithmetic on life_layout_query, shared by the device gather
// (life_frames.hip gather_impl) and the CPU tests.
enum GatherFormat { kGatherDense = 0, kGatherVtk = 1, kGatherBits = 2 };
struct GatherPiece {
    int32_t rank;         // the block's global rank
    int32_t slot;         // staging slot at the root: -1 = its own export, else 0 / 1
    int64_t bytes;        // message size = row_bytes * rows
    int64_t row_bytes;    // bytes per exported row
    int64_t rows;         // block rows
    int64_t dst;          // byte offset of its first row in the frame
    int32_t shared_first; // BITS: its first byte of every row is shared with the block on its left (OR-ed)
    int32_t shared_last;  // BITS: its last byte of every row is shared with the block on its right
};
int64_t gather_frame_row_bytes(int64_t nx, int fmt);
// Fills pieces[0 .. world) (the root's own first, then ranks 0 .. world-2 in
// receive order); *slot_bytes = the largest piece (one staging slot).
// Returns world, or LIFE_EINVAL.
int gather_plan(int64_t nx, int64_t ny, int dims0, int dims1, int kernel, int fmt, GatherPiece *pieces, int max,
                int64_t *slot_bytes);

// Launch-tail plan of one bit-tile launch over a full-width region (tile
// rows [ty0, ty1) of T owned rows each, the region ending at owned row
// yend): the first F tile rows stay full tiles, the rest become n2 tile rows
// of half-height tiles (T2 owned rows), banded in the last tile column like
// the full ones, dispatched last, so that the launch's last round is short
// items filling the slots the full tiles leave (life_kernels.hip
// launch_tstep).  Items of r tile rows: (ntx - 1) r + ceil(r
// / B) with bands of B tile rows (B > 1), else ntx r.  mode 1: round 4's rule
// (the fewest bottom rows whose half tiles fill one round, when the last
// round is under half full); mode 2: the split with the smallest makespan of
// a list schedule (items dealt in launch order to the earliest free of
// `slots` resident workgroups; full tiles last 1, half tiles c + (1 - c) /
// 2, c the fixed share of a tile: window load, stores, turnover).  F == ty1:
// no split.  Cached per argument set (a launch repeats its shape).
struct TailPlan {
    int64_t F = 0, n2 = 0;
    double makespan = 0.0;  // model tile-times (full tile = 1)
};
// items of `rows` tile rows `ntx` tile columns wide (the last column banded
// in items of B tile rows when B > 1)
inline int64_t tail_row_items(int64_t ntx, int64_t B, int64_t rows) {
    return rows <= 0 ? 0 : B > 1 ? (ntx - 1) * rows + (rows + B - 1) / B : ntx * rows;
}
// the list schedule's makespan of `pre` full items of another launch
// dispatched first (the ring beside an interior), F_rows full tile rows, then
// n2 half rows
double tail_makespan2(int64_t ntx, int64_t B, int64_t F_rows, int64_t n2, int64_t slots, double c, int64_t pre = 0);
TailPlan tail_plan(int64_t ntx, int64_t B, int64_t ty0, int64_t ty1, int64_t yend, int64_t T, int64_t T2,
                   int64_t slots, int mode, double c, int64_t pre = 0);
// The same with the band list: nfull ordinary tile columns, then the last
// column's sub-columns; r tile rows take nfull r + sum ceil(r / B_i) items.
// The forms above are the one-band case (nfull = ntx - 1, {B}; B <= 1: ntx
// ordinary columns, no bands).
inline int64_t tail_row_items(int64_t nfull, const BandRows &bands, int64_t rows) {
    if (rows <= 0) return 0;
    int64_t n = nfull * rows;
    for (int i = 0; i < bands.n; i++) n += (rows + bands.B[i] - 1) / bands.B[i];
    return n;
}
double tail_makespan2(int64_t nfull, const BandRows &bands, int64_t F_rows, int64_t n2, int64_t slots, double c,
                      int64_t pre = 0);
TailPlan tail_plan(int64_t nfull, const BandRows &bands, int64_t ty0, int64_t ty1, int64_t yend, int64_t T,
                   int64_t T2, int64_t slots, int mode, double c, int64_t pre = 0);

}  // namespace life
