// life_kernels.hip -- gfx950 (CDNA4) kernels of the Game-of-Life hot path.
//
// Replaces the reference's life_step (6-cartesian/life_cart.c:189-215, the
// same body as 3-life/life2d.c:104-130): B3/S23 on a periodic grid.  The
// reference reads 9 ints through a modulo-wrapping ind() per cell; here every
// shard is a padded block whose one-cell apron holds the periodic / remote
// neighbours (filled by the halo phase), so the stencil is branch-free.
//
// Stencil mapping (both encodings): one lane owns a 16-byte unit of a row and
// walks R consecutive rows down, keeping the horizontal 3-sums of rows y-1,
// y, y+1 in registers (vertical reuse in registers, no LDS round trip).  The
// horizontal neighbours of a unit's edge cells come from lanes +-1 by DPP
// wave shifts (v_mov_b32_dpp wave_shr/wave_shl); lane 0 / lane 63 fetch the
// one dword beyond the wave's span themselves.  HBM traffic is one read and
// one write of each cell's encoding plus 2/R of re-read halo rows.
//
//  * ByteEnc: 1 byte per cell.  SWAR on 4 cells per dword: horizontal sum via
//    v_alignbyte, 9-cell sum n9 <= 9 per byte, rule ((n9 - c) | c) == 3.
//  * BitEnc: 1 bit per cell in 64-cell interleaved pairs (E = even cells,
//    O = odd cells, life_bitops.h).  Horizontal (L,C,R) full adder -> 2-bit
//    sum per row; three rows add to n9 = u0 + 2*S; alive' = (n9 == 3) |
//    (alive & n9 == 4).  Every boolean step is one v_bitop3_b32 (per pair:
//    2 funnel shifts + 4 ops for the two rows sums, 2 x 8 for the rule).
//    Other Life-like rules (life_dev_set_rule) run table-rule instances of
//    the same bit kernels: the rule is a compile-time policy on the shared
//    bodies (ConwayRule / TableRule, life_bitops.h), 2 x 25 for the rule.
#include "life_kernels.h"
#include "life_act.h"
#include "life_bitops.h"
#include "life_diag.h"
#include "life_env.h"
#include "life_tile_decode.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <stdint.h>

namespace life {
namespace {

constexpr int kBlock = 256;  // 4 waves of 64

__device__ __forceinline__ uint32_t from_left(uint32_t old, uint32_t v) {
    // lane i <- lane i-1 (wave_shr:1); lane 0 keeps `old`.
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t from_right(uint32_t old, uint32_t v) {
    // lane i <- lane i+1 (wave_shl:1); lane 63 keeps `old`.
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xf, 0xf, false);
}

// ------------------------------------------------------------------ encodings
struct ByteEnc {
    static constexpr int64_t kCellsPerUnit = 16;
    static constexpr uint32_t kCell0 = 0xFFu;  // cell 0 of a dword
    static __device__ __forceinline__ int64_t dword_of(int64_t x) { return x >> 2; }
    static __device__ __forceinline__ uint32_t pos_in_dword(int64_t x) { return 8u * (uint32_t)(x & 3); }
    static __device__ __forceinline__ uint32_t top_shift(int64_t x) { return 24u - pos_in_dword(x); }
    struct H {
        uint32_t v[4];
    };
    // Horizontal 3-sum (x-1, x, x+1) of 16 byte cells; l / r: dword left of
    // d.x and dword right of d.w.
    static __device__ __forceinline__ H hsum(uint4 d, uint32_t l, uint32_t r) {
        H h;
        h.v[0] = d.x + __builtin_amdgcn_alignbyte(d.x, l, 3) + __builtin_amdgcn_alignbyte(d.y, d.x, 1);
        h.v[1] = d.y + __builtin_amdgcn_alignbyte(d.y, d.x, 3) + __builtin_amdgcn_alignbyte(d.z, d.y, 1);
        h.v[2] = d.z + __builtin_amdgcn_alignbyte(d.z, d.y, 3) + __builtin_amdgcn_alignbyte(d.w, d.z, 1);
        h.v[3] = d.w + __builtin_amdgcn_alignbyte(d.w, d.z, 3) + __builtin_amdgcn_alignbyte(r, d.w, 1);
        return h;
    }
    static __device__ __forceinline__ uint32_t rule1(uint32_t n9, uint32_t c) {
        const uint32_t m = (n9 - c) | c;                          // n8 | alive, per byte <= 9
        const uint32_t t = m ^ 0x03030303u;                       // 0 where m == 3
        const uint32_t nz = (t + 0x7F7F7F7Fu) & 0x80808080u;      // 0x80 where t != 0
        return (nz ^ 0x80808080u) >> 7;
    }
    static __device__ __forceinline__ uint4 rule(const H &a, const H &b, const H &c, uint4 v) {
        uint4 o;
        o.x = rule1(a.v[0] + b.v[0] + c.v[0], v.x);
        o.y = rule1(a.v[1] + b.v[1] + c.v[1], v.y);
        o.z = rule1(a.v[2] + b.v[2] + c.v[2], v.z);
        o.w = rule1(a.v[3] + b.v[3] + c.v[3], v.w);
        return o;
    }
};


// ------------------------------------------------------------------ stencil
// Per-lane constants of one stencil launch.  Every load is unconditional (a
// lane right of the row reads a clamped, in-pitch unit) and every store
// goes somewhere (a lane that must not write redirects to `sink` with row
// stride 0), so a lane's whole strip is ONE basic block and the prefetch ring
// below really keeps D rows of loads in flight.
struct Lane {
    const uint8_t *in;
    int64_t pitch, h, ya;
    int64_t off;        // byte offset of the (clamped) unit in a padded row
    int64_t exoff;      // extra dword: left (lane 0), right (lane 63), wrap-left (unit 0)
    uint32_t exshift;   // wrap-left: move cell w-1 to the top position of the dword
    int64_t xoff;       // word 0 of a row (wrap-right source)
    uint4 pmask;        // wrap-right: where cell w sits inside this unit (last unit only)
    uint32_t pshift;    //   ... its bit/byte position within that dword
    bool pright;        // wrap-right: cell w is the right extra (w % cells_per_unit == 0)
    bool needex;        // lanes 0 / 63 and the wrap-left unit: the extra dword is read
    bool wrapy;
};

__device__ __forceinline__ const uint8_t *row_ptr(const Lane &c, int64_t y) {
    // owned row y in [-1, h]; with a periodic y axis inside the shard the
    // apron rows are the opposite owned rows (ind() wrap, life_cart.c:11).
    if (c.wrapy) y = y < 0 ? y + c.h : (y >= c.h ? y - c.h : y);
    return c.in + (y + c.ya) * c.pitch;
}

struct RowData {
    uint4 d;
    uint32_t ex, e0;
};

// A dword every lane reads at the same address, through the VECTOR memory
// path: the opaque zero offset keeps the compiler from turning a
// wave-uniform address into a scalar (constant-cache) load of grid data
// another kernel wrote.
__device__ __forceinline__ uint32_t load_u32_vec(const uint8_t *p) {
    uint32_t z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return *reinterpret_cast<const uint32_t *>(p + z);
}

template <bool WRAPX>
__device__ __forceinline__ RowData load_row(const Lane &c, int64_t y) {
    const uint8_t *row = row_ptr(c, y);
    RowData r;
    r.d = *reinterpret_cast<const uint4 *>(row + c.off);
    // only the lanes whose neighbour dword lies outside the wave (0, 63, the
    // wrap-left unit) load it: one memory instruction per row instead of two
    // for the other 62 lanes (their ex is never read: DPP takes lanes +-1)
    r.ex = c.needex ? *reinterpret_cast<const uint32_t *>(row + c.exoff) : 0u;
    r.e0 = WRAPX ? load_u32_vec(row + c.xoff) : 0u;  // one address per wave
    return r;
}

template <class E, bool WRAPX>
__device__ __forceinline__ typename E::H row_sum(const Lane &c, RowData &r) {
    uint32_t ex = r.ex << c.exshift;
    uint32_t right = from_right(ex, r.d.x);
    if (WRAPX) {
        // the cell right of w-1 is cell 0 of the row (periodic x inside the shard)
        const uint32_t c0 = (r.e0 & E::kCell0) << c.pshift;
        r.d.x = (r.d.x & ~c.pmask.x) | (c0 & c.pmask.x);
        r.d.y = (r.d.y & ~c.pmask.y) | (c0 & c.pmask.y);
        r.d.z = (r.d.z & ~c.pmask.z) | (c0 & c.pmask.z);
        r.d.w = (r.d.w & ~c.pmask.w) | (c0 & c.pmask.w);
        right = c.pright ? r.e0 : right;
    }
    return E::hsum(r.d, from_left(ex, r.d.w), right);
}

// N output rows starting at owned row ys (owned rows ys-1 .. ys+N are read),
// D rows of loads kept in flight.
template <class E, int N, int D, bool WRAPX, class RP = ConwayRule>
__device__ __forceinline__ void strip_full(const Lane &c, int64_t ys, uint8_t *dst, int64_t spitch,
                                           const RP &rp = RP{}) {
    static_assert(D <= N + 2, "prefetch deeper than the strip");
    RowData q[D];
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = load_row<WRAPX>(c, ys - 1 + k);
    typename E::H hp, hc;
    uint4 cc;
#pragma unroll
    for (int k = 0; k < N + 2; ++k) {
        RowData r = q[k % D];
        if (k + D < N + 2) q[k % D] = load_row<WRAPX>(c, ys - 1 + k + D);
        const typename E::H hn = row_sum<E, WRAPX>(c, r);
        if (k == 0) {
            hp = hn;
        } else if (k == 1) {
            hc = hn;
            cc = r.d;
        } else {
            if constexpr (RP::kTable)
                *reinterpret_cast<uint4 *>(dst) = rule_unit(rp, hp, hc, hn, cc);
            else
                *reinterpret_cast<uint4 *>(dst) = E::rule(hp, hc, hn, cc);
            dst += spitch;
            hp = hc;
            hc = hn;
            cc = r.d;
        }
    }
}

template <class E, bool WRAPX, class RP = ConwayRule>
__device__ __forceinline__ void strip_tail(const Lane &c, int64_t ys, int n, uint8_t *dst, int64_t spitch,
                                           const RP &rp = RP{}) {
    RowData r = load_row<WRAPX>(c, ys - 1);
    typename E::H hp = row_sum<E, WRAPX>(c, r);
    r = load_row<WRAPX>(c, ys);
    typename E::H hc = row_sum<E, WRAPX>(c, r);
    uint4 cc = r.d;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        r = load_row<WRAPX>(c, ys + 1 + i);
        const typename E::H hn = row_sum<E, WRAPX>(c, r);
        if constexpr (RP::kTable)
            *reinterpret_cast<uint4 *>(dst) = rule_unit(rp, hp, hc, hn, cc);
        else
            *reinterpret_cast<uint4 *>(dst) = E::rule(hp, hc, hn, cc);
        dst += spitch;
        hp = hc;
        hc = hn;
        cc = r.d;
    }
}

template <class E, int R, int D, bool WRAPX>
__global__ __launch_bounds__(kBlock) void step_kernel(StepArgs a) {
    int64_t b = blockIdx.x;
    if (a.xcd) {
        // blocks b, b + 8, ... share an XCD: give each XCD a contiguous
        // row-major run of strips, so the strips beside and below a strip
        // (the extra dwords of lanes 0 / 63, the two halo rows) hit its L2
        const int64_t n = (int64_t)gridDim.x, x = b & 7, k = b >> 3, per = n >> 3, rem = n & 7;
        b = (x < rem ? x * (per + 1) : rem * (per + 1) + (x - rem) * per) + k;
    }
    const int64_t bx = b % a.nbx, by = b / a.nbx;
    const int lane = threadIdx.x & 63;
    const int64_t wbase = a.u0 + (bx * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 64;
    if (wbase >= a.u1) return;  // the whole wave is right of the region
    const int64_t ys = a.r0 + by * R;
    const int64_t u = wbase + lane;
    const int64_t uc = u < a.units ? u : a.units;  // unit `units` is in-pitch: right-neighbour provider
    Lane c;
    c.in = a.in;
    c.pitch = a.pitch;
    c.h = a.h;
    c.ya = a.ya;
    c.wrapy = a.wrapy != 0;
    c.xoff = a.xoff;
    c.off = a.xoff + 16 * uc;
    c.exoff = c.off;
    c.exshift = 0;
    if (lane == 0) c.exoff = c.off - 4;
    if (lane == 63 && u < a.units) c.exoff = c.off + 16;
    c.needex = lane == 0 || lane == 63;
    c.pmask = make_uint4(0u, 0u, 0u, 0u);
    c.pshift = 0;
    c.pright = false;
    if (WRAPX) {
        if (u == 0) {  // left of cell 0 is cell w-1
            const int64_t wl = a.w - 1;
            c.exoff = a.xoff + E::dword_of(wl) * 4;
            c.exshift = E::top_shift(wl);
            c.needex = true;
        }
        if (u == a.units - 1) {  // right of cell w-1 is cell 0
            const int64_t q = a.w - (a.units - 1) * E::kCellsPerUnit;  // 1 .. kCellsPerUnit
            if (q == E::kCellsPerUnit) {
                c.pright = true;
            } else {
                const int comp = (int)E::dword_of(q);
                const uint32_t m = E::kCell0 << E::pos_in_dword(q);
                c.pshift = E::pos_in_dword(q);
                c.pmask.x = comp == 0 ? m : 0u;
                c.pmask.y = comp == 1 ? m : 0u;
                c.pmask.z = comp == 2 ? m : 0u;
                c.pmask.w = comp == 3 ? m : 0u;
            }
        }
    }
    const bool st = u < a.u1;
    uint8_t *dst = st ? a.out + (ys + a.ya) * a.pitch + a.xoff + 16 * u : a.sink + 16 * lane;
    const int64_t spitch = st ? a.pitch : 0;
    const int64_t n = a.r1 - ys < R ? a.r1 - ys : R;
    if (n == R)
        strip_full<E, R, D, WRAPX>(c, ys, dst, spitch);
    else
        strip_tail<E, WRAPX>(c, ys, (int)n, dst, spitch);
}

// step_kernel's text again, under a rule policy, for the table-rule kernel
// below.  A twin, not a body both kernels call: with the B3/S23 kernels routed
// through a shared body (by reference or by value) 18 to 31 of this unit's 133
// B3/S23 instances compiled to other schedules, a few instructions each, and
// rules must leave those code objects as they were.  Keep the two in step.
template <class E, int R, int D, bool WRAPX, class RP>
__device__ __forceinline__ void step_body(const StepArgs &a, const RP &rp) {
    int64_t b = blockIdx.x;
    if (a.xcd) {
        const int64_t n = (int64_t)gridDim.x, x = b & 7, k = b >> 3, per = n >> 3, rem = n & 7;
        b = (x < rem ? x * (per + 1) : rem * (per + 1) + (x - rem) * per) + k;
    }
    const int64_t bx = b % a.nbx, by = b / a.nbx;
    const int lane = threadIdx.x & 63;
    const int64_t wbase = a.u0 + (bx * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 64;
    if (wbase >= a.u1) return;  // the whole wave is right of the region
    const int64_t ys = a.r0 + by * R;
    const int64_t u = wbase + lane;
    const int64_t uc = u < a.units ? u : a.units;  // unit `units` is in-pitch: right-neighbour provider
    Lane c;
    c.in = a.in;
    c.pitch = a.pitch;
    c.h = a.h;
    c.ya = a.ya;
    c.wrapy = a.wrapy != 0;
    c.xoff = a.xoff;
    c.off = a.xoff + 16 * uc;
    c.exoff = c.off;
    c.exshift = 0;
    if (lane == 0) c.exoff = c.off - 4;
    if (lane == 63 && u < a.units) c.exoff = c.off + 16;
    c.needex = lane == 0 || lane == 63;
    c.pmask = make_uint4(0u, 0u, 0u, 0u);
    c.pshift = 0;
    c.pright = false;
    if (WRAPX) {
        if (u == 0) {  // left of cell 0 is cell w-1
            const int64_t wl = a.w - 1;
            c.exoff = a.xoff + E::dword_of(wl) * 4;
            c.exshift = E::top_shift(wl);
            c.needex = true;
        }
        if (u == a.units - 1) {  // right of cell w-1 is cell 0
            const int64_t q = a.w - (a.units - 1) * E::kCellsPerUnit;  // 1 .. kCellsPerUnit
            if (q == E::kCellsPerUnit) {
                c.pright = true;
            } else {
                const int comp = (int)E::dword_of(q);
                const uint32_t m = E::kCell0 << E::pos_in_dword(q);
                c.pshift = E::pos_in_dword(q);
                c.pmask.x = comp == 0 ? m : 0u;
                c.pmask.y = comp == 1 ? m : 0u;
                c.pmask.z = comp == 2 ? m : 0u;
                c.pmask.w = comp == 3 ? m : 0u;
            }
        }
    }
    const bool st = u < a.u1;
    uint8_t *dst = st ? a.out + (ys + a.ya) * a.pitch + a.xoff + 16 * u : a.sink + 16 * lane;
    const int64_t spitch = st ? a.pitch : 0;
    const int64_t n = a.r1 - ys < R ? a.r1 - ys : R;
    if (n == R)
        strip_full<E, R, D, WRAPX>(c, ys, dst, spitch, rp);
    else
        strip_tail<E, WRAPX>(c, ys, (int)n, dst, spitch, rp);
}

// The one-generation bit kernel under a table rule (life_dev_set_rule): what
// narrow or short blocks run.  One strip shape (kRuleStepRows rows per lane,
// 4 rows of loads in flight): these blocks are small, life_tune does not
// reach it.
constexpr int kRuleStepRows = 16;
struct RStepArgs {
    StepArgs s;
    RuleWords w;
};
template <bool WRAPX>
__global__ __launch_bounds__(kBlock) void rule_step_kernel(RStepArgs a) {
    step_body<BitEnc, kRuleStepRows, 4, WRAPX>(a.s, TableRule(a.w));
}

// ------------------------------------------------------------------ temporal
// Temporally blocked stencils (layouts with generations_per_exchange = K
// > 1): m <= K generations per launch, each cell read once from and written
// once to HBM per pass (plus the ghost rows of its window).  A tile is one
// workgroup of NW vertically stacked waves holding a window of NW*R rows x 64
// lane columns in registers, all m generations with one barrier each; lanes 0
// and 63 are the tile's x-apron, so a tile owns 62 lane columns.  A lane
// column is one interleaved pair (64 cells) for the bit encoding
// (tile_body_bit) and one 32-cell word, packed from 32 byte cells on load,
// for the byte encoding (tile_body_byte).  Two launch forms:
//
//  * tstep_kernel: one launch per pass, up to 4 tile regions (the boundary
//    ring of a partitioned shard, or the whole shard);
//  * tflow_kernel (bit): every pass of a step call on a single wrapped shard
//    in one persistent launch, tiles handed from pass to pass (LIFE_OPT_FLOW).

constexpr int kStackWaves = 8;  // waves per byte tile workgroup (2 per SIMD; 12 measured slower, profiles/r02/r2w)
struct TArgs {
    const uint8_t *in;
    uint8_t *out;
    int64_t pitch, xoff, W, h, ya;  // W = lane columns per owned row: pairs (bit) or 32-cell words (byte)
    // up to kMaxRegions tile regions in one launch (the boundary ring of a
    // partitioned shard); workgroup b belongs to the region with first[k] <= b
    int64_t tx0[kMaxRegions], tx1[kMaxRegions], ty0[kMaxRegions], ty1[kMaxRegions], first[kMaxRegions + 1];
    int32_t nreg, m;  // generations of the launch = ghost rows at each end of a window (bit)
    // banded tile column (bit; tile_geom): nband > 0 cuts the tiles of the
    // last tile column (tile columns [.., btx1) end with it) into nband
    // sub-columns; sub-column i owns pairs [borg[i], borg[i] + bown[i]) in
    // bands of G = 2^bgsh[i] lanes, 64 / G tile rows per workgroup.  A region
    // whose tx1 == btx1 lists its full tiles first, then the ceil((ty1 -
    // ty0) / (64 / G)) banded items of sub-column 0, then those of 1
    int32_t nband, bgsh[kMaxBands], bown[kMaxBands];
    int64_t borg[kMaxBands], btx1;
    // tail split (bit, a launch of one region; launch_tstep): with tail_ntx
    // > 0, workgroups >= tail_first run half-height tiles (R / 2 rows per
    // wave) over owned rows [tail_y, tail_yend), tile columns [tail_tx0,
    // tail_tx0 + tail_ntx) per tile row, the last one banded like the full
    // tiles when it is the banded column (tail_tx0 + tail_ntx == btx1), so
    // the last round of a launch is made of half-length items
    int64_t tail_first, tail_y, tail_yend, tail_ntx, tail_tx0;
    // XCD-aware order (bit, LIFE_XCD_ORDER): workgroups [0, xcd_n) are
    // renumbered so that each XCD (blocks b, b + 8, ... share one) walks a
    // contiguous row-major run of items; 0: dispatch order
    int64_t xcd_n;
    // deep-halo pass (Extend::x, bit): the lanes holding the apron pairs -1
    // and W store them too
    int32_t xext;
    // the item decode's constants, made from the fields above once per
    // launch (tile_args_seal, life_tile_decode.h): the kernels find their
    // item in 32-bit arithmetic and read none of the region fields
    TileDec d;
};
static_assert(kMaxRegions == kTdMaxRegions && kMaxBands == kTdMaxBands, "life_tile_decode.h");

// Census instances of the bit tiles (LIFE_OPT_POPULATION): a
// tile also counts, after every generation of its pass, the live cells it
// owns -- the rows and lanes it will store, without the apron rows and pairs
// a deep-halo pass advances -- and adds the pass's m counts to one stripe of
// the shard's counters: cnt[stripe][kPopGens], the stripe chosen by the
// workgroup index (kPopStripes, a power of two; each stripe on cache lines of
// its own).  The launcher's fold kernel sums the stripes into the trace.
// Whole pairs only: a shard whose width is no multiple of 64 holds apron cells
// in its last pair and takes the generic path (life_step.hip).
struct PopArgs {
    unsigned long long *cnt;
    int64_t y0, y1;  // the counted rows [y0, y1) of the launch's tile grid: the shard's real owned rows
};

template <int NW>
using Xch =uint32_t[2][NW][4][64];  // byte tiles: [parity][wave][top s0/s1, bottom s0/s1][lane]
// bit tiles: [parity][1 + wave][top e0 e1 o0 o1, bottom ...][lane]; slots 0
// and NW + 1 stay zero (the dead rows beyond the window): no branch on the
// wave index in the generation loop
template <int NW>
using XchP = uint32_t[2][NW + 2][8][64];
template <int NW>
struct XchB {
    XchP<NW> s;
};

// Bit tiles over interleaved pairs.  Lane l of a tile holds pair column
// 62 tx + l - 1 of R consecutive window rows as (E, O) register pairs; wave
// i holds window rows [iR, (i+1)R) of a window that starts m rows above the
// tile, T = NW*R - 2m owned rows per tile.  Per generation and row: the
// neighbour dwords of the lanes on either side by two ds_bpermute (the LDS
// pipe; measured 4 % faster than a DPP move for the left one,
// profiles/r03/ubench_pair.txt), 2 v_alignbit, 2 full adders (4 v_bitop3) for
// the even and odd cells' horizontal sums, and the rule (8 v_bitop3) per
// dword: 22 VALU + 2 LDS per pair-row, 11 VALU per 32 cells (the natural
// one-word layout: 13).  Each generation a wave publishes the sums of its
// first and last row in LDS (8 dwords per lane), one barrier, and takes its
// neighbours'; the window's top and bottom m rows and the edge lanes absorb
// the wrong values that enter from outside (m rows / m <= 32 cells after m
// generations), so rows [m, NW*R - m) of lanes 1..62 are exact and stored.
//
// FLOW (tflow_kernel): the window is loaded with agent-scope (`sc1`,
// L1-bypassing) 8-B atomic-form loads, and stored with `sc1` write-through
// stores (FLOW 1) or plain stores (FLOW 2, the kernel releases them with a
// fence): the rows are another workgroup's output of the same launch.
//
// Banded tiles: a tile column that owns o < 62 pairs (the last one: W =
// 62 (ntx - 1) + o) wastes part of a 64-lane tile.  BAND: the wave is cut
// into groups of G = 2^gsh lanes (1 ghost + own owned + ghost pairs), group
// g holding tile row ty + g of pairs [org, org + own): one workgroup carries
// nb <= 64 / G tile rows ("bands").  The neighbour dwords a group's edge
// lanes fetch come from the adjacent group: garbage, exactly as a tile's
// lanes 0 / 63 read beyond the tile, absorbed by the ghost lanes.  Only the
// loads and stores differ (per-lane rows); the generation loop is the tile's.
// The column may run as two such sub-columns (life::band_split; 65536^2: o =
// 32 as 30 pairs at G = 32 and 2 at G = 4, 36 lanes per tile row instead of
// 64): each is a narrow tile column of its own, whose ghost lanes load the
// other's edge pair from the input buffer.  Without BAND: an ordinary tile
// (gsh = 6, nb = 1).
// LIFE_FLOW_BP_AHEAD (default 1): the dataflow tiles' generation loop issues
// each row's two neighbour permutes that many rows ahead of their use, rows
// fenced in program order.  Left to itself the compiler scheduled that loop
// (more live state around it than in tstep_bit_kernel's) with every permute
// right before its wait: mean permute -> wait distance 1.8 instructions
// against 7.6-9.8 in the per-launch tiles (tests/test_isa.py), the
// scheduling loss round 4 measured at 8 % there.  (Forcing the same in the
// per-launch tiles, whose own schedule is good, cost 1-3.5 %: off there.)
#ifndef LIFE_FLOW_BP_AHEAD
#define LIFE_FLOW_BP_AHEAD 1
#endif
// LIFE_FAST_WRAP: a tile's wrapped pair column and first row by one
// conditional add / subtract instead of a 64-bit remainder (per lane for the
// column) when the axis is long enough for the index to be at most one
// period out; the remainder stays for short axes.  Driver-shaped launch
// 0.4346 vs 0.4400 ms mean over three ABAB pairs on one box (-1.2 %, noisy),
// byte flat; parity + golden modules green (profiles/r04/fastwrap_ad).
#ifndef LIFE_FAST_WRAP
#define LIFE_FAST_WRAP 1
#endif
// LIFE_TILE_STRAIGHT (compile time, A/B): a plain tile's wave decides once
// whether its R window rows cross the periodic seam and whether it stores all
// of its R rows; when not / so -- all but the waves at a window's ends and the
// first and last tile rows of a launch -- the loads and the stores are R
// instructions in one basic block each, the row base walked by the pitch in
// scalar registers (0: a wrap test per loaded row, two range tests per stored
// row; profiles/tilehead).
#ifndef LIFE_TILE_STRAIGHT
#define LIFE_TILE_STRAIGHT 1
#endif

//
// ACT (tskip kernels, LIFE_OPT_SKIP_DEAD): a plain tile also notes, per row it
// stores, whether any lane, the lane of its first pair or the lane of its last
// pair stored a set bit (one ballot per row: wave-uniform masks in SGPRs), and
// one lane ORs the masks into `act`, the zeroed map of the output buffer
// (life_act.h: R <= kActRows rows of a wave lie in at most two map rows, all in
// map column tx).  Compiles to nothing when off: the other instances keep
// their code.
//
// POP (tpop kernels, LIFE_OPT_POPULATION): after each generation's update a
// wave popcounts the cells it owns (2 v_bcnt per pair row, kPopValuPerPairRow)
// and leaves the wave's sum in pl[g][wave] (LDS); after the stores one wave
// adds the m sums of the workgroup to its stripe of pa->cnt.  The ownership
// test is recomputed from the lane id in every generation, as the store code
// does after the loop: nothing more stays live across the loop.  Compiles to
// nothing when off, as ACT.
template <int R, bool WRAPX, bool WRAPY, int FLOW, int NW, bool BAND = false, class RP = ConwayRule, bool ACT = false,
          bool POP = false>
__device__ __forceinline__ void tile_body_bit(const TArgs &a, const uint8_t *in, uint8_t *out, int tx,
                                              int ty, XchB<NW> &xb, int gsh = 6, int nb = 1,
                                              int ybase = 0, int yend = -1, int org = 0, int own = 62,
                                              const RP &rule = RP{}, uint32_t *act = nullptr,
                                              const PopArgs *pa = nullptr, uint32_t *pl = nullptr) {
    XchP<NW> &xch = xb.s;
    static_assert(R >= 3, "window");
    static_assert(!ACT || (!BAND && !FLOW && R <= kActRows), "activity map: plain tiles");
    const int K = a.m;  // ghost rows per window end
    const int T = NW * R - 2 * K;
    const int lane = threadIdx.x & 63;
    const int laddr = ((lane - 1) & 63) << 2, raddr = ((lane + 1) & 63) << 2;
    // wave index: uniform, so every row address below is scalar (SALU) math
    const int wi = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gl = BAND ? lane >> gsh : 0;                  // this lane's band (tile row ty + gl)
    const int pin = BAND ? lane & ((1 << gsh) - 1) : lane;  // lane within its group
    // pair column of this lane (BAND: the sub-column's pairs start at org; tx is not used)
    // Column and row indices are 32-bit: pair columns up to W + 62 and rows
    // up to h + 17 T + NW R are below 2^31 for every launch the host lets
    // through (tile_args_seal); only row x pitch byte offsets are 64-bit.
    const int W = (int)a.W, h = (int)a.h;
    const int j = (BAND ? org : tx * 62) + pin - 1;
    int jl;
    if (WRAPX) {
        // j lies in [-1, W + 62): one conditional add / subtract when W >= 64
        // (a remainder per lane otherwise)
        if (LIFE_FAST_WRAP && W >= 64) {
            jl = j < 0 ? j + W : (j >= W ? j - W : j);
        } else {
            jl = j % W;
            if (jl < 0) jl += W;
        }
    } else {
        jl = j > W ? W : j;  // pairs -1 .. W hold cells / apron; beyond: clamp (never stored)
    }
    const uint32_t voff = (uint32_t)a.xoff + 8u * (uint32_t)jl;
    const int y0 = ybase + ty * T - K + wi * R;  // owned row of register row 0 (>= -K)
    // Row pointers are walked: with a periodic y axis the walk wraps at h;
    // with an apron the last tile's window may run past the apron row h+K-1
    // into the allocation slack below the buffer (kTemporalSlackRows; those
    // rows are never stored).
    const uint8_t *row0 = in + a.ya * a.pitch;  // owned row 0
    uint32_t ve[R], vo[R];
    {
        int y = y0 + (BAND ? (gl < nb ? gl : nb - 1) * T : 0);  // bands: per-lane rows
        if (WRAPY) {
            // y lies in [-K, h + 16 T + NW R) (a band lane adds gl T, gl < 16):
            // one conditional add / subtract when h exceeds that margin with
            // room to spare (a remainder otherwise)
            if (LIFE_FAST_WRAP && h > 65 * (NW * R)) {
                y = y < 0 ? y + h : (y >= h ? y - h : y);
            } else {
                y %= h;
                if (y < 0) y += h;
            }
        }
        const uint8_t *p = row0 + (int64_t)y * a.pitch;
        auto load_row = [&](int r) {
            uint64_t q;
            if (FLOW)
                q = __hip_atomic_load(reinterpret_cast<uint64_t *>(const_cast<uint8_t *>(p) + voff),
                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                q = *reinterpret_cast<const uint64_t *>(p + voff);
            ve[r] = (uint32_t)q;
            vo[r] = (uint32_t)(q >> 32);
        };
        // A plain tile's rows are wave-uniform.  Unless the wave's R rows cross
        // the periodic seam (the first and last tile rows of a launch only) the
        // row base is walked by the pitch with no test per row: the R loads in
        // one basic block (LIFE_TILE_STRAIGHT, tests/test_isa_tile_head.py).
        // Without WRAPY the walk never wraps (the window may run into the
        // slack rows below the buffer, see above).
        if (LIFE_TILE_STRAIGHT && !BAND && (!WRAPY || y + R <= h)) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                load_row(r);
                p += a.pitch;
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                load_row(r);
                ++y;
                if (WRAPY && y == h) {
                    y = 0;
                    p = row0;
                } else {
                    p += a.pitch;
                }
            }
        }
    }
    auto hsum = [&](uint32_t e, uint32_t o, uint32_t &e0, uint32_t &e1, uint32_t &o0, uint32_t &o1) {
        BitEnc::pair_sums(e, o, bperm(laddr, o), bperm(raddr, e), e0, e1, o0, o1);
    };
    // Register budget (80 VGPRs at 3 tiles per CU, R = 24: 48 hold the
    // window): only the rolling sums of three rows stay live across the
    // loop.  Row 0 is updated first (its upper neighbour's sums come from LDS
    // right after the barrier), the bottom row's own sums and the row below
    // the wave are read back from LDS when row R-1 is reached.  No branch on
    // the wave index inside the loop (the zero slots stand for the dead rows
    // beyond the window): a branch there split the loop body into blocks and
    // the every row's ds_bpermute was hoisted above it, their 2R results
    // spilling (46-83 VGPRs at R = 24).
    // POP: bit r set when register row r of a lane whose rows start at owned row yb is counted -- one
    // of the rows the wave stores (r0, r1 and ylim below) inside the counted rows [pa->y0, pa->y1)
    auto pop_rows = [&](int64_t yb) -> uint32_t {
        const int64_t R64 = R;
        const int64_t yl = min(yend >= 0 ? yend : a.h, pa->y1);
        const int lo = max(min(max(K - wi * R, 0), R), (int)min(max(pa->y0 - yb, (int64_t)0), R64));
        const int hi = min(min(max(NW * R - K - wi * R, 0), R), (int)min(max(yl - yb, (int64_t)0), R64));
        return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
    };
    // a plain tile's mask is wave-uniform: one SGPR across the loop (banded lanes recompute theirs)
    const uint32_t rm_s = POP && !BAND ? (uint32_t)__builtin_amdgcn_readfirstlane((int)pop_rows(y0)) : 0u;
    if (wi == 0 || wi == NW - 1)  // the dead slots (ordered by the first barrier below)
        for (int q = 0; q < 16; ++q) xch[q >> 3][wi == 0 ? 0 : NW + 1][q & 7][lane] = 0u;
    if (LIFE_WG_TRACE && !FLOW) {  // phase stamps of the per-launch tiles (scripts/wg_trace.py): window loaded
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_trace(2, 64);
    }
    for (int g = 0; g < a.m; ++g) {
        const int par = g & 1;
        uint32_t pe0, pe1, po0, po1, ce0, ce1, co0, co1;
        {
            uint32_t be0, be1, bo0, bo1;
            hsum(ve[R - 1], vo[R - 1], be0, be1, bo0, bo1);
            xch[par][wi + 1][4][lane] = be0;
            xch[par][wi + 1][5][lane] = be1;
            xch[par][wi + 1][6][lane] = bo0;
            xch[par][wi + 1][7][lane] = bo1;
        }
        hsum(ve[0], vo[0], pe0, pe1, po0, po1);
        xch[par][wi + 1][0][lane] = pe0;
        xch[par][wi + 1][1][lane] = pe1;
        xch[par][wi + 1][2][lane] = po0;
        xch[par][wi + 1][3][lane] = po1;
        __syncthreads();
        hsum(ve[1], vo[1], ce0, ce1, co0, co1);
        {
            // the wave above (slot 0 above the window: zero, dead ghost rows)
            const uint32_t ae0 = xch[par][wi][4][lane], ae1 = xch[par][wi][5][lane];
            const uint32_t ao0 = xch[par][wi][6][lane], ao1 = xch[par][wi][7][lane];
            ve[0] = rule(ae0, ae1, pe0, pe1, ce0, ce1, ve[0]);
            vo[0] = rule(ao0, ao1, po0, po1, co0, co1, vo[0]);
        }
        constexpr int BAH = FLOW ? LIFE_FLOW_BP_AHEAD : 0;  // permutes ahead (dataflow tiles only)
        uint32_t bl[BAH > 0 ? BAH : 1], br[BAH > 0 ? BAH : 1];
#pragma unroll
        for (int k = 0; k < BAH; ++k)
            if (2 + k < R - 1) {
                bl[k] = bperm(laddr, vo[2 + k]);
                br[k] = bperm(raddr, ve[2 + k]);
            }
#pragma unroll
        for (int r = 1; r < R - 1; ++r) {
            uint32_t ne0, ne1, no0, no1;
            if (r + 1 == R - 1) {  // published before the barrier
                ne0 = xch[par][wi + 1][4][lane];
                ne1 = xch[par][wi + 1][5][lane];
                no0 = xch[par][wi + 1][6][lane];
                no1 = xch[par][wi + 1][7][lane];
            } else if (BAH > 0) {
                const uint32_t l = bl[0], rr = br[0];
#pragma unroll
                for (int k = 0; k + 1 < BAH; ++k) {
                    bl[k] = bl[k + 1];
                    br[k] = br[k + 1];
                }
                if (r + 1 + BAH < R - 1) {
                    bl[BAH - 1] = bperm(laddr, vo[r + 1 + BAH]);
                    br[BAH - 1] = bperm(raddr, ve[r + 1 + BAH]);
                }
                __builtin_amdgcn_sched_barrier(0);
                BitEnc::pair_sums(ve[r + 1], vo[r + 1], l, rr, ne0, ne1, no0, no1);
            } else {
                hsum(ve[r + 1], vo[r + 1], ne0, ne1, no0, no1);
            }
            ve[r] = rule(pe0, pe1, ce0, ce1, ne0, ne1, ve[r]);
            vo[r] = rule(po0, po1, co0, co1, no0, no1, vo[r]);
            pe0 = ce0;
            pe1 = ce1;
            po0 = co0;
            po1 = co1;
            ce0 = ne0;
            ce1 = ne1;
            co0 = no0;
            co1 = no1;
        }
        {
            // the wave below (slot NW + 1 below the window: zero)
            const uint32_t de0 = xch[par][wi + 2][0][lane], de1 = xch[par][wi + 2][1][lane];
            const uint32_t do0 = xch[par][wi + 2][2][lane], do1 = xch[par][wi + 2][3][lane];
            ve[R - 1] = rule(pe0, pe1, ce0, ce1, de0, de1, ve[R - 1]);
            vo[R - 1] = rule(po0, po1, co0, co1, do0, do1, vo[R - 1]);
        }
        if (POP) {
            // generation g + 1 of the pass: the cells this wave will store (st and the row tests
            // below, without the xext apron pairs), inside the counted rows [pa->y0, pa->y1)
            int l3 = (int)(threadIdx.x & 63);
            asm volatile("" : "+v"(l3));
            const int gl3 = BAND ? l3 >> gsh : 0;
            const int pin3 = BAND ? l3 & ((1 << gsh) - 1) : l3;
            const bool own3 = BAND ? (pin3 >= 1 && pin3 <= own && gl3 < nb)
                                   : (l3 >= 1 && l3 <= 62 && tx * 62 + l3 - 1 < a.W);
            // Straight-line code, no test per row: every row's two popcounts times its bit of the row
            // mask (v_bcnt x 2 and a v_cndmask; the bit is scalar in a plain tile).  A branch here, even
            // a wave-uniform one around the rows a wave does not own, split the loop body, the compiler
            // hoisted the permutes above it and spilled 100-150 VGPRs.
            const uint32_t rm = BAND ? pop_rows(y0 + (int64_t)(gl3 < nb ? gl3 : 0) * T) : rm_s;
            uint32_t c = 0u;
#pragma unroll
            for (int r = 0; r < R; ++r)
                c = __umul24((uint32_t)__popc(ve[r]) + (uint32_t)__popc(vo[r]), (rm >> r) & 1u) + c;
            if (!own3) c = 0u;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);  // < 2^17: 64 lanes x R rows x 64 cells
            if (l3 == 0) pl[g * NW + wi] = c;
        }
    }
    if (LIFE_WG_TRACE && !FLOW) wg_trace(3, 64);  // generations done
    // window rows [K, NW*R - K) are the tile's owned rows [ty*T, ty*T + T);
    // this wave's share of them (a half-height tile's ghost rows may span more
    // than one wave: K > R)
    const int r0 = min(max(K - wi * R, 0), R), r1 = min(max(NW * R - K - wi * R, 0), R);
    // Which lanes store, recomputed here from the lane id (the empty asm
    // makes it a fresh value): nothing per-lane but voff and the window lives
    // across the generation loop.  Extra live state there (the deep-halo
    // apron-pair test kept the 64-bit column index alive) made the compiler
    // issue each row's ds_bpermute right before its use and cost 2-8 % of the
    // launch (tests/test_isa.py).  The apron pairs of a
    // deep-halo pass (Extend::x) exist only on a partitioned x axis.
    int lane2 = (int)(threadIdx.x & 63);
    asm volatile("" : "+v"(lane2));
    const int gl2 = BAND ? lane2 >> gsh : 0;
    const int pin2 = BAND ? lane2 & ((1 << gsh) - 1) : lane2;
    const int j2 = (BAND ? org : tx * 62) + pin2 - 1;
    const bool st = (BAND ? (pin2 >= 1 && pin2 <= own && gl2 < nb)
                          : (lane2 >= 1 && lane2 <= 62 && j2 < (int)a.W)) ||
                    (!WRAPX && a.xext && (!BAND || gl2 < nb) && (j2 == -1 || j2 == (int)a.W));
    const int yb = y0 + (BAND ? (gl2 < nb ? gl2 : 0) * T : 0);  // this lane's band
    const int ylim = yend >= 0 ? yend : (int)a.h;  // half tiles of a region stop at its last row
    uint8_t *q = out + (a.ya + yb + r0) * a.pitch + voff;
    auto store_row = [&](int r) {
        const uint64_t v = (uint64_t)ve[r] | ((uint64_t)vo[r] << 32);
        if (FLOW == 1)
            __hip_atomic_store(reinterpret_cast<uint64_t *>(q), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            *reinterpret_cast<uint64_t *>(q) = v;
    };
    // ACT: the row masks (life_act.h) of what this wave stores in map rows ar0 and ar0 + 1, wave-uniform
    uint32_t am[2][kActWords] = {};
    const int ar0 = ACT ? (yb + r0) / kActRows : 0;
    const int llast = ACT ? min(kActPairs, (int)a.W - tx * kActPairs) : 0;  // lane of the last owned pair
    // A plain tile's wave that holds no ghost row and ends inside the stored
    // rows (every wave but those at a window's ends, in every tile row but a
    // cut last one) stores its R rows under one lane mask, in one basic
    // block; the others test each row (a wave of ghost rows only: none).
    if (LIFE_TILE_STRAIGHT && !BAND && !ACT && r0 == 0 && r1 == R && yb + R <= ylim) {
        if (st) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                store_row(r);
                q += a.pitch;
            }
        }
    } else if (r0 < r1) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r < r0 || r >= r1) continue;
            if (st && yb + r < ylim) store_row(r);
            if (ACT && yb + r < ylim) {  // (uniform: every lane of the wave is here)
                const unsigned long long nz = __ballot(st && (ve[r] | vo[r]) != 0u);
                const uint32_t bit = 1u << ((yb + r) % kActRows);
                const int k = (yb + r) / kActRows == ar0 ? 0 : 1;
                if (nz) am[k][kActAny] |= bit;
                if ((nz >> 1) & 1ull) am[k][kActFirst] |= bit;  // lane 1 holds pair 62 tx
                if ((nz >> llast) & 1ull) am[k][kActLast] |= bit;
            }
            q += a.pitch;
        }
    }
    if (LIFE_WG_TRACE && !FLOW) wg_trace(4, 64);  // stores issued
    if (ACT && lane2 == 0) {
        // stored rows are owned rows (< h): a nonzero mask's map row exists.  Waves (24 rows) and
        // vertically adjacent tiles share 32-row words: OR, not store.
        const int64_t ncol = act_cols(a.W);
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int w = 0; w < kActWords; ++w)
                if (am[k][w]) atomicOr(act + act_word(ar0 + k, tx, ncol, w), am[k][w]);
    }
    if (POP) {
        // one wave, a lane per generation: the workgroup's counts into its stripe (a dead tile adds nothing)
        __syncthreads();
        if (wi == 0 && lane2 < a.m) {
            uint32_t c = 0u;
#pragma unroll
            for (int w = 0; w < NW; ++w) c += pl[lane2 * NW + w];
            if (c)
                atomicAdd(pa->cnt + (int64_t)(blockIdx.x & (kPopStripes - 1)) * kPopGens + lane2,
                          (unsigned long long)c);
        }
    }
}

// Waves per SIMD the byte tiles are compiled for (LIFE_BYTE_WPE, compile
// time, A/B): 4 = 2 tiles of 8 waves per CU (up to 128 VGPRs), 6 = 3 tiles
// (80 VGPRs: the load / compute / store phases of three tiles overlap).
#ifndef LIFE_BYTE_WPE
#define LIFE_BYTE_WPE 4
#endif
#ifndef LIFE_BYTE_LOAD_CHUNK
#define LIFE_BYTE_LOAD_CHUNK 0
#endif
// LIFE_BYTE_BP_AHEAD: the generation loop's left-neighbour permutes are
// issued this many rows ahead of their use, the rows fenced in program order
// (LIFE_BYTE_BP_FENCE; unfenced, the compiler sinks every permute next to
// its use and waits for it).  A tile spends 33 us loading, 93 us in its
// generations, 4 us storing (scripts/wg_trace.py, profiles/r04/byte_ab):
// 2 ahead measured 2.29-2.30 against 2.33-2.36 ms per 32-generation launch
// (4 ahead 2.32, profiles/r04/byte_ab).
#ifndef LIFE_BYTE_BP_AHEAD
#define LIFE_BYTE_BP_AHEAD 2
#endif
#ifndef LIFE_BYTE_BP_FENCE
#define LIFE_BYTE_BP_FENCE 1
#endif
// Byte tiles: lane l of a tile holds word column 62 tx + l - 1 -- 32 byte
// cells, packed into one register word per row by v_dot4_u32_u8 on load
// (two 16-B loads) and unpacked on store -- in the drifting frame
// (bit_hsum_drift: left neighbour only, 12 VALU + 1 LDS per row and
// generation; +2 % over the centred frame for bytes,
// profiles/r01/drift_ab.jsonl).  GK ghost rows per window end, compile-time
// (a runtime depth measured 29 % slower here, profiles/r02/ghost_ab.txt).
// The same window / exchange / barrier scheme as the bit tiles.
template <int R, int GK, bool WRAPX, bool WRAPY, int NW>
__device__ __forceinline__ void tile_body_byte(const TArgs &a, const uint8_t *in, uint8_t *out, int64_t tx,
                                               int64_t ty, Xch<NW> &xch) {
    static_assert(R >= 3 && GK >= 1 && GK <= 32, "window");
    constexpr int K = GK;
    constexpr int T = NW * R - 2 * K;
    const int lane = threadIdx.x & 63;
    const int laddr = ((lane - 1) & 63) << 2;
    const int wi = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j = tx * 62 + lane - 1;  // word column of this lane
    int64_t jl;
    if (WRAPX) {
        if (LIFE_FAST_WRAP && a.W >= 64) {  // j in [-1, W + 62), as tile_body_bit
            jl = j < 0 ? j + a.W : (j >= a.W ? j - a.W : j);
        } else {
            jl = j % a.W;
            if (jl < 0) jl += a.W;
        }
    } else {
        jl = j > a.W ? a.W : j;
    }
    const uint32_t voff = (uint32_t)(a.xoff + 32 * jl);
    const int64_t y0 = ty * T - K + (int64_t)wi * R;
    const uint8_t *row0 = in + a.ya * a.pitch;
    uint32_t v[R];
    {
        int64_t y = y0;
        if (WRAPY) {
            if (LIFE_FAST_WRAP && a.h >= 2 * (int64_t)(NW * R) + 64) {  // y in [-K, h + T)
                y = y < 0 ? y + a.h : (y >= a.h ? y - a.h : y);
            } else {
                y %= a.h;
                if (y < 0) y += a.h;
            }
        }
        const uint8_t *p = row0 + y * a.pitch;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // LIFE_BYTE_LOAD_CHUNK rows of loads in flight at most: a
            // scheduling fence after every chunk keeps the load phase's
            // registers (8 per row in flight) inside the occupancy budget
            if (LIFE_BYTE_LOAD_CHUNK > 0 && r > 0 && r % (LIFE_BYTE_LOAD_CHUNK > 0 ? LIFE_BYTE_LOAD_CHUNK : 1) == 0)
                __builtin_amdgcn_sched_barrier(0);
            const uint4 *q = reinterpret_cast<const uint4 *>(p + voff);
            v[r] = pack32(q[0], q[1]);
            ++y;
            if (WRAPY && y == a.h) {
                y = 0;
                p = row0;
            } else {
                p += a.pitch;
            }
        }
    }
    for (int g = 0; g < a.m; ++g) {
        const int par = g & 1;
        uint32_t t0, t1, b0, b1, tL, bL;  // xL: the row's own cells in the drifting frame
        bit_hsum_drift(v[0], laddr, t0, t1, tL);
        bit_hsum_drift(v[R - 1], laddr, b0, b1, bL);
        xch[par][wi][0][lane] = t0;
        xch[par][wi][1][lane] = t1;
        xch[par][wi][2][lane] = b0;
        xch[par][wi][3][lane] = b1;
        __syncthreads();
        if (g == 0) wg_trace(1);  // window loaded, first generation's sums published
        uint32_t a0 = 0u, a1 = 0u, d0 = 0u, d1 = 0u;
        if (wi > 0) {
            a0 = xch[par][wi - 1][2][lane];
            a1 = xch[par][wi - 1][3][lane];
        }
        if (wi < NW - 1) {
            d0 = xch[par][wi + 1][0][lane];
            d1 = xch[par][wi + 1][1][lane];
        }
        uint32_t p0 = t0, p1 = t1, c0, c1, cL;
        bit_hsum_drift(v[1], laddr, c0, c1, cL);
        const uint32_t h10 = c0, h11 = c1;
        // LIFE_BYTE_BP_AHEAD rows' left-neighbour words in flight ahead of
        // their use (0: each fetched in its own row)
        constexpr int AH = LIFE_BYTE_BP_AHEAD;
        uint32_t ahead[AH > 0 ? AH : 1];
#pragma unroll
        for (int k = 0; k < AH; ++k)
            if (2 + k < R - 1) ahead[k] = bperm(laddr, v[2 + k]);
#pragma unroll
        for (int r = 1; r < R - 1; ++r) {
            uint32_t n0, n1, nL;
            if (r + 1 == R - 1) {
                n0 = b0;
                n1 = b1;
                nL = bL;
            } else if (AH > 0) {
                const uint32_t l = ahead[0];
#pragma unroll
                for (int k = 0; k + 1 < AH; ++k) ahead[k] = ahead[k + 1];
                if (r + 1 + AH < R - 1) ahead[AH - 1] = bperm(laddr, v[r + 1 + AH]);
                // rows stay in program order: the compiler would otherwise
                // sink every permute next to its use again
                if (LIFE_BYTE_BP_FENCE) __builtin_amdgcn_sched_barrier(0);
                nL = __builtin_amdgcn_alignbit(v[r + 1], l, 31);
                BitEnc::fa(__builtin_amdgcn_alignbit(v[r + 1], l, 30), nL, v[r + 1], n0, n1);
            } else {
                bit_hsum_drift(v[r + 1], laddr, n0, n1, nL);
            }
            v[r] = BitEnc::rule1(p0, p1, c0, c1, n0, n1, cL);
            cL = nL;
            p0 = c0;
            p1 = c1;
            c0 = n0;
            c1 = n1;
        }
        v[R - 1] = BitEnc::rule1(p0, p1, b0, b1, d0, d1, bL);
        v[0] = BitEnc::rule1(a0, a1, t0, t1, h10, h11, tL);
    }
    wg_trace(2);  // generations done
    const int r0 = min(max(K - wi * R, 0), R), r1 = min(max(NW * R - K - wi * R, 0), R);
    const bool st = lane >= 1 && lane <= 62 && j < a.W;
    uint8_t *q = out + (a.ya + y0 + r0) * a.pitch + voff;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < r0 || r >= r1) continue;
        v[r] = drift_realign(v[r], a.m);  // every lane: the bpermute reads lane + 1
        if (st && y0 + r < a.h) {
            uint4 *o = reinterpret_cast<uint4 *>(q);
            o[0] = unpack_half(v[r], 0);
            o[1] = unpack_half(v[r], 1);
        }
        q += a.pitch;
    }
    wg_trace(3);  // stores issued
}

// Waves per SIMD the bit tiles are compiled for (the VGPR budget): 3 tiles
// of 8 waves or 2 of 12 per CU at <= 80 VGPRs; 16-wave tiles: 2 per CU at 64
// (R = 16) or 1 at 128.
constexpr int bit_wpe(int NW, int R) { return NW == 16 ? (R <= 16 ? 8 : 4) : (R <= 24 ? 6 : 4); }

// Banded item i of a region's last tile column: tile rows [ty0, ty0 + rows)
// as the items of sub-column 0 (ceil(rows / B_0), B_i = 64 >> bgsh[i] tile
// rows each), then those of sub-column 1.  Wave-uniform throughout.
template <int RS, bool WRAPX, bool WRAPY, int NW, class RP = ConwayRule, bool POP = false>
__device__ __forceinline__ void band_item(const TArgs &a, int i, int ty0, int rows, XchB<NW> &xch, int ybase = 0,
                                          int yend = -1, const RP &rule = RP{}, const PopArgs *pa = nullptr,
                                          uint32_t *pl = nullptr) {
    const int n0 = (rows + (64 >> a.bgsh[0]) - 1) >> (6 - a.bgsh[0]);
    const bool second = a.nband > 1 && i >= n0;
    if (second) i -= n0;
    const int gsh = second ? a.bgsh[1] : a.bgsh[0], own = second ? a.bown[1] : a.bown[0];
    const int org = (int)(second ? a.borg[1] : a.borg[0]);
    const int B = 64 >> gsh, t = i * B;  // first tile row of the item within the region
    const int nb = rows - t < B ? rows - t : B;
    if (POP)
        tile_body_bit<RS, WRAPX, WRAPY, 0, NW, true, RP, false, POP>(a, a.in, a.out, 0, ty0 + t, xch, gsh, nb, ybase,
                                                                     yend, org, own, rule, nullptr, pa, pl);
    else
        tile_body_bit<RS, WRAPX, WRAPY, 0, NW, true>(a, a.in, a.out, 0, ty0 + t, xch, gsh, nb, ybase, yend, org, own,
                                                     rule);
}

// One workgroup per item (life_tile_decode.h: which one, from the launch's
// constants in 32-bit arithmetic): a tile, a banded item, or an item of the
// tail (TArgs::tail_*) -- RS = R / 2 rows per wave, tile rows of TS = NW RS -
// 2m owned rows from owned row tail_y, the last one stopping at tail_yend;
// per tile row the ordinary tiles from column tail_tx0, then the banded items
// of the last tile column.  (Round 5's half tiles spanned the last column as
// full-width tiles; banded they take (64 - o - 2) / 64 fewer lanes there.)
// One call site per kind: four copies of the generation loop, as before.
template <int R, bool WRAPX, bool WRAPY, int NW, class RP, bool POP = false>
__device__ __forceinline__ void tstep_bit_items(const TArgs &a, XchB<NW> &xch, const RP &rule,
                                                const PopArgs *pa = nullptr, uint32_t *pl = nullptr) {
    wg_trace(0);
    const TileItem it = tile_decode(a.d, blockIdx.x);
    if (it.kind == kTileNone) return;  // whole workgroup
    const bool tail = it.kind == kTileTail || it.kind == kTileTailBand;
    const int ybase = tail ? (int)a.tail_y : 0, yend = tail ? (int)a.tail_yend : -1;
    if (it.kind == kTileFull) {
        if (POP)
            tile_body_bit<R, WRAPX, WRAPY, 0, NW, false, RP, false, POP>(a, a.in, a.out, it.tx, it.ty, xch, 6, 1, 0, -1,
                                                                         0, 62, rule, nullptr, pa, pl);
        else
            tile_body_bit<R, WRAPX, WRAPY, 0, NW>(a, a.in, a.out, it.tx, it.ty, xch, 6, 1, 0, -1, 0, 62, rule);
    } else if (it.kind == kTileBand) {
        band_item<R, WRAPX, WRAPY, NW, RP, POP>(a, (int)it.bi, it.ty0, it.rows, xch, 0, -1, rule, pa, pl);
    } else if (it.kind == kTileTail) {
        if (POP)
            tile_body_bit<R / 2, WRAPX, WRAPY, 0, NW, false, RP, false, POP>(a, a.in, a.out, it.tx, it.ty, xch, 6, 1,
                                                                             ybase, yend, 0, 62, rule, nullptr, pa, pl);
        else
            tile_body_bit<R / 2, WRAPX, WRAPY, 0, NW>(a, a.in, a.out, it.tx, it.ty, xch, 6, 1, ybase, yend, 0, 62,
                                                      rule);
    } else {
        band_item<R / 2, WRAPX, WRAPY, NW, RP, POP>(a, (int)it.bi, 0, it.rows, xch, ybase, yend, rule, pa, pl);
    }
    wg_trace(1);
}

template <int R, bool WRAPX, bool WRAPY, int NW>
__global__ __launch_bounds__(64 * NW, bit_wpe(NW, R)) void tstep_bit_kernel(TArgs a) {
    __shared__ XchB<NW> xch;
    tstep_bit_items<R, WRAPX, WRAPY, NW>(a, xch, ConwayRule{});
}

// The same tiles with B3/S23 in 7 gates per dword (ConwayRule7, life_bitops.h;
// LIFE_OPT_RULE7): per pair row 2 v_alignbit + 2 full adders (4) + 2 x 7 = 20
// VALU against tstep_bit_kernel's 22, under the same launch bounds (80 VGPRs
// at 3 tiles per CU) and over the same items; tests/test_isa_rule7.py pins
// the count and the schedule.
// A kernel of its own name: tstep_bit_kernel stays in the build, its text and
// code untouched, as the A/B arm (LIFE_RULE7=0) and the instance
// tests/test_isa.py reads.  The model behind kernel_work() keeps counting 22
// per pair row for both arms (tstep_valu_per_tile_lane).
template <int R, bool WRAPX, bool WRAPY, int NW>
__global__ __launch_bounds__(64 * NW, bit_wpe(NW, R)) void tstep_bit7_kernel(TArgs a) {
    __shared__ XchB<NW> xch;
    tstep_bit_items<R, WRAPX, WRAPY, NW>(a, xch, ConwayRule7{});
}

// The same tiles under a table rule (life_dev_set_rule): the tail is 25
// v_bitop3 per dword instead of 12 and its 20 uniform words live in VGPRs,
// so the instance is compiled for 2 tiles per CU (4 waves per SIMD, at most
// 128 VGPRs) rather than squeezed into the 80 of 3 tiles.  VALU per pair row
// and generation: 2 v_alignbit + 2 full adders (4) + 2 x 25 =
// kRuleValuPerPairRow (life_kernels.h; pinned against the code object by
// tests/test_isa_rule.py).
// (LIFE_RULE_WPE, compile time, A/B: 6 = 3 tiles per CU at <= 80 VGPRs)
#ifndef LIFE_RULE_WPE
#define LIFE_RULE_WPE 4
#endif
struct RTArgs {
    TArgs t;
    RuleWords w;
};
// Waves per SIMD the B3/S23 census instances are compiled for (LIFE_POP_WPE,
// compile time, A/B): 6 = 3 tiles per CU at <= 80 VGPRs, as the plain tiles
// (the launch-tail plans count the same slots), 4 = 2 tiles at <= 128.
#ifndef LIFE_POP_WPE
#define LIFE_POP_WPE 6
#endif
template <int R, bool WRAPX, bool WRAPY, int NW>
__global__ __launch_bounds__(64 * NW, LIFE_RULE_WPE) void trule_bit_kernel(RTArgs a) {
    __shared__ XchB<NW> xch;
    tstep_bit_items<R, WRAPX, WRAPY, NW>(a.t, xch, TableRule(a.w));
}

// The census instances of both (PopArgs): the same items through the same
// dispatch, each tile also counting what it owns after every generation.
struct PTArgs {
    TArgs t;
    PopArgs p;
};
template <int R, bool WRAPX, bool WRAPY, int NW>
__global__ __launch_bounds__(64 * NW, LIFE_POP_WPE) void tpop_bit_kernel(PTArgs a) {
    __shared__ XchB<NW> xch;
    __shared__ uint32_t pl[kPopGens * NW];
    tstep_bit_items<R, WRAPX, WRAPY, NW, ConwayRule, true>(a.t, xch, ConwayRule{}, &a.p, pl);
}
struct RPTArgs {
    TArgs t;
    RuleWords w;
    PopArgs p;
};
template <int R, bool WRAPX, bool WRAPY, int NW>
__global__ __launch_bounds__(64 * NW, LIFE_RULE_WPE) void tpop_rule_kernel(RPTArgs a) {
    __shared__ XchB<NW> xch;
    __shared__ uint32_t pl[kPopGens * NW];
    tstep_bit_items<R, WRAPX, WRAPY, NW, TableRule, true>(a.t, xch, TableRule(a.w), &a.p, pl);
}

// ---- skip-dead passes (LIFE_OPT_SKIP_DEAD; DESIGN.md 5.9, life_act.h)
// A pass over a single shard whose axes both wrap in the stencil runs only
// the tiles whose input window may hold a live cell: nothing is born from
// nothing (B0 rules are refused), so a tile whose window is dead produces a
// dead block.  Three stream-ordered steps per pass (launch_tskip):
//  1. act_plan_kernel, a thread per tile of the plain tile grid (no banded
//     column, no tail split): the tile is kActRun if any cell of the input
//     buffer's map under its window is set, else kActClear if any cell of the
//     output buffer's OLD map under its owned rows is set, else kActSkip; the
//     three counts go to the call's counters;
//  2. the output buffer's map is zeroed (only now: step 1 has read it);
//  3. tskip_*_kernel, a workgroup per tile, reads its class before anything
//     else: kActSkip returns (the whole workgroup, before any barrier),
//     kActClear stores zeros over its owned rows and pairs and nothing else,
//     kActRun is tile_body_bit as a plain tile with the ACT flag.
struct PlanArgs {
    const uint32_t *src_map, *dst_map;
    uint8_t *cls;
    unsigned long long *cnt;  // run, cleared, skipped
    int64_t W, h, T, ntx, nty;
    int32_t m;
};
__global__ __launch_bounds__(256) void act_plan_kernel(PlanArgs p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int c = -1;  // past the last tile
    if (i < p.ntx * p.nty) {
        const int64_t tx = i % p.ntx, ty = i / p.ntx;
        if (act_window_live(p.src_map, p.W, act_read_rows(ty, p.T, p.m, p.h), tx))
            c = kActRun;
        else if (act_own_live(p.dst_map, p.W, act_own_rows(ty, p.T, p.h), tx))
            c = kActClear;
        else
            c = kActSkip;
        p.cls[i] = (uint8_t)c;
    }
    const unsigned long long run = __ballot(c == kActRun), clr = __ballot(c == kActClear),
                             skp = __ballot(c == kActSkip);
    if ((threadIdx.x & 63) == 0) {
        if (run) atomicAdd(p.cnt, (unsigned long long)__popcll(run));
        if (clr) atomicAdd(p.cnt + 1, (unsigned long long)__popcll(clr));
        if (skp) atomicAdd(p.cnt + 2, (unsigned long long)__popcll(skp));
    }
}

struct KArgs {
    TArgs t;
    const uint8_t *cls;  // class per tile, row-major over ntx x nty
    uint32_t *act;       // the output buffer's map, zeroed
    int64_t ntx, nty;
    uint32_t ntx_mul;    // tile_recip(ntx): the tile of a workgroup without a division
};
template <int R, int NW, class RP, bool POP = false>
__device__ __forceinline__ void tskip_body(const KArgs &k, XchB<NW> &xch, const RP &rule,
                                           const PopArgs *pa = nullptr, uint32_t *pl = nullptr) {
    const TArgs &a = k.t;
    const uint32_t wg = blockIdx.x;  // (tiles < 2^31: launch_tskip)
    if (wg >= (uint32_t)k.ntx * (uint32_t)k.nty) return;
    const int c = __builtin_amdgcn_readfirstlane((int)k.cls[wg]);
    if (c == kActSkip) return;  // whole workgroup, uniform, before any barrier
    uint32_t qy, rx;
    tile_divmod(wg, (uint32_t)k.ntx, k.ntx_mul, qy, rx);
    const int tx = (int)rx, ty = (int)qy;
    if (c == kActClear) {
        const int64_t T = (int64_t)NW * R - 2 * a.m;
        const int64_t ya = ty * T, yb = act_own_end(ty, T, a.h);
        const int lane = threadIdx.x & 63;
        const int64_t j = tx * kActPairs + lane;
        if (lane < kActPairs && j < a.W)
            for (int64_t y = ya + (threadIdx.x >> 6); y < yb; y += NW)
                *reinterpret_cast<uint64_t *>(a.out + (a.ya + y) * a.pitch + a.xoff + 8 * j) = 0ull;
        return;
    }
    if (POP)
        tile_body_bit<R, true, true, 0, NW, false, RP, true, POP>(a, a.in, a.out, tx, ty, xch, 6, 1, 0, -1, 0, 62,
                                                                  rule, k.act, pa, pl);
    else
        tile_body_bit<R, true, true, 0, NW, false, RP, true>(a, a.in, a.out, tx, ty, xch, 6, 1, 0, -1, 0, 62, rule,
                                                             k.act);
}
template <int R, int NW>
__global__ __launch_bounds__(64 * NW, bit_wpe(NW, R)) void tskip_bit_kernel(KArgs k) {
    __shared__ XchB<NW> xch;
    tskip_body<R, NW>(k, xch, ConwayRule{});
}
struct RKArgs {
    KArgs k;
    RuleWords w;
};
template <int R, int NW>
__global__ __launch_bounds__(64 * NW, LIFE_RULE_WPE) void tskip_rule_kernel(RKArgs a) {
    __shared__ XchB<NW> xch;
    tskip_body<R, NW>(a.k, xch, TableRule(a.w));
}
// their census instances
struct PKArgs {
    KArgs k;
    PopArgs p;
};
template <int R, int NW>
__global__ __launch_bounds__(64 * NW, LIFE_POP_WPE) void tpop_skip_kernel(PKArgs a) {
    __shared__ XchB<NW> xch;
    __shared__ uint32_t pl[kPopGens * NW];
    tskip_body<R, NW, ConwayRule, true>(a.k, xch, ConwayRule{}, &a.p, pl);
}
struct RPKArgs {
    KArgs k;
    RuleWords w;
    PopArgs p;
};
template <int R, int NW>
__global__ __launch_bounds__(64 * NW, LIFE_RULE_WPE) void tpop_skip_rule_kernel(RPKArgs a) {
    __shared__ XchB<NW> xch;
    __shared__ uint32_t pl[kPopGens * NW];
    tskip_body<R, NW, TableRule, true>(a.k, xch, TableRule(a.w), &a.p, pl);
}

// Folds the stripes of a pass into the trace and zeroes them: block g < m
// stores the sum of generation g's counters to trace[g]; every block (the
// launch has kPopGens) leaves its counters zero for the next pass.
__global__ __launch_bounds__(64) void pop_fold_kernel(unsigned long long *cnt, unsigned long long *trace, int m) {
    const int g = blockIdx.x;
    unsigned long long c = 0;
    for (int s = threadIdx.x; s < kPopStripes; s += 64) {
        c += cnt[(int64_t)s * kPopGens + g];
        cnt[(int64_t)s * kPopGens + g] = 0ull;
    }
    for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);
    if (threadIdx.x == 0 && g < m) trace[g] = c;
}

template <int R, int GK, bool WRAPX, bool WRAPY, int NW>
__global__ __launch_bounds__(64 * NW, LIFE_BYTE_WPE) void tstep_byte_kernel(TArgs a) {
    __shared__ Xch<NW> xch;
    wg_trace(0);
    // per-XCD row-major runs and regions as the bit tiles (no bands, no tail: every item is a tile)
    const TileItem it = tile_decode(a.d, blockIdx.x);
    if (it.kind != kTileFull) return;
    tile_body_byte<R, GK, WRAPX, WRAPY, NW>(a, a.in, a.out, it.tx, it.ty, xch);
}

// tflow_kernel: `passes` launches of the bit tiles (m generations each, both
// axes periodic inside one shard) as ONE persistent launch.  Workgroups pull
// work items (pass p, tile) in order from a queue head; a tile of pass p > 0
// starts once every tile whose rows its window reads -- tile rows ty-2..ty+2
// (a short last tile row lets a window reach two rows over), columns
// tx-1..tx+1, periodic -- has finished pass p-1, which also guarantees that no
// reader of the rows it overwrites (pass p-1 of the same tiles) is still
// running.  Pass p walks the tile rows from row p (mod nty), so the rows a
// tile waits for were pulled about a whole pass earlier: no pass boundary
// drains the chip (the per-launch ramp and tail of tstep_kernel, ~48 us).
// Deadlock-free without co-residency: an item waits only on items pulled
// before it, and a pulled item is running on a resident workgroup.
// Hand-off (MI355X_MICROARCH.md, inter-workgroup visibility, row 1): the
// window rows are loaded `sc1`; every storing wave waits vmcnt(0), then a
// workgroup barrier, then one lane stores the tile's pass count `sc1`; the
// polling wave's lanes read the flags `sc1`, a barrier, then every wave loads.
struct FArgs {
    TArgs t;                         // geometry, m; t.in / t.out: buffers of pass 0
    int64_t ntx, nty, items;         // items = passes * per_pass
    // BAND: the last tile column (t.btx1 - 1; one sub-column) as banded items
    // of B = 64 >> t.bgsh[0] tile rows; a pass is ngroups groups of B tile
    // rows, each (ntx - 1) * B ordinary items then one banded item (tile rows
    // past nty: no-op items)
    int64_t per_pass, ngroups, B;
    unsigned int *head;              // queue head (zeroed before the launch), then an error word: 1 + the
                                     // last item whose dependency wait timed out (0: none)
    unsigned int *done;              // per tile: passes completed (zeroed before the launch)
};

// BAND (a last tile column owning o <= 30 pairs: 32768^2's 16, 16384^2's
// 8): that column runs as banded items, as tstep_bit_kernel does, instead of
// full-width tiles that waste (64 - o - 2) / 64 of their lanes.  Without it
// the instance has no banded code in its loop (the banded items cost the
// ordinary tiles 2.5 % there, code size in the persistent loop;
// profiles/r02/r2x).
template <int R, bool WRAPX, bool WRAPY, int FLOW, int NW, bool BAND = false>
__global__ __launch_bounds__(64 * NW, bit_wpe(NW, R)) void tflow_kernel(FArgs f) {
    __shared__ XchB<NW> xch;
    __shared__ unsigned int item_sh;
    const TArgs &a = f.t;
    const int64_t tiles = f.ntx * f.nty;
    const int lane = threadIdx.x & 63;
    unsigned int *prev_flag = nullptr;  // wave 0, lanes < prev_n: the finished item's tile counters
    unsigned int prev_val = 0;
    int prev_n = 0;
    int traced = 0;  // diagnostics builds: items 0..3 stamp pulled / dependencies met / stored
    wg_trace(0);
    for (;;) {
        // ONE thread-0 region per iteration, behind the barrier that closes
        // the previous item: publish that item (its stores were drained by
        // every wave before the barrier), then pull the next.  (Two thread-0
        // regions on either side of the loop's back edge were merged by the
        // compiler into a region that lanes 1..63 of wave 0 never wait for:
        // the workgroup then re-ran its item forever.)
        if (!BAND && threadIdx.x == 0) {
            if (prev_flag) {
                if (FLOW == 2) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __hip_atomic_store(prev_flag, prev_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            item_sh = atomicAdd(f.head, 1u);
        }
        if (BAND && threadIdx.x < 64) {  // one wave-0 region: a banded item publishes its nb tiles
            if (prev_n > 0) {
                if (FLOW == 2) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                if (lane < prev_n)
                    __hip_atomic_store(prev_flag + (int64_t)lane * f.ntx, prev_val, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
            if (lane == 0) item_sh = atomicAdd(f.head, 1u);
        }
        __syncthreads();
        // uniform: scalar registers, scalar arithmetic
        const uint32_t item = __builtin_amdgcn_readfirstlane(item_sh);
        if ((int64_t)item >= f.items) return;  // the whole workgroup leaves
        if (LIFE_WG_TRACE && traced < 4) wg_trace(1 + 3 * traced);
        const uint32_t ntx = (uint32_t)f.ntx, nty = (uint32_t)f.nty;
        uint32_t p;
        int64_t tx, ty;
        int nb = 1;  // tile rows of this item (a banded item: up to B)
        if (!BAND) {
            p = item / (uint32_t)tiles;
            const uint32_t k = item - p * (uint32_t)tiles, kr = k / ntx;
            tx = k - kr * ntx;
            ty = (kr + p) % nty;
        } else {
            p = item / (uint32_t)f.per_pass;
            const uint32_t k = item - p * (uint32_t)f.per_pass;
            const uint32_t nfull = ntx - 1, G1 = nfull * (uint32_t)f.B + 1u;
            const uint32_t g = k / G1, off = k - g * G1;
            const int64_t ty0 = (int64_t)((g + p) % (uint32_t)f.ngroups) * f.B;  // groups rotate per pass
            if (off < nfull * (uint32_t)f.B) {
                tx = off % nfull;
                ty = ty0 + off / nfull;
            } else {
                tx = a.btx1 - 1;
                ty = ty0;
                nb = (int)(f.nty - ty0 < f.B ? f.nty - ty0 : f.B);
            }
            if (ty >= f.nty) {  // a padding item of the last group
                prev_n = 0;
                prev_flag = nullptr;
                __syncthreads();  // item_sh is rewritten by the next pull
                continue;
            }
        }
        if (p > 0 && threadIdx.x < 64) {
            // tile rows ty-2 .. ty+nb+1 x columns tx-1..tx+1 (one lane each)
            bool ok = true;
            const unsigned int *flag = nullptr;
            if (lane < 3 * (nb + 4)) {
                const int64_t dy = lane / 3 - 2, dx = lane % 3 - 1;
                int64_t yy = (ty + dy) % f.nty, xx = (tx + dx) % f.ntx;
                if (yy < 0) yy += f.nty;
                if (xx < 0) xx += f.ntx;
                flag = f.done + yy * f.ntx + xx;
            }
            // bounded: a wait of ~seconds means a broken invariant; record it
            // (the host reports it at the next sync) rather than hang the GPU
            for (uint32_t spin = 0;; ++spin) {
                if (flag)
                    ok = __hip_atomic_load(const_cast<unsigned int *>(flag), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT) >= p;
                if (__all(ok)) break;
                if (spin == (1u << 20)) {
                    if (lane == 0) atomicMax(f.head + 1, item + 1);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (FLOW == 2) {  // plain producer stores: the valid form needs the acquire
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        if (LIFE_WG_TRACE && traced < 4) wg_trace(2 + 3 * traced);
        const uint8_t *in = (p & 1) ? a.out : a.in;
        uint8_t *out = const_cast<uint8_t *>((p & 1) ? a.in : a.out);
        if (BAND && tx == a.btx1 - 1)
            tile_body_bit<R, WRAPX, WRAPY, FLOW, NW, true>(a, in, out, tx, ty, xch, a.bgsh[0], nb, 0, -1, a.borg[0],
                                                           a.bown[0]);
        else
            tile_body_bit<R, WRAPX, WRAPY, FLOW, NW>(a, in, out, tx, ty, xch);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have left
        __syncthreads();
        if (LIFE_WG_TRACE && traced < 4) wg_trace(3 + 3 * traced++);
        prev_flag = f.done + ty * f.ntx + tx;
        prev_val = p + 1;
        prev_n = nb;
    }
}

// tflow_kernel again under a rule policy, for the 7-gate arm below (a twin for
// the reason given at step_body: tflow_kernel keeps its own text and so
// its code, the A/B arm and the instance tests/test_isa.py reads).  Queue,
// dependency wait and hand-off are tflow_kernel's, line for line.
template <int R, bool WRAPX, bool WRAPY, int FLOW, int NW, bool BAND, class RP>
__device__ __forceinline__ void tflow_body(const FArgs &f, XchB<NW> &xch, unsigned int &item_sh, const RP &rule) {
    const TArgs &a = f.t;
    const int64_t tiles = f.ntx * f.nty;
    const int lane = threadIdx.x & 63;
    unsigned int *prev_flag = nullptr;
    unsigned int prev_val = 0;
    int prev_n = 0;
    int traced = 0;
    wg_trace(0);
    for (;;) {
        // ONE thread-0 region per iteration (see tflow_kernel)
        if (!BAND && threadIdx.x == 0) {
            if (prev_flag) {
                if (FLOW == 2) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __hip_atomic_store(prev_flag, prev_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            item_sh = atomicAdd(f.head, 1u);
        }
        if (BAND && threadIdx.x < 64) {
            if (prev_n > 0) {
                if (FLOW == 2) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                if (lane < prev_n)
                    __hip_atomic_store(prev_flag + (int64_t)lane * f.ntx, prev_val, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
            if (lane == 0) item_sh = atomicAdd(f.head, 1u);
        }
        __syncthreads();
        const uint32_t item = __builtin_amdgcn_readfirstlane(item_sh);
        if ((int64_t)item >= f.items) return;  // the whole workgroup leaves
        if (LIFE_WG_TRACE && traced < 4) wg_trace(1 + 3 * traced);
        const uint32_t ntx = (uint32_t)f.ntx, nty = (uint32_t)f.nty;
        uint32_t p;
        int64_t tx, ty;
        int nb = 1;
        if (!BAND) {
            p = item / (uint32_t)tiles;
            const uint32_t k = item - p * (uint32_t)tiles, kr = k / ntx;
            tx = k - kr * ntx;
            ty = (kr + p) % nty;
        } else {
            p = item / (uint32_t)f.per_pass;
            const uint32_t k = item - p * (uint32_t)f.per_pass;
            const uint32_t nfull = ntx - 1, G1 = nfull * (uint32_t)f.B + 1u;
            const uint32_t g = k / G1, off = k - g * G1;
            const int64_t ty0 = (int64_t)((g + p) % (uint32_t)f.ngroups) * f.B;
            if (off < nfull * (uint32_t)f.B) {
                tx = off % nfull;
                ty = ty0 + off / nfull;
            } else {
                tx = a.btx1 - 1;
                ty = ty0;
                nb = (int)(f.nty - ty0 < f.B ? f.nty - ty0 : f.B);
            }
            if (ty >= f.nty) {  // a padding item of the last group
                prev_n = 0;
                prev_flag = nullptr;
                __syncthreads();
                continue;
            }
        }
        if (p > 0 && threadIdx.x < 64) {
            bool ok = true;
            const unsigned int *flag = nullptr;
            if (lane < 3 * (nb + 4)) {
                const int64_t dy = lane / 3 - 2, dx = lane % 3 - 1;
                int64_t yy = (ty + dy) % f.nty, xx = (tx + dx) % f.ntx;
                if (yy < 0) yy += f.nty;
                if (xx < 0) xx += f.ntx;
                flag = f.done + yy * f.ntx + xx;
            }
            for (uint32_t spin = 0;; ++spin) {  // bounded, as tflow_kernel's
                if (flag)
                    ok = __hip_atomic_load(const_cast<unsigned int *>(flag), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT) >= p;
                if (__all(ok)) break;
                if (spin == (1u << 20)) {
                    if (lane == 0) atomicMax(f.head + 1, item + 1);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (FLOW == 2) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        if (LIFE_WG_TRACE && traced < 4) wg_trace(2 + 3 * traced);
        const uint8_t *in = (p & 1) ? a.out : a.in;
        uint8_t *out = const_cast<uint8_t *>((p & 1) ? a.in : a.out);
        if (BAND && tx == a.btx1 - 1)
            tile_body_bit<R, WRAPX, WRAPY, FLOW, NW, true>(a, in, out, tx, ty, xch, a.bgsh[0], nb, 0, -1, a.borg[0],
                                                           a.bown[0], rule);
        else
            tile_body_bit<R, WRAPX, WRAPY, FLOW, NW>(a, in, out, tx, ty, xch, 6, 1, 0, -1, 0, 62, rule);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have left
        __syncthreads();
        if (LIFE_WG_TRACE && traced < 4) wg_trace(3 + 3 * traced++);
        prev_flag = f.done + ty * f.ntx + tx;
        prev_val = p + 1;
        prev_n = nb;
    }
}
// the dataflow tiles with B3/S23 in 7 gates per dword (ConwayRule7; LIFE_OPT_RULE7, bit 1)
template <int R, bool WRAPX, bool WRAPY, int FLOW, int NW, bool BAND = false>
__global__ __launch_bounds__(64 * NW, bit_wpe(NW, R)) void tflow7_kernel(FArgs f) {
    __shared__ XchB<NW> xch;
    __shared__ unsigned int item_sh;
    tflow_body<R, WRAPX, WRAPY, FLOW, NW, BAND>(f, xch, item_sh, ConwayRule7{});
}

// Natural 32-cell word j of a bit-encoded row (bit k = cell 32j + k) from
// the pair layout and back: the even / odd halves are 16-bit halves of the
// pair's E / O dwords.  Small-grid kernels work in natural words inside the
// CU and convert once per launch.
__device__ __forceinline__ uint32_t load_nat32(const uint8_t *row, int64_t j) {
    const uint16_t *h = reinterpret_cast<const uint16_t *>(row) + 4 * (j >> 1) + (j & 1);
    return nat32(h[0], h[2]);
}
__device__ __forceinline__ void store_nat32(uint8_t *row, int64_t j, uint32_t x) {
    uint16_t *h = reinterpret_cast<uint16_t *>(row) + 4 * (j >> 1) + (j & 1);
    h[0] = (uint16_t)compact16(x);
    h[2] = (uint16_t)compact16(x >> 1);
}

// ------------------------------------------------------------------ small grids
// LDS-resident stencil for a grid that fits one CU (configs[1]: p46gun_big,
// 500^2): one 1024-thread workgroup imports the shard into LDS as bits
// (W = ceil(w/32) words per row, two h x W buffers), runs G generations with
// one barrier each, and exports the result in the shard's own encoding.  No
// HBM traffic and no launch per generation: the per-generation cost is
// ~1-2k cycles of one CU instead of a full-chip launch.  Both axes wrap
// inside the shard (single-shard grids only); a width that is not a
// multiple of 32 is wrapped by the same patching as WRAPX.
constexpr int kSmallThreads = 1024;

struct SArgs {
    const uint8_t *in;
    uint8_t *out;
    int64_t pitch, xoff, ya;
    int32_t w, h, W, gens, bit;
};

__global__ __launch_bounds__(kSmallThreads) void small_kernel(SArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int W = a.W, h = a.h, w = a.w, n = W * h;
    uint32_t *A = lds, *B = lds + n;
    const int t = threadIdx.x;
    const int q = w - 32 * (W - 1);                   // valid bits in the last word: 1..32
    const uint32_t lastmask = q == 32 ? 0xFFFFFFFFu : ((1u << q) - 1u);
    // import: one word per thread-iteration
    for (int i = t; i < n; i += kSmallThreads) {
        const int y = i / W, j = i % W;
        const uint8_t *row = a.in + (int64_t)(y + a.ya) * a.pitch + a.xoff;
        uint32_t v = 0;
        if (a.bit) {
            v = load_nat32(row, j);
        } else {
            for (int k = 0; k < 32 && 32 * j + k < w; ++k) v |= (uint32_t)(row[32 * j + k] != 0) << k;
        }
        A[i] = j == W - 1 ? v & lastmask : v;
    }
    __syncthreads();
    // thread -> (word column j, rows [y0, y1))
    const int groups = kSmallThreads / W;  // W <= 1024 is checked on the host
    const int j = t % W, g = t / W;
    const int R = (h + groups - 1) / groups;
    const int y0 = g < groups ? g * R : h, y1 = min(h, y0 + R);
    const int jl = j == 0 ? W - 1 : j - 1, jr = j == W - 1 ? 0 : j + 1;
    const uint32_t lshift = j == 0 ? 31u - (uint32_t)((w - 1) & 31) : 0u;  // bit of cell w-1 -> bit 31
    const bool last = j == W - 1;
    for (int gen = 0; gen < a.gens; ++gen) {
        if (y0 < y1) {
            auto hsum = [&](int y, uint32_t &s0, uint32_t &s1, uint32_t &c) {
                y = y < 0 ? y + h : (y >= h ? y - h : y);
                const uint32_t *r = A + y * W;
                c = r[j];
                uint32_t lw = r[jl] << lshift;
                uint32_t rw = r[jr];
                uint32_t cc = c;
                if (last) {  // the cell right of w-1 is cell 0
                    if (q < 32)
                        cc = (cc & lastmask) | ((rw & 1u) << q);
                }
                const uint32_t L = __builtin_amdgcn_alignbit(cc, lw, 31);
                const uint32_t Rr = __builtin_amdgcn_alignbit(rw, cc, 1);
                BitEnc::fa(L, cc, Rr, s0, s1);
            };
            uint32_t p0, p1, c0, c1, n0, n1, cp, cc, cn;
            hsum(y0 - 1, p0, p1, cp);
            hsum(y0, c0, c1, cc);
            for (int y = y0; y < y1; ++y) {
                hsum(y + 1, n0, n1, cn);
                const uint32_t v = BitEnc::rule1(p0, p1, c0, c1, n0, n1, cc);
                B[y * W + j] = last ? v & lastmask : v;
                p0 = c0;
                p1 = c1;
                c0 = n0;
                c1 = n1;
                cc = cn;
            }
        }
        __syncthreads();
        uint32_t *tmp = A;
        A = B;
        B = tmp;
    }
    // export into the shard's encoding (owned cells only)
    for (int i = t; i < n; i += kSmallThreads) {
        const int y = i / W, jj = i % W;
        uint8_t *row = a.out + (int64_t)(y + a.ya) * a.pitch + a.xoff;
        const uint32_t v = A[i];
        if (a.bit) {
            store_nat32(row, jj, v);
        } else {
            for (int k = 0; k < 32 && 32 * jj + k < w; ++k) row[32 * jj + k] = (uint8_t)((v >> k) & 1u);
        }
    }
}

// ------------------------------------------------------- small grids, in VGPRs
// Register-resident variant of the small-grid path (configs[1] p46gun_big
// 500^2).  One 1024-lane workgroup holds the whole grid in VGPRs: a wave is
// split into 64/Wp lane groups (Wp = W rounded up to a power of two), each
// group owns a strip of R consecutive rows, one word column per lane; the
// grid is ns = h/R strips (R divides h, so every strip is full).  Per
// generation a lane computes the 2-bit horizontal sums of its R rows
// (neighbour words by ds_bpermute inside the group, periodic in x),
// publishes the sums of its first and last row in LDS, one barrier, reads the
// strip above's last / the strip below's first sums (periodic in y), and
// applies the rule to its R rows.  PATCH (w % 32 != 0): the x wrap crosses a
// partial word, so cell w-1 is moved to bit 31 of word 0's left word and
// cell 0 is put at bit q of the last word before the sums.
//
// WIN (windowed, several CUs): workgroup b owns rows [b*own, b*own + own) and
// holds the window of ns*R = own + 2K rows starting K rows above them (y
// periodic); the strips at the window's top and bottom take zeros from
// outside, so after m <= K generations rows [K, K + own) of the window are
// exact and only those are stored (in != out; the host runs ceil(gens / K)
// launches, swapping buffers).  ceil(h / own) workgroups instead of one.
constexpr int kRegThreads = 1024;
constexpr int kRegMaxW = 64;

struct RArgs {
    const uint8_t *in;
    uint8_t *out;
    int64_t pitch, xoff, ya;
    int32_t w, h, W, lgWp, gens, bit, ns;
    int32_t own, K;  // WIN: owned rows per workgroup, halo rows above/below
    // WIN, the launches of one call: 1 = the buffer holds natural 32-cell
    // words (bit k = cell 32j + k at row + xoff + 4j) instead of the shard's
    // encoding -- every launch but the first reads them, every launch but the
    // last writes them (no pair (de)interleave or byte (un)packing between
    // launches)
    int32_t nat_in, nat_out;
};

// ROT16 (W == Wp == 16, rows of 481..512 cells, e.g. p46gun_big): a lane
// group is exactly one 16-lane DPP row, so the periodic neighbour words come
// from DPP row rotates on the VALU instead of two ds_bpermute round trips
// through the LDS pipe per row and generation.
template <int R, bool PATCH, bool WIN, bool ROT16 = false>
__global__ __launch_bounds__(kRegThreads) void rsmall_kernel(RArgs a) {
    // [parity][top s0/s1, bottom s0/s1][thread]; WIN: 64 zero slots behind the
    // threads stand for the rows outside the window
    __shared__ uint32_t xch[2][4][kRegThreads + (WIN ? 64 : 0)];
    const int t = threadIdx.x;
    if (WIN && t < 64)
        for (int q = 0; q < 8; ++q) xch[q >> 2][q & 3][kRegThreads + t] = 0u;  // ordered by the first barrier
    const int Wp = 1 << a.lgWp, W = a.W;
    const int j = t & (Wp - 1);  // word column
    const int st = t >> a.lgWp;  // strip
    const bool active = st < a.ns && j < W;
    const int base = (t & 63) & ~(Wp - 1);  // first lane of this lane group
    const int jl = j == 0 ? W - 1 : j - 1, jr = j + 1 >= W ? 0 : j + 1;
    const int addr_l = (base + jl) << 2, addr_r = (base + jr) << 2;
    const int q = a.w - 32 * (W - 1);  // valid cells in the last word: 1..32
    const bool last = j == W - 1;
    const uint32_t keep = (last && q < 32) ? (1u << q) - 1u : 0xFFFFFFFFu;
    const uint32_t lsh = j == 0 ? (uint32_t)((32 - q) & 31) : 0u;  // cell w-1 -> bit 31
    const uint32_t qs = (uint32_t)(q & 31);
    const int sa = st == 0 ? a.ns - 1 : st - 1, sb = st + 1 >= a.ns ? 0 : st + 1;
    int ta = ((sa << a.lgWp) + j) & (kRegThreads - 1), tb = ((sb << a.lgWp) + j) & (kRegThreads - 1);
    if (WIN) {
        if (st == 0) ta = kRegThreads + (j & 63);
        if (st + 1 >= a.ns) tb = kRegThreads + (j & 63);
    }
    const int y0 = st * R;
    // WIN: owned row of window row 0 (may be negative: periodic in y)
    const int64_t wy = WIN ? (int64_t)blockIdx.x * a.own - a.K : 0;

    uint32_t v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t x = 0;
        if (active) {
            int64_t gy = y0 + r;
            if (WIN) {
                gy = (wy + gy) % a.h;
                if (gy < 0) gy += a.h;
            }
            const uint8_t *row = a.in + (gy + a.ya) * a.pitch + a.xoff;
            if (WIN && a.nat_in) {
                x = reinterpret_cast<const uint32_t *>(row)[j];
            } else if (a.bit) {
                x = load_nat32(row, j);
            } else {
                for (int k = 0; k < 32 && 32 * j + k < a.w; ++k) x |= (uint32_t)(row[32 * j + k] != 0) << k;
            }
        }
        v[r] = x;
    }
    auto hsum = [&](uint32_t c, uint32_t &s0, uint32_t &s1) {
        uint32_t l;
        uint32_t rw;
        if (ROT16) {
            l = (uint32_t)__builtin_amdgcn_mov_dpp((int)c, 0x121, 0xf, 0xf, false);   // row_ror:1 -> lane j-1
            rw = (uint32_t)__builtin_amdgcn_mov_dpp((int)c, 0x12F, 0xf, 0xf, false);  // row_ror:15 -> lane j+1
        } else {
            l = bperm(addr_l, c);
            rw = bperm(addr_r, c);
        }
        if (PATCH) {
            l <<= lsh;
            // (c & keep) | (rw << qs & ~keep): the last word gets cell 0 at bit q (above it: don't-care)
            c = b3<((0xF0 & 0xCC) | (~0xCC & 0xAA)) & 0xFF>(c, keep, rw << qs);
        }
        BitEnc::fa(__builtin_amdgcn_alignbit(c, l, 31), c, __builtin_amdgcn_alignbit(rw, c, 1), s0, s1);
    };
    for (int g = 0; g < a.gens; ++g) {
        const int par = g & 1;
        uint32_t h0[R], h1[R];
        hsum(v[0], h0[0], h1[0]);
        if (R > 1) hsum(v[R - 1], h0[R - 1], h1[R - 1]);
        xch[par][0][t] = h0[0];
        xch[par][1][t] = h1[0];
        xch[par][2][t] = h0[R - 1];
        xch[par][3][t] = h1[R - 1];
        __syncthreads();
        const uint32_t a0 = xch[par][2][ta], a1 = xch[par][3][ta];
        const uint32_t d0 = xch[par][0][tb], d1 = xch[par][1][tb];
#pragma unroll
        for (int r = 1; r < R - 1; ++r) hsum(v[r], h0[r], h1[r]);
#pragma unroll
        for (int r = 1; r < R - 1; ++r)
            v[r] = BitEnc::rule1(h0[r - 1], h1[r - 1], h0[r], h1[r], h0[r + 1], h1[r + 1], v[r]);
        if (R == 1) {
            v[0] = BitEnc::rule1(a0, a1, h0[0], h1[0], d0, d1, v[0]);
        } else {
            v[0] = BitEnc::rule1(a0, a1, h0[0], h1[0], h0[1], h1[1], v[0]);
            v[R - 1] = BitEnc::rule1(h0[R - 2], h1[R - 2], h0[R - 1], h1[R - 1], d0, d1, v[R - 1]);
        }
    }
    if (!active) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int64_t gy = y0 + r;
        if (WIN) {
            // window rows [K, K + own) that exist
            if (gy < a.K || gy >= a.K + a.own || wy + gy >= a.h) continue;
            gy += wy;
        }
        uint8_t *row = a.out + (gy + a.ya) * a.pitch + a.xoff;
        const uint32_t x = v[r] & keep;
        if (WIN && a.nat_out) {
            reinterpret_cast<uint32_t *>(row)[j] = x;
        } else if (a.bit) {
            store_nat32(row, j, x);
        } else {
            for (int k = 0; k < 32 && 32 * j + k < a.w; ++k) row[32 * j + k] = (uint8_t)((x >> k) & 1u);
        }
    }
}

// Strip heights with a kernel instance: the smallest that divides h and
// gives at most kRegThreads / Wp strips is used.
constexpr int kRegRows[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 25, 32};

template <bool PATCH, bool WIN>
hipError_t launch_rs(const RArgs &a, int R, unsigned blocks, hipStream_t s) {
    // only the waves that own strips (the barrier counts the launched waves)
    const unsigned threads = (unsigned)((((int64_t)a.ns << a.lgWp) + 63) / 64 * 64);
    if (WIN && R == 1 && a.W == 16 && a.lgWp == 4) {  // the automatic window shape, 16-word rows
        rsmall_kernel<1, PATCH, WIN, true><<<blocks, threads, 0, s>>>(a);
        return hipGetLastError();
    }
    switch (R) {
#define LIFE_RS(N) \
    case N: rsmall_kernel<N, PATCH, WIN><<<blocks, threads, 0, s>>>(a); break;
        LIFE_RS(1) LIFE_RS(2) LIFE_RS(3) LIFE_RS(4) LIFE_RS(5) LIFE_RS(6) LIFE_RS(8) LIFE_RS(10) LIFE_RS(12)
        LIFE_RS(16) LIFE_RS(20) LIFE_RS(25) LIFE_RS(32)
#undef LIFE_RS
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

inline bool is_bit(const life_layout &L) { return L.kernel == LIFE_KERNEL_BIT; }

}  // namespace

namespace {
// Measured on MI355X at 65536^2 (scripts/tune.py, profiles/): byte R16/D8 the
// fastest of {16,32,64} x {2,4,8} once the strips are dealt to the XCDs in
// row-major runs (1.497 ms against 1.647 for the former R64/D2,
// profiles/r03/r5j tune_byte1.log); bit R16 with the whole strip in flight
// (D18) 1.7 % ahead of D8 (profiles/r03/r5b tune_bit1.log).
struct Tunings {
    StepTuning t[2] = {{env::read(env::kStepRows), env::read(env::kStepDepth, 8)},    // [0] byte
                       {env::read(env::kStepRows), env::read(env::kStepDepth, 18)}};  // [1] bit
    // temporal tiles: register rows per wave, per encoding [byte (32-cell
    // words), bit (64-cell pairs)]; a tile workgroup is kStackWaves waves
    // (window = waves x rows, tile = window - 2 ghost rows per end)
    int nr[2] = {env::read(env::kTemporalRowsByte), env::read(env::kTemporalRows)};
};
Tunings &tunings() {
    static Tunings t;
    return t;
}
// Tile heights with a kernel instance.  Round 5 kept the shipped shapes and
// one alternative each: every other shape measured slower at 65536^2
// (profiles/r02/r2w, r03/r4g) and at 32768^2 (bit 32x8, 24x12, 16x16:
// 0.96-0.99 of 24x8, profiles/r05/a).
// (byte 64-row tiles, round 5: 61.3 vs 60.5 T at 65536^2, 48.1 vs 50.0 T at
// 32768^2 -- flat, removed; profiles/r05/g)
bool temporal_rows_ok(bool bit, int nr) { return bit ? (nr == 16 || nr == 24) : (nr == 32 || nr == 48); }
}  // namespace

StepTuning step_tuning(bool bit) { return tunings().t[bit ? 1 : 0]; }

int temporal_rows(bool bit) {
    const int nr = tunings().nr[bit ? 1 : 0];
    return temporal_rows_ok(bit, nr) ? nr : bit ? 24 : 48;
}

// 8 for both encodings: the bit tiles have instances for NW == 8 only
// (LIFE_BIT_SHAPES; 24x12 and 16x16 ran 0.96-0.99 of 24x8, profiles/r05/a)
int tile_waves(bool) { return kStackWaves; }

// VALU instructions per lane position of a tile for m generations.  Bit, per
// pair row and generation: 2 v_alignbit + 2 full adders (4 v_bitop3) + the
// rule for both dwords (16 v_bitop3) = 22 (+ 2 ds_bpermute on the LDS pipe);
// byte, per word row: the drifting frame (12) plus pack (8 v_dot4 + 3
// shifts) and unpack (8 x bfe/mul24/and) once per row and launch.
// Census instances (pop): kPopValuPerPairRow more per pair row and generation
// (the two v_bcnt; the wave's reduction and the ownership test are per
// generation, not per row, and not modelled).
// The 7-gate arm (LIFE_OPT_RULE7: 20 per pair row) is priced at the same 22:
// the model counts the work of the 8-gate formulation for both arms, so the
// booked lane-ops and the roofline fractions built on them are "22-op
// equivalents" that compare across the arms (a faster arm shows a higher
// fraction); what really issues is pinned by tests/test_isa_rule7.py.
double tstep_valu_per_tile_lane(int m, bool byte, bool rule, bool pop) {
    if (byte) return (double)kStackWaves * (double)temporal_rows(false) * (12.0 * (double)m + 35.0);
    return (double)tile_waves(true) * (double)temporal_rows(true) *
           ((rule ? (double)kRuleValuPerPairRow : 22.0) + (pop ? (double)kPopValuPerPairRow : 0.0)) * (double)m;
}

void set_temporal_rows(int kernel, int nr) {
    for (int k = 0; k < 2; k++)
        if ((kernel < 0 || kernel == k) && temporal_rows_ok(k == 1, nr)) tunings().nr[k] = nr;
}

void set_step_tuning(int kernel, int rows, int depth) {
    for (int k = 0; k < 2; k++) {
        if (kernel >= 0 && kernel != k) continue;
        if (rows == 16 || rows == 32 || rows == 64) tunings().t[k].rows = rows;
        if (depth == 2 || depth == 4 || depth == 8 || depth == 18) tunings().t[k].depth = depth;
    }
}

namespace {
template <class E, int R, int D>
hipError_t launch_rd(const StepArgs &a, bool wrapx, unsigned grid, hipStream_t s) {
    if (wrapx)
        step_kernel<E, R, D, true><<<grid, kBlock, 0, s>>>(a);
    else
        step_kernel<E, R, D, false><<<grid, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

template <class E, int R>
hipError_t launch_r(const StepArgs &a, int depth, bool wrapx, unsigned grid, hipStream_t s) {
    switch (depth) {
    case 2: return launch_rd<E, R, 2>(a, wrapx, grid, s);
    case 8: return launch_rd<E, R, 8>(a, wrapx, grid, s);
    case 18:  // R = 16 only: the lane's whole strip (16 + 2 rows) loaded before any row is computed
        if constexpr (R == 16) return launch_rd<E, 16, 18>(a, wrapx, grid, s);
        return launch_rd<E, R, 4>(a, wrapx, grid, s);
    default: return launch_rd<E, R, 4>(a, wrapx, grid, s);
    }
}

template <class E>
hipError_t launch_e(const StepArgs &a, const StepTuning &t, bool wrapx, unsigned grid, hipStream_t s) {
    switch (t.rows) {
    case 16: return launch_r<E, 16>(a, t.depth, wrapx, grid, s);
    case 64: return launch_r<E, 64>(a, t.depth, wrapx, grid, s);
    default: return launch_r<E, 32>(a, t.depth, wrapx, grid, s);
    }
}
}  // namespace

// Per-XCD runs of one-generation strips (StepArgs::xcd).  Measured at
// 65536^2 (profiles/r03/r5f): byte 1.872 -> 1.730 ms (0.73 -> 0.79 of the copy
// ceiling), bit 0.1998 -> 0.2012 ms (within noise, off): on for the byte
// encoding.  LIFE_XCD_ORDER_ONEGEN=0/1 forces it for both.
static bool onegen_xcd_enabled(bool bit) {
    static const int v = env::read(env::kXcdOrderOnegen);
    return v >= 0 ? v == 1 : !bit;
}

hipError_t launch_step(const life_layout &L, const uint8_t *in, uint8_t *out, uint8_t *sink,
                       const Region &reg, Wrap wrap, hipStream_t s, const RuleWords *rule) {
    if (reg.u1 <= reg.u0 || reg.r1 <= reg.r0) return hipSuccess;
    if (rule && !is_bit(L)) return hipErrorInvalidValue;  // no quiet B3/S23 in its place
    StepTuning t = step_tuning(is_bit(L));
    if (t.rows != 16 && t.rows != 64) t.rows = 32;
    if (rule) t.rows = kRuleStepRows;
    StepArgs a;
    a.in = in;
    a.out = out;
    a.sink = sink;
    a.pitch = L.pitch;
    a.xoff = L.xoff;
    a.units = L.units;
    a.w = L.w;
    a.h = L.h;
    a.ya = L.yapron;
    a.u0 = reg.u0;
    a.u1 = reg.u1;
    a.r0 = reg.r0;
    a.r1 = reg.r1;
    a.nbx = (reg.u1 - reg.u0 + kBlock - 1) / kBlock;
    a.wrapy = wrap.y ? 1 : 0;
    a.xcd = onegen_xcd_enabled(is_bit(L)) ? 1 : 0;
    const int64_t nby = (reg.r1 - reg.r0 + t.rows - 1) / t.rows;
    const unsigned grid = (unsigned)(a.nbx * nby);
    if (rule) {
        const RStepArgs ra{a, *rule};
        if (wrap.x)
            rule_step_kernel<true><<<grid, kBlock, 0, s>>>(ra);
        else
            rule_step_kernel<false><<<grid, kBlock, 0, s>>>(ra);
        return hipGetLastError();
    }
    return is_bit(L) ? launch_e<BitEnc>(a, t, wrap.x, grid, s) : launch_e<ByteEnc>(a, t, wrap.x, grid, s);
}

namespace {
// One launch; with events (timing on) through hipExtLaunchKernel, which
// stamps them with the dispatch's own start and end: no event packets
// between back-to-back launches (each cost a ~5 us bubble and ~6 us of host
// time before the first launch, profiles/r03/r4d trace).
hipError_t launch_fn(const void *fn, unsigned grid, unsigned threads, void *arg, hipStream_t s, hipEvent_t ev0,
                     hipEvent_t ev1) {
    void *args[] = {arg};
    if (ev0 || ev1) return hipExtLaunchKernel(fn, dim3(grid), dim3(threads), args, 0, s, ev0, ev1, 0);
    return hipLaunchKernel(fn, dim3(grid), dim3(threads), args, 0, s);
}

template <int R, int GK>
const void *byte_fn(Wrap wrap) {
    constexpr int NW = kStackWaves;
    if (wrap.x && wrap.y) return (const void *)tstep_byte_kernel<R, GK, true, true, NW>;
    if (wrap.x) return (const void *)tstep_byte_kernel<R, GK, true, false, NW>;
    if (wrap.y) return (const void *)tstep_byte_kernel<R, GK, false, true, NW>;
    return (const void *)tstep_byte_kernel<R, GK, false, false, NW>;
}

template <int GK>
const void *byte_k(Wrap wrap) {
    switch (temporal_rows(false)) {
    case 32: return byte_fn<32, GK>(wrap);
    default: return byte_fn<48, GK>(wrap);
    }
}

template <int R, int NW>
const void *bit_fn(Wrap wrap, bool rule7) {
    if (rule7) {  // the 7-gate arm (tstep_bit7_kernel)
        if (wrap.x && wrap.y) return (const void *)tstep_bit7_kernel<R, true, true, NW>;
        if (wrap.x) return (const void *)tstep_bit7_kernel<R, true, false, NW>;
        if (wrap.y) return (const void *)tstep_bit7_kernel<R, false, true, NW>;
        return (const void *)tstep_bit7_kernel<R, false, false, NW>;
    }
    if (wrap.x && wrap.y) return (const void *)tstep_bit_kernel<R, true, true, NW>;
    if (wrap.x) return (const void *)tstep_bit_kernel<R, true, false, NW>;
    if (wrap.y) return (const void *)tstep_bit_kernel<R, false, true, NW>;
    return (const void *)tstep_bit_kernel<R, false, false, NW>;
}

// the bit tile shape's instances: per-launch tiles and the occupancy probe
#define LIFE_BIT_SHAPES(X) X(24, 8) X(16, 8)
const void *bit_k(Wrap wrap, bool rule7) {
    const int R = temporal_rows(true), NW = tile_waves(true);
#define LIFE_BIT_CASE(r, nw) \
    if (R == r && NW == nw) return bit_fn<r, nw>(wrap, rule7);
    LIFE_BIT_SHAPES(LIFE_BIT_CASE)
#undef LIFE_BIT_CASE
    return nullptr;
}
const void *tstep_bit_fn(bool rule7) { return bit_k(Wrap{true, true}, rule7); }

// the same shapes under a table rule (trule_bit_kernel)
template <int R, int NW>
const void *rule_fn(Wrap wrap) {
    if (wrap.x && wrap.y) return (const void *)trule_bit_kernel<R, true, true, NW>;
    if (wrap.x) return (const void *)trule_bit_kernel<R, true, false, NW>;
    if (wrap.y) return (const void *)trule_bit_kernel<R, false, true, NW>;
    return (const void *)trule_bit_kernel<R, false, false, NW>;
}
const void *rule_k(Wrap wrap) {
    const int R = temporal_rows(true), NW = tile_waves(true);
#define LIFE_BIT_CASE(r, nw) \
    if (R == r && NW == nw) return rule_fn<r, nw>(wrap);
    LIFE_BIT_SHAPES(LIFE_BIT_CASE)
#undef LIFE_BIT_CASE
    return nullptr;
}

// the census instances of both (tpop_bit_kernel / tpop_rule_kernel)
template <int R, int NW>
const void *pop_fn(Wrap wrap, bool rule) {
    if (rule) {
        if (wrap.x && wrap.y) return (const void *)tpop_rule_kernel<R, true, true, NW>;
        if (wrap.x) return (const void *)tpop_rule_kernel<R, true, false, NW>;
        if (wrap.y) return (const void *)tpop_rule_kernel<R, false, true, NW>;
        return (const void *)tpop_rule_kernel<R, false, false, NW>;
    }
    if (wrap.x && wrap.y) return (const void *)tpop_bit_kernel<R, true, true, NW>;
    if (wrap.x) return (const void *)tpop_bit_kernel<R, true, false, NW>;
    if (wrap.y) return (const void *)tpop_bit_kernel<R, false, true, NW>;
    return (const void *)tpop_bit_kernel<R, false, false, NW>;
}
const void *pop_k(Wrap wrap, bool rule) {
    const int R = temporal_rows(true), NW = tile_waves(true);
#define LIFE_BIT_CASE(r, nw) \
    if (R == r && NW == nw) return pop_fn<r, nw>(wrap, rule);
    LIFE_BIT_SHAPES(LIFE_BIT_CASE)
#undef LIFE_BIT_CASE
    return nullptr;
}
}  // namespace

// Byte tiles are compiled for a fixed ghost depth (a runtime depth measured
// 29 % slower, profiles/r02/ghost_ab.txt): K (16 / 32), and 1 for the
// one-generation launches of step(1) calls at the default tile height (a
// 384-row window then re-reads 2 rows instead of 64)
// (LIFE_BYTE_ONE_GHOST=0: K ghost rows for them too; A/B knob)
static bool byte_one_ghost(const life_layout &L, int m) {
    static const bool on = env::read(env::kByteOneGhost) != 0;
    return on && !is_bit(L) && m == 1 && temporal_rows(false) == 48;
}
int tile_ghost(const life_layout &L, int m) {
    return is_bit(L) ? m : byte_one_ghost(L, m) ? 1 : L.generations_per_exchange;
}

// LIFE_BANDS=0: no banded tile column (A/B knob)
static bool bands_enabled() { static const bool on = env::read(env::kBands) != 0; return on; }

// LIFE_BAND_SPLIT=0: at most one sub-column, the rule before the split (A/B knob)
static bool band_split_enabled() { static const bool on = env::read(env::kBandSplit) != 0; return on; }

TileGeom tile_geom(const life_layout &L, int m, bool one_band) {
    TileGeom g;
    const bool bit = is_bit(L);
    g.lanes = 62;
    g.cells = bit ? 64 : 32;
    g.rows = (int64_t)tile_waves(bit) * temporal_rows(bit) - 2 * (int64_t)tile_ghost(L, m);
    const int64_t W = (L.w + g.cells - 1) / g.cells;  // lane columns (pairs / words) per row
    g.ntx = (W + g.lanes - 1) / g.lanes;
    g.nty = (L.h + g.rows - 1) / g.rows;
    // the last tile column owns o lane columns, run as the sub-columns of
    // life::band_split (65536^2: 1024 pairs, o = 32, {30, G 32} + {2, G 4};
    // 32768^2: o = 16, {14, G 16} + {2, G 4}).  One band: G >= o + 2 lanes
    // when G <= 32 (o = 32: a whole tile, o = 16: G = 32)
    const int64_t o = W - g.lanes * (g.ntx - 1);
    const bool split = !one_band && band_split_enabled();
    const BandSplit sp = bit && bands_enabled() ? band_split(o, split ? kMaxBands : 1) : BandSplit{};
    g.nband = sp.n;
    for (int i = 0; i < kMaxBands; i++) g.band[i] = sp.b[i];
    g.bcol = g.nband > 0 ? g.ntx - 1 : -1;
    return g;
}

// LIFE_XCD_ORDER=0: dispatch-order bit tiles instead of per-XCD row-major
// runs (TArgs::xcd_n).  Measured at the driver's 65536^2 call (profiles/r03/
// r5a): FETCH_SIZE x2 0.758 -> 0.572 GB per launch, WRITE_SIZE 0.554 -> 0.539
// GB (1.22x -> 1.035x compulsory), time within the run-to-run spread (+1 %)
static bool xcd_order_enabled() { static const bool on = env::read(env::kXcdOrder) != 0; return on; }
// LIFE_XCD_ORDER_BYTE=0: dispatch order for the byte tiles.  The per-XCD
// order measured (profiles/r03/r5b, 65536^2): 64.4-65.7 -> 66.9-67.0 T,
// FETCH_SIZE x2 5.81 -> 5.41 GB per 32-generation launch, WRITE unchanged.
// Walking each XCD's run in strips of 4 / 8 / 16 tile columns instead (so the
// tile below, sharing 64 ghost rows, is in flight beside each tile) fetched
// 1-3 % less and ran 12 / 5 / 0 % slower (r5l): a 768 KB window per tile
// leaves no L2 reuse to find
static bool xcd_order_byte_enabled() { static const bool on = env::read(env::kXcdOrderByte) != 0; return on; }

// LIFE_TAIL_SPLIT: 0 no half-height tail tiles, 1 the round-4 rule (the
// fewest bottom tile rows whose half tiles fill one round, when the last
// round is under half full), 2 (default) the split a list-scheduling model
// of the launch says ends first (life::tail_plan, life_plan.cpp).  (Round 6
// measured a third tier, 3/4-height tiles, chosen by the same model: 5-7 %
// slower at the small blocks, profiles/r06/c -- removed.)
static int tail_split_mode() { static const int v = env::read(env::kTailSplit); return v; }
// the fixed share of a tile's duration (window load, stores, workgroup
// turnover) in the tail model's item durations (life::tail_plan)
constexpr double kTailC = 0.06;
// resident workgroups of a kernel on this device (occupancy)
static int slots_of(const void *fn, int threads) {
    int dev = 0, cus = 0, per = 0;
    if (!fn || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, threads, 0) != hipSuccess)
        return 0;
    return cus * per;
}
// the bit tiles of the current shape, of either arm (cached per shape and arm)
static int tstep_bit_slots(bool rule7) {
    static int cached[2] = {0, 0}, key[2] = {-1, -1};
    const int k = temporal_rows(true) * 64 + tile_waves(true);
    if (k != key[rule7]) {
        cached[rule7] = slots_of(tstep_bit_fn(rule7), 64 * tile_waves(true));
        key[rule7] = k;
    }
    return cached[rule7];
}
// the table-rule tiles of the current shape: 2 per CU, not 3
static int trule_bit_slots() {
    static int cached = 0, key = -1;
    const int k = temporal_rows(true) * 64 + tile_waves(true);
    if (k != key) {
        cached = slots_of(rule_k(Wrap{true, true}), 64 * tile_waves(true));
        key = k;
    }
    return cached;
}

int tile_slots(const life_layout &L, bool rule, bool rule7) {
    if (is_bit(L)) return rule ? trule_bit_slots() : tstep_bit_slots(rule7);
    static int cached = 0, key = -1;
    const int k = temporal_rows(false);
    if (k != key) {
        cached = slots_of(byte_k<32>(Wrap{true, true}), 64 * kStackWaves);
        key = k;
    }
    return cached;
}

int64_t region_items(const TileGeom &g, const TileRegion &r) {
    if (r.tx1 <= r.tx0 || r.ty1 <= r.ty0) return 0;
    const BandRows b = region_bands(g, r.tx1);
    return tail_row_items(r.tx1 - r.tx0 - (b.n > 0 ? 1 : 0), b, r.ty1 - r.ty0);
}

BandRows region_bands(const TileGeom &g, int64_t tx1) {
    BandRows b;
    if (g.nband > 0 && tx1 == g.bcol + 1)
        for (b.n = 0; b.n < g.nband; b.n++) b.B[b.n] = 64 >> g.band[b.n].gsh;
    return b;
}

life_layout extended_layout(const life_layout &L, const Extend &ext) {
    life_layout V = L;
    V.h += 2 * ext.y;
    V.yapron -= ext.y;
    V.rows = V.h + 2 * V.yapron;
    return V;
}

// The tail plan of a bit launch over tile columns [tx0, tx1) x rows [ty0,
// ty1) of tile_geom(L, m), beside `pre` items of another launch dispatched
// just before it (launch_tstep; cached by life::tail_plan).
static TailPlan tail_plan_for(const life_layout &L, const TileGeom &g, int m, int64_t tx0, int64_t tx1, int64_t ty0,
                              int64_t ty1, int64_t pre, bool rule, bool rule7) {
    const int64_t T2 = (int64_t)tile_waves(true) * (temporal_rows(true) / 2) - 2 * (int64_t)tile_ghost(L, m);
    const int64_t yend = std::min(ty1 * g.rows, L.h);
    const BandRows b = region_bands(g, tx1);
    return tail_plan(tx1 - tx0 - (b.n > 0 ? 1 : 0), b, ty0, ty1, yend, g.rows, T2,
                     rule ? trule_bit_slots() : tstep_bit_slots(rule7), tail_split_mode(), kTailC, pre);
}

void prewarm_tail_plans(const life_layout &L, int mmax, bool ext_y, bool rule, bool rule7) {
    if (!is_bit(L) || L.generations_per_exchange < 2 || tail_split_mode() == 0) return;
    const int K = L.generations_per_exchange;
    for (int m = 1; m <= std::min(mmax, K); ++m)
        for (int e = 0; e <= (ext_y ? K - m : 0); ++e) {
            Extend x;
            x.y = e;
            const life_layout V = extended_layout(L, x);
            const TileGeom g = tile_geom(V, m);
            if (g.rows >= 1) (void)tail_plan_for(V, g, m, 0, g.ntx, 0, g.nty, 0, rule, rule7);
        }
}

// the banded column of g as the kernels take it (none: nband = 0)
static void set_bands(TArgs &a, const TileGeom &g) {
    a.nband = (int32_t)g.nband;
    a.btx1 = g.bcol + 1;
    for (int i = 0; i < kMaxBands; i++) {
        const bool on = i < g.nband;
        a.bgsh[i] = on ? g.band[i].gsh : 6;
        a.bown[i] = on ? g.band[i].own : 0;
        a.borg[i] = on ? g.bcol * g.lanes + g.band[i].first : 0;
    }
}

// The 32-bit range tile_body_bit works in: pair columns up to W + 62 and
// rows up to h + 17 T + NW R (a banded lane of the last item) below 2^31.
static bool tile_body_fits32(const TArgs &a, int window_rows, int64_t nty) {
    const int64_t lim = (int64_t)1 << 31, T = window_rows - 2 * (int64_t)a.m;
    return a.W + 64 < lim && a.h + 66 * (int64_t)window_rows < lim && (nty + 17) * T + window_rows < lim &&
           a.xoff + 8 * (a.W + 64) < 2 * lim;
}
// The item decode's constants of a bit launch (TArgs::d) from its regions,
// bands, tail and XCD order; false: a count beyond the 32 bits the kernels
// work in (no grid that fits in HBM comes near), the launch fails.
static bool tile_args_seal(TArgs &a, int window_rows, int ghost, bool bit) {
    life_tile_launch l = {};
    l.nreg = a.nreg;
    l.nband = bit ? a.nband : 0;  // (the byte tiles have no banded column)
    l.m = ghost;                  // ghost rows at each end of a window: m (bit), the apron depth or 1 (byte)
    l.window_rows = window_rows;
    int64_t nty = 0;
    for (int k = 0; k < a.nreg; k++) {
        l.tx0[k] = a.tx0[k];
        l.tx1[k] = a.tx1[k];
        l.ty0[k] = a.ty0[k];
        l.ty1[k] = a.ty1[k];
        l.first[k] = a.first[k];
        nty = std::max(nty, a.ty1[k]);
    }
    l.first[a.nreg] = a.first[a.nreg];
    for (int i = 0; i < kMaxBands; i++) l.bgsh[i] = a.bgsh[i];
    l.btx1 = a.btx1;
    l.tail_first = a.tail_first;
    l.tail_y = a.tail_y;
    l.tail_yend = a.tail_yend;
    l.tail_ntx = a.tail_ntx;
    l.tail_tx0 = a.tail_tx0;
    l.xcd_n = a.xcd_n;
    return (!bit || tile_body_fits32(a, window_rows, nty)) && tile_decode_fill(l, &a.d);
}

hipError_t launch_tstep(const life_layout &Lin, const uint8_t *in, uint8_t *out, const TileRegion *r, int nreg,
                        int m, Wrap wrap, hipStream_t s, double *valu_lane_ops, hipEvent_t ev0, hipEvent_t ev1,
                        Extend ext, int64_t concurrent, const RuleWords *rule, unsigned long long *pop, bool rule7) {
    const int K = Lin.generations_per_exchange;
    const bool bit = is_bit(Lin);
    if (rule && !bit) return hipErrorInvalidValue;  // no quiet B3/S23 in its place
    if (pop && (!bit || Lin.w % 64 != 0 || m > kPopGens)) return hipErrorInvalidValue;  // whole pairs (PopArgs)
    // m <= 32: the tile's edge lanes absorb at most 32 wrong cells; m <= the
    // apron depth a partitioned axis provides.  Deep-halo passes: bit only
    // (the byte windows hold K ghost rows whatever m is), the window's top
    // ghost rows inside the apron (y + m <= yapron), no wrapped axis extended.
    if (nreg < 0 || nreg > kMaxRegions || m > K || m > 32 || K < 2 || Lin.yapron != K || ext.y < 0 ||
        ((ext.y > 0 || ext.x) && (!bit || ext.y + m > K || (ext.y > 0 && wrap.y) || (ext.x && wrap.x))) ||
        tile_waves(bit) * temporal_rows(bit) - 2 * tile_ghost(Lin, m) < 1 || (!bit && K != 16 && K != 32))
        return hipErrorInvalidValue;
    const life_layout L = extended_layout(Lin, ext);
    const TileGeom g = tile_geom(L, m);
    TArgs a;
    a.in = in;
    a.out = out;
    a.pitch = L.pitch;
    a.xoff = L.xoff;
    a.W = (L.w + g.cells - 1) / g.cells;  // the last lane column may be partial: its upper cells are the right apron
    a.h = L.h;
    a.ya = L.yapron;
    a.m = m;
    a.xext = ext.x ? 1 : 0;
    a.nreg = 0;
    a.first[0] = 0;
    set_bands(a, g);
    for (int k = 0; k < nreg; k++) {
        if (r[k].tx1 <= r[k].tx0 || r[k].ty1 <= r[k].ty0) continue;
        const int n = a.nreg++;
        a.tx0[n] = r[k].tx0;
        a.tx1[n] = r[k].tx1;
        a.ty0[n] = r[k].ty0;
        a.ty1[n] = r[k].ty1;
        a.first[n + 1] = a.first[n] + region_items(g, r[k]);
    }
    if (a.nreg == 0 || m <= 0) return hipSuccess;
    int64_t items = a.first[a.nreg];  // one workgroup per tile (or banded item)
    a.tail_first = a.tail_y = a.tail_yend = a.tail_ntx = a.tail_tx0 = 0;
    const int64_t T2 = (int64_t)tile_waves(bit) * (temporal_rows(bit) / 2) - 2 * (int64_t)tile_ghost(L, m);
    if (bit && T2 >= 1 && a.nreg == 1 && tail_split_mode() > 0 && concurrent >= 0) {
        // One region: the whole shard, a deep-halo pass over the extended
        // shard, a row strip's interior, or (round 6) the interior of an
        // exchange pass beside its ring (`concurrent` = the ring's items,
        // dispatched just before it on another stream).  The launch runs
        // items / slots rounds of equal tiles; a last round under full leaves
        // CUs idle for up to a whole tile time.  The bottom tile rows are
        // re-tiled as half-height tiles (banded in the last column like the
        // full tiles, round 6), dispatched last, so the final round is
        // half-length items on every slot (life::tail_plan).  The byte tiles
        // (2 per CU, 32 ghost rows: a third of a half tile) lost 3-4 % with
        // half tiles (profiles/r02/r2z) and keep whole tiles.
        const int64_t tx0 = a.tx0[0], tx1 = a.tx1[0], ty0 = a.ty0[0], ty1 = a.ty1[0];
        const int64_t yend = std::min(ty1 * g.rows, L.h);
        const BandRows bands = region_bands(g, tx1);
        const TailPlan p = tail_plan_for(L, g, m, tx0, tx1, ty0, ty1, concurrent, rule != nullptr, rule7);
        if (p.F < ty1 && p.F >= ty0) {
            a.ty1[0] = p.F;
            a.first[1] = region_items(g, TileRegion{tx0, tx1, ty0, p.F});
            a.tail_first = a.first[1];
            a.tail_y = p.F * g.rows;
            a.tail_yend = yend;
            a.tail_ntx = tx1 - tx0;
            a.tail_tx0 = tx0;
            items = a.tail_first + tail_row_items(tx1 - tx0 - (bands.n > 0 ? 1 : 0), bands, p.n2);
        }
    }
    const bool split = a.tail_ntx > 0;
    a.xcd_n = (bit ? xcd_order_enabled() : xcd_order_byte_enabled()) ? (split ? a.tail_first : items) : 0;
    if (!tile_args_seal(a, tile_waves(bit) * temporal_rows(bit), tile_ghost(L, m), bit)) return hipErrorInvalidValue;
    if (valu_lane_ops) {
        const double lane = 64.0 * tstep_valu_per_tile_lane(m, !bit, rule != nullptr, pop != nullptr);
        *valu_lane_ops = (double)(split ? a.tail_first : items) * lane;
        if (split)  // half tiles: R / 2 register rows per wave
            *valu_lane_ops += (double)(items - a.tail_first) * lane * 0.5;
    }
    if (pop) {
        // the counted rows: the shard's own, not the apron rows a deep-halo pass advances
        const PopArgs pa{pop, ext.y, ext.y + Lin.h};
        const void *pfn = pop_k(wrap, rule != nullptr);
        if (!pfn) return hipErrorInvalidValue;
        if (rule) {
            RPTArgs ra{a, *rule, pa};
            return launch_fn(pfn, (unsigned)items, 64u * (unsigned)tile_waves(true), &ra, s, ev0, ev1);
        }
        PTArgs ta{a, pa};
        return launch_fn(pfn, (unsigned)items, 64u * (unsigned)tile_waves(true), &ta, s, ev0, ev1);
    }
    if (rule) {
        const void *rfn = rule_k(wrap);
        if (!rfn) return hipErrorInvalidValue;
        RTArgs ra{a, *rule};
        return launch_fn(rfn, (unsigned)items, 64u * (unsigned)tile_waves(true), &ra, s, ev0, ev1);
    }
    // (B3/S23 without a census, here: the only tiles with a 7-gate arm)
    const void *fn = bit                      ? bit_k(wrap, rule7)
                     : byte_one_ghost(L, m) ? byte_fn<48, 1>(wrap)
                     : K == 16              ? byte_k<16>(wrap)
                                            : byte_k<32>(wrap);
    if (!fn) return hipErrorInvalidValue;
    return launch_fn(fn, (unsigned)items, 64u * (unsigned)tile_waves(bit), &a, s, ev0, ev1);
}

namespace {
const void *skip_k(bool rule) {
    const int R = temporal_rows(true), NW = tile_waves(true);
#define LIFE_BIT_CASE(r, nw) \
    if (R == r && NW == nw) return rule ? (const void *)tskip_rule_kernel<r, nw> : (const void *)tskip_bit_kernel<r, nw>;
    LIFE_BIT_SHAPES(LIFE_BIT_CASE)
#undef LIFE_BIT_CASE
    return nullptr;
}
const void *skip_pop_k(bool rule) {
    const int R = temporal_rows(true), NW = tile_waves(true);
#define LIFE_BIT_CASE(r, nw)  \
    if (R == r && NW == nw) \
        return rule ? (const void *)tpop_skip_rule_kernel<r, nw> : (const void *)tpop_skip_kernel<r, nw>;
    LIFE_BIT_SHAPES(LIFE_BIT_CASE)
#undef LIFE_BIT_CASE
    return nullptr;
}
}  // namespace

hipError_t launch_pop_fold(unsigned long long *cnt, unsigned long long *trace, int m, hipStream_t s) {
    if (m < 0 || m > kPopGens) return hipErrorInvalidValue;
    pop_fold_kernel<<<kPopGens, 64, 0, s>>>(cnt, trace, m);
    return hipGetLastError();
}

int64_t act_map_bytes(const life_layout &L) {
    return act_cols((L.w + 63) / 64) * act_rows(L.h) * kActWords * (int64_t)sizeof(uint32_t);
}

int64_t skip_tiles(const life_layout &L, int m) {
    const int64_t T = (int64_t)tile_waves(true) * temporal_rows(true) - 2 * (int64_t)m;
    if (!is_bit(L) || T < 1) return 0;
    return act_cols((L.w + 63) / 64) * ((L.h + T - 1) / T);
}

hipError_t launch_tskip(const life_layout &L, const uint8_t *in, uint8_t *out, int m, const uint32_t *src_map,
                        uint32_t *dst_map, uint8_t *cls, unsigned long long *cnt, hipStream_t s,
                        const RuleWords *rule, unsigned long long *pop) {
    const int K = L.generations_per_exchange;
    const int64_t T = (int64_t)tile_waves(true) * temporal_rows(true) - 2 * (int64_t)m;
    // both axes wrap in the stencil: whole pairs, no apron to fill
    if (!is_bit(L) || m < 1 || m > K || m > 32 || K < 2 || L.yapron != K || T < 1 || L.w % 64 != 0)
        return hipErrorInvalidValue;
    KArgs k{};
    TArgs &a = k.t;
    a.in = in;
    a.out = out;
    a.pitch = L.pitch;
    a.xoff = L.xoff;
    a.W = L.w / 64;
    a.h = L.h;
    a.ya = L.yapron;
    a.m = m;
    a.btx1 = -1;  // plain tiles: no banded column, no tail split, dispatch order
    k.ntx = act_cols(a.W);
    k.nty = (L.h + T - 1) / T;
    k.ntx_mul = tile_recip((uint32_t)k.ntx);
    k.cls = cls;
    k.act = dst_map;
    const int64_t tiles = k.ntx * k.nty;
    if (tiles > 0x7fffffff || !tile_body_fits32(a, tile_waves(true) * temporal_rows(true), k.nty))
        return hipErrorInvalidValue;
    PlanArgs p{src_map, dst_map, cls, cnt, a.W, a.h, T, k.ntx, k.nty, m};
    act_plan_kernel<<<(unsigned)((tiles + 255) / 256), 256, 0, s>>>(p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(dst_map, 0, (size_t)act_map_bytes(L), s);
    if (e != hipSuccess) return e;
    if (pop) {
        if (m > kPopGens) return hipErrorInvalidValue;
        const PopArgs pa{pop, 0, L.h};
        const void *pfn = skip_pop_k(rule != nullptr);
        if (!pfn) return hipErrorInvalidValue;
        if (rule) {
            RPKArgs ra{k, *rule, pa};
            return launch_fn(pfn, (unsigned)tiles, 64u * (unsigned)tile_waves(true), &ra, s, nullptr, nullptr);
        }
        PKArgs ka{k, pa};
        return launch_fn(pfn, (unsigned)tiles, 64u * (unsigned)tile_waves(true), &ka, s, nullptr, nullptr);
    }
    const void *fn = skip_k(rule != nullptr);
    if (!fn) return hipErrorInvalidValue;
    if (rule) {
        RKArgs ra{k, *rule};
        return launch_fn(fn, (unsigned)tiles, 64u * (unsigned)tile_waves(true), &ra, s, nullptr, nullptr);
    }
    return launch_fn(fn, (unsigned)tiles, 64u * (unsigned)tile_waves(true), &k, s, nullptr, nullptr);
}

namespace {
// Instances of the dataflow tiles (bit, both axes wrapped): one per tile shape
// and hand-off form.
// (LIFE_FLOW_BANDS=0: full-width tiles in the last column; A/B knob)
bool flow_bands_enabled() { static const bool on = env::read(env::kFlowBands) != 0; return on; }
const void *flow_kernel_of(const life_layout &L, int flow, bool band = false, bool rule7 = false) {
    if (!is_bit(L)) return nullptr;
    const int R = temporal_rows(true), NW = tile_waves(true);
#define LIFE_BIT_CASE(r, nw)                                                                     \
    if (rule7 && R == r && NW == nw) {                                                           \
        if (band)                                                                                \
            return flow == 2 ? (const void *)tflow7_kernel<r, true, true, 2, nw, true>           \
                             : (const void *)tflow7_kernel<r, true, true, 1, nw, true>;          \
        return flow == 2 ? (const void *)tflow7_kernel<r, true, true, 2, nw>                     \
                         : (const void *)tflow7_kernel<r, true, true, 1, nw>;                    \
    }
    LIFE_BIT_SHAPES(LIFE_BIT_CASE)
#undef LIFE_BIT_CASE
#define LIFE_BIT_CASE(r, nw)                                                                     \
    if (R == r && NW == nw) {                                                                    \
        if (band)                                                                                \
            return flow == 2 ? (const void *)tflow_kernel<r, true, true, 2, nw, true>            \
                             : (const void *)tflow_kernel<r, true, true, 1, nw, true>;           \
        return flow == 2 ? (const void *)tflow_kernel<r, true, true, 2, nw>                      \
                         : (const void *)tflow_kernel<r, true, true, 1, nw>;                     \
    }
    LIFE_BIT_SHAPES(LIFE_BIT_CASE)
#undef LIFE_BIT_CASE
    return nullptr;
}
// the banded form for this geometry: a banded last column (tile_geom)
bool flow_band(const TileGeom &g) { return g.nband > 0 && flow_bands_enabled(); }
// the dataflow form's geometry: one band at most (tile_geom's one_band mode)
TileGeom flow_geom(const life_layout &L, int m) { return tile_geom(L, m, true); }
}  // namespace

int64_t flow_items_per_pass(const life_layout &L, int m, bool work_only) {
    const TileGeom g = flow_geom(L, m);
    if (!flow_band(g)) return g.ntx * g.nty;
    const int64_t B = 64 >> g.band[0].gsh, ngroups = (g.nty + B - 1) / B;
    // work_only: without the no-op padding items of the last group
    return work_only ? (g.ntx - 1) * g.nty + ngroups : ngroups * ((g.ntx - 1) * B + 1);
}

bool flow_ok(const life_layout &L, int m) {
    // an instance for this encoding / tile shape, and the dependency rule
    // reads tile rows ty-2..ty+2: a window may reach at most one tile row
    // beyond its neighbours (ghost rows <= T)
    if (!flow_kernel_of(L, 1) || m < 1) return false;
    const TileGeom g = flow_geom(L, m);
    return g.rows >= tile_ghost(L, m);
}

int flow_slots(const life_layout &L, bool rule7) {
    static int cached[2] = {0, 0}, key[2] = {-1, -1};
    const int k = is_bit(L) ? temporal_rows(true) * 64 + tile_waves(true) : -2;
    if (k != key[rule7]) {
        cached[rule7] = slots_of(flow_kernel_of(L, 1, false, rule7), 64 * tile_waves(is_bit(L)));
        key[rule7] = k;
    }
    return cached[rule7];
}

hipError_t prewarm_tflow(const life_layout &L, int m, int flow, unsigned int *head, hipStream_t s, bool rule7) {
    const TileGeom g = flow_geom(L, m);
    const void *fn = flow_kernel_of(L, flow, flow_band(g), rule7);
    if (!fn || !flow_ok(L, m) || flow_slots(L, rule7) <= 0) return hipErrorInvalidValue;  // (caches the slot count)
    FArgs f{};  // no items: the one workgroup pulls item 0 and leaves
    f.head = head;
    const hipError_t e = hipMemsetAsync(head, 0, sizeof(unsigned int), s);
    if (e != hipSuccess) return e;
    return launch_fn(fn, 1u, 64u * (unsigned)tile_waves(true), &f, s, nullptr, nullptr);
}

hipError_t launch_tflow(const life_layout &L, const uint8_t *in, uint8_t *out, int m, int64_t passes,
                        unsigned int *head, unsigned int *done, Wrap wrap, int flow, hipStream_t s, hipEvent_t ev0,
                        hipEvent_t ev1, bool rule7) {
    const void *fn = flow_kernel_of(L, flow, false, rule7);
    if (!fn || !wrap.x || !wrap.y || m < 1 || m > 32 || m > L.generations_per_exchange || passes < 1 ||
        !flow_ok(L, m))
        return hipErrorInvalidValue;
    const TileGeom g = flow_geom(L, m);
    FArgs f{};
    f.t.in = in;
    f.t.out = out;
    f.t.pitch = L.pitch;
    f.t.xoff = L.xoff;
    f.t.W = (L.w + g.cells - 1) / g.cells;
    f.t.h = L.h;
    f.t.ya = L.yapron;
    f.t.m = m;
    const bool band = flow_band(g);
    if (band) fn = flow_kernel_of(L, flow, true, rule7);
    TileGeom gb = g;
    if (!band) gb.nband = 0, gb.bcol = -1;
    set_bands(f.t, gb);
    f.ntx = g.ntx;
    f.nty = g.nty;
    f.B = band ? 64 >> g.band[0].gsh : 1;
    f.ngroups = (g.nty + f.B - 1) / f.B;
    f.per_pass = flow_items_per_pass(L, m);
    f.items = passes * f.per_pass;
    f.head = head;
    f.done = done;
    if (!tile_body_fits32(f.t, tile_waves(true) * temporal_rows(true), f.nty)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(head, 0, sizeof(unsigned int), s);  // the error word is the caller's
    if (e == hipSuccess) e = hipMemsetAsync(done, 0, sizeof(unsigned int) * (size_t)(g.ntx * g.nty), s);
    if (e != hipSuccess) return e;
    const int n = flow_slots(L, rule7);  // resident workgroups
    if (n <= 0) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>(f.items, n);
    // every workgroup pulls one item past the last: the 32-bit head must not wrap
    if (f.items + (int64_t)grid > kFlowMaxHead) return hipErrorInvalidValue;
    return launch_fn(fn, grid, 64u * (unsigned)tile_waves(true), &f, s, ev0, ev1);
}

int reg_small_rows(const life_layout &L) {
    const int64_t W = (L.w + 31) / 32;
    if (W > kRegMaxW || L.h <= 0) return 0;
    int64_t Wp = 1;
    while (Wp < W) Wp <<= 1;
    const int64_t strips = kRegThreads / Wp;
    for (int R : kRegRows)
        if (L.h % R == 0 && L.h / R <= strips) return R;
    return 0;
}

hipError_t launch_reg_small(const life_layout &L, const uint8_t *in, uint8_t *out, int64_t gens,
                            hipStream_t s) {
    const int R = reg_small_rows(L);
    if (R == 0 || gens <= 0 || gens > INT32_MAX) return hipErrorInvalidValue;
    RArgs a;
    a.in = in;
    a.out = out;
    a.pitch = L.pitch;
    a.xoff = L.xoff;
    a.ya = L.yapron;
    a.w = (int32_t)L.w;
    a.h = (int32_t)L.h;
    a.W = (int32_t)((L.w + 31) / 32);
    a.lgWp = 0;
    while ((1 << a.lgWp) < a.W) ++a.lgWp;
    a.gens = (int32_t)gens;
    a.bit = is_bit(L) ? 1 : 0;
    a.ns = (int32_t)(L.h / R);
    a.own = a.h;
    a.K = 0;
    a.nat_in = a.nat_out = 0;
    return L.w % 32 ? launch_rs<true, false>(a, R, 1, s) : launch_rs<false, false>(a, R, 1, s);
}

// Windowed plan: strip height R, halo K, strips per window ns (ns*R = own +
// 2K), owned rows per workgroup.  Zero when the grid is not a VGPR shape, or
// too short for one window to leave owned rows to more than one workgroup.
// R = 0: automatic, R = 1 and K = min(30, (ns - 4) / 2), i.e. 4 owned rows per
// workgroup -- the p46gun_big sweep (profiles/r01/p46_window_*.jsonl): R = 1
// beats R >= 2 at every K, and the rate rises with K up to 30 (a
// generation costs one barrier's latency whatever the window holds, so
// deeper halos mean fewer launches).
RegWinPlan reg_win_plan(const life_layout &L, int R, int K) {
    RegWinPlan p{};
    const int64_t W = (L.w + 31) / 32;
    if (W > kRegMaxW || L.h <= 0) return p;
    int64_t Wp = 1;
    while (Wp < W) Wp <<= 1;
    const int64_t ns = kRegThreads / Wp;
    if (R == 0) {
        R = 1;
        K = (int)std::min<int64_t>(30, (ns - 4) / 2);
        if (K < 8) return p;
    }
    if (K < 1 || (R != 1 && R != 2 && R != 3 && R != 4 && R != 5 && R != 6 && R != 8)) return p;
    const int64_t own = ns * R - 2 * K;
    if (own < 1 || own >= L.h) return p;
    p.R = R;
    p.K = K;
    p.ns = (int)ns;
    p.own = (int)own;
    p.blocks = (int)((L.h + own - 1) / own);
    return p;
}

hipError_t launch_reg_win(const life_layout &L, const RegWinPlan &p, const uint8_t *in, uint8_t *out, int gens,
                          hipStream_t s, bool nat_in, bool nat_out) {
    if (p.blocks < 1 || gens < 1 || gens > p.K || in == out) return hipErrorInvalidValue;
    RArgs a;
    a.in = in;
    a.out = out;
    a.pitch = L.pitch;
    a.xoff = L.xoff;
    a.ya = L.yapron;
    a.w = (int32_t)L.w;
    a.h = (int32_t)L.h;
    a.W = (int32_t)((L.w + 31) / 32);
    a.lgWp = 0;
    while ((1 << a.lgWp) < a.W) ++a.lgWp;
    a.gens = gens;
    a.bit = is_bit(L) ? 1 : 0;
    a.ns = p.ns;
    a.own = p.own;
    a.K = p.K;
    const bool fits = L.xoff + 4 * (int64_t)a.W <= L.pitch;  // natural words inside the padded row
    a.nat_in = nat_in && fits ? 1 : 0;
    a.nat_out = nat_out && fits ? 1 : 0;
    const unsigned b = (unsigned)p.blocks;
    return L.w % 32 ? launch_rs<true, true>(a, p.R, b, s) : launch_rs<false, true>(a, p.R, b, s);
}

int64_t small_lds_bytes(const life_layout &L) {
    const int64_t W = (L.w + 31) / 32;
    return W > kSmallThreads ? INT64_MAX : 2 * W * L.h * 4;
}

hipError_t launch_small(const life_layout &L, const uint8_t *in, uint8_t *out, int64_t gens, hipStream_t s) {
    const int64_t bytes = small_lds_bytes(L);
    if (bytes > kSmallMaxLds || gens <= 0 || gens > INT32_MAX) return hipErrorInvalidValue;
    static bool attr_set = false;  // opt in to more than 64 KiB of dynamic LDS
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute((const void *)small_kernel,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmallMaxLds);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    SArgs a;
    a.in = in;
    a.out = out;
    a.pitch = L.pitch;
    a.xoff = L.xoff;
    a.ya = L.yapron;
    a.w = (int32_t)L.w;
    a.h = (int32_t)L.h;
    a.W = (int32_t)((L.w + 31) / 32);
    a.gens = (int32_t)gens;
    a.bit = is_bit(L) ? 1 : 0;
    small_kernel<<<1, kSmallThreads, (size_t)bytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace life
