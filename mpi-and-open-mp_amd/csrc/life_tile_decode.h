// life_tile_decode.h -- which item a workgroup of a per-launch tile kernel
// runs (tstep_bit_kernel and its 7-gate, table-rule and census twins), from
// constants the launcher computes once, in 32-bit arithmetic.
//
// A launch is up to kMaxRegions tile regions, each listing its ordinary tiles
// row-major (ntx columns without the banded one), then the banded items of its
// last tile column; optionally a tail of half-height tiles laid out the same
// way; optionally the XCD-aware renumbering of the first xcd_n workgroups.
// Every count of a grid that fits in HBM is far below 2^31 (a tile owns at
// least 62 pairs x 1 row; the launcher checks the range and fails the launch
// otherwise), so the kernels need no 64-bit division: wr / ntx is one
// multiply-high by a host-made reciprocal and one correction step.
//
// Plain C++ (host and device): life_plan.cpp replays the mapping on the CPU
// through life_tile_decode_query (tests/test_tile_decode_host.py).
#pragma once
#include <stdint.h>

#include "life_mi355x.h"

#ifdef __HIP__
#define LIFE_TD_HD __host__ __device__ inline
#else
#define LIFE_TD_HD inline
#endif

namespace life {

constexpr int kTdMaxRegions = LIFE_TILE_MAX_REGIONS;  // = kMaxRegions (life_kernels.h)
constexpr int kTdMaxBands = 2;                        // = kMaxBands (life_host.h)

// floor(2^32 / d) (d = 1: 2^32 - 1): mulhi(n, it) is n / d or one less for
// every 32-bit n, so one conditional step makes quotient and remainder exact
inline uint32_t tile_recip(uint32_t d) { return d <= 1 ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / d); }
LIFE_TD_HD void tile_divmod(uint32_t n, uint32_t d, uint32_t mul, uint32_t &q, uint32_t &r) {
    q = (uint32_t)(((uint64_t)n * mul) >> 32);
    r = n - q * d;
    if (r >= d) {
        ++q;
        r -= d;
    }
}

struct TileDecRegion {
    int32_t tx0, ty0, rows;  // first tile column and row, tile rows
    uint32_t ntx;            // ordinary tile columns (without the banded one)
    uint32_t nfull;          // ntx * rows: the region's items before its banded ones
    uint32_t mul;            // tile_recip(ntx)
};
struct TileDec {
    uint32_t xcd_n, xcd_per, xcd_rem;  // workgroups renumbered, xcd_n / 8 and xcd_n % 8
    uint32_t nwg;                      // items of the regions; workgroups beyond (and not tail) do nothing
    uint32_t tail_first;               // first workgroup of the tail; 0xFFFFFFFF: no tail
    int32_t nreg;
    uint32_t first[kTdMaxRegions];     // first item of each region
    TileDecRegion reg[kTdMaxRegions], tail;
};

enum TileKind : int32_t { kTileNone = 0, kTileFull = 1, kTileBand = 2, kTileTail = 3, kTileTailBand = 4 };
struct TileItem {
    int32_t kind;
    int32_t region;  // of a full-height item
    int32_t tx, ty;  // an ordinary tile's column and row (tail: row within the tail)
    int32_t ty0, rows;  // a banded item's region: first tile row and tile rows
    uint32_t bi;        // a banded item's index among its region's banded items
};

// The per-XCD row-major renumbering of workgroups [0, xcd_n): XCD x = wg % 8
// runs items first_x + wg / 8.  A bijection of [0, xcd_n).
LIFE_TD_HD uint32_t tile_xcd_item(const TileDec &d, uint32_t wg) {
    if (wg >= d.xcd_n) return wg;
    const uint32_t x = wg & 7u, k = wg >> 3, per = d.xcd_per, rem = d.xcd_rem;
    return (x < rem ? x * (per + 1u) : rem * (per + 1u) + (x - rem) * per) + k;
}

LIFE_TD_HD TileItem tile_decode(const TileDec &d, uint32_t wg0) {
    TileItem it = {kTileNone, 0, 0, 0, 0, 0, 0u};
    const uint32_t wg = tile_xcd_item(d, wg0);
    if (wg >= d.tail_first) {
        const TileDecRegion &t = d.tail;
        const uint32_t i = wg - d.tail_first;
        it.rows = t.rows;
        if (i < t.nfull) {
            uint32_t q, r;
            tile_divmod(i, t.ntx, t.mul, q, r);
            it.kind = kTileTail;
            it.tx = t.tx0 + (int32_t)r;
            it.ty = (int32_t)q;
        } else {
            it.kind = kTileTailBand;
            it.bi = i - t.nfull;
        }
        return it;
    }
    if (wg >= d.nwg) return it;
    int k = 0;
    while (k + 1 < d.nreg && wg >= d.first[k + 1]) ++k;
    const TileDecRegion &g = d.reg[k];
    const uint32_t wr = wg - d.first[k];
    it.region = k;
    it.ty0 = g.ty0;
    it.rows = g.rows;
    if (wr < g.nfull) {
        uint32_t q, r;
        tile_divmod(wr, g.ntx, g.mul, q, r);
        it.kind = kTileFull;
        it.tx = g.tx0 + (int32_t)r;
        it.ty = g.ty0 + (int32_t)q;
    } else {
        it.kind = kTileBand;
        it.bi = wr - g.nfull;
    }
    return it;
}

// The constants of a launch description; false (and *why, when given) when a
// count leaves the 32-bit range the kernels work in or the description is
// inconsistent.  The limits leave room for every intermediate: pair columns
// up to 62 tx1 + 64 and rows up to (ty1 + 17) T + window_rows stay below 2^31.
inline bool tile_decode_fill(const life_tile_launch &l, TileDec *d, const char **why = nullptr) {
    auto fail = [&](const char *w) {
        if (why) *why = w;
        return false;
    };
    const int64_t lim = (int64_t)1 << 31;
    *d = TileDec{};
    if (l.nreg < 1 || l.nreg > kTdMaxRegions || l.nband < 0 || l.nband > kTdMaxBands) return fail("regions / bands");
    const int64_t T = (int64_t)l.window_rows - 2 * (int64_t)l.m;
    if (l.m < 1 || l.window_rows < 2 || T < 1 || l.window_rows > (1 << 16)) return fail("window rows / generations");
    d->nreg = l.nreg;
    int64_t first = 0;
    for (int k = 0; k < l.nreg; k++) {
        const int64_t ntx = l.tx1[k] - l.tx0[k] - (l.nband > 0 && l.tx1[k] == l.btx1 ? 1 : 0);
        const int64_t rows = l.ty1[k] - l.ty0[k];
        // (a tail planned from the region's first tile row on leaves it no row: every workgroup is a tail item)
        if (l.tx0[k] < 0 || l.ty0[k] < 0 || rows < (l.tail_ntx > 0 ? 0 : 1) || ntx < 0 || l.tx1[k] <= l.tx0[k])
            return fail("empty region");
        if (l.tx1[k] * 62 + 64 >= lim || (l.ty1[k] + 17) * T + l.window_rows >= lim || ntx * rows >= lim)
            return fail("tile indices beyond 32 bits");
        if (l.first[k] != first || l.first[k + 1] < first + ntx * rows || l.first[k + 1] >= lim)
            return fail("item counts");
        first = l.first[k + 1];
        d->first[k] = (uint32_t)l.first[k];
        d->reg[k] = TileDecRegion{(int32_t)l.tx0[k], (int32_t)l.ty0[k], (int32_t)rows, (uint32_t)ntx,
                                  (uint32_t)(ntx * rows), tile_recip((uint32_t)ntx)};
    }
    d->nwg = (uint32_t)first;
    d->tail_first = 0xFFFFFFFFu;
    if (l.tail_ntx > 0) {
        const int64_t TS = (int64_t)(l.window_rows / 2) - 2 * (int64_t)l.m;
        if (TS < 1 || l.nreg != 1 || l.tail_first != first || l.tail_yend <= l.tail_y || l.tail_y < 0 || l.tail_tx0 < 0)
            return fail("tail");
        const int64_t rows = (l.tail_yend - l.tail_y + TS - 1) / TS;
        const int64_t ntx = l.tail_ntx - (l.nband > 0 && l.tail_tx0 + l.tail_ntx == l.btx1 ? 1 : 0);
        if ((l.tail_tx0 + l.tail_ntx) * 62 + 64 >= lim || l.tail_yend + 17 * T + l.window_rows >= lim ||
            ntx * rows >= lim || first + ntx * rows + 2 * rows >= lim)
            return fail("tail indices beyond 32 bits");
        d->tail_first = (uint32_t)l.tail_first;
        d->tail = TileDecRegion{(int32_t)l.tail_tx0, 0, (int32_t)rows, (uint32_t)ntx, (uint32_t)(ntx * rows),
                                tile_recip((uint32_t)ntx)};
    }
    if (l.xcd_n < 0 || l.xcd_n > first) return fail("renumbered workgroups");
    d->xcd_n = (uint32_t)l.xcd_n;
    d->xcd_per = d->xcd_n >> 3;
    d->xcd_rem = d->xcd_n & 7u;
    return true;
}

}  // namespace life
