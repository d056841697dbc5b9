// life_act.h -- the activity map of the skip-dead passes (LIFE_OPT_SKIP_DEAD):
// the ONE definition of which map cells a bit tile's window reads, which it
// owns, and the wrap on both axes.  The plan kernel (life_kernels.hip), the
// host (life_step.hip) and the CPU tests (tests/test_skip_plan.py, g++ alone)
// all include it; no HIP types.
//
// One map per grid buffer.  A map cell covers kActPairs pair columns (a tile
// column, whatever the pass length m) by kActRows owned rows; ncol = ceil(W /
// kActPairs) = the tile columns, nrow = ceil(h / kActRows).  The tile height
// T = 8R - 2m changes with m from pass to pass inside one call (61
// generations: 11, 10, 10, 10, 10, 10), the map's granularity never.
//
// A map cell is kActWords row masks (bit r = row 32 R + r of the block "may
// hold a live cell"): over all its pairs, over its FIRST pair alone and over
// its LAST pair alone.  A tile's window is its own tile column plus ONE pair
// on either side: the last pair of the column on its left and the first pair
// of the column on its right.  With a flag per block only, a glider in tile
// column 0 of a 3-column grid would run the tiles of all three columns every
// pass (each column's window touches both others), and every tile row whose
// window touches the glider's 32-row block; with the masks the plan is exact
// to the row and, at the window's edges, to the pair.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LIFE_ACT_HD __host__ __device__ inline
#else
#define LIFE_ACT_HD inline
#endif

namespace life {

constexpr int kActRows = 32;   // owned rows per map cell: the bits of a mask
constexpr int kActPairs = 62;  // pair columns per map cell: one tile column
constexpr int kActWords = 3;   // masks per map cell
constexpr int kActAny = 0, kActFirst = 1, kActLast = 2;

// a tile's class in a skip-dead pass (act_plan_kernel)
constexpr int kActSkip = 0;   // window dead, owned block of dst already dead: nothing runs
constexpr int kActClear = 1;  // window dead, dst's old block may hold a live cell: zero stores
constexpr int kActRun = 2;    // the tile body runs

// mask k of map cell (r, c)
LIFE_ACT_HD int64_t act_word(int64_t r, int64_t c, int64_t ncol, int k) { return (r * ncol + c) * kActWords + k; }
LIFE_ACT_HD int64_t act_cols(int64_t W) { return (W + kActPairs - 1) / kActPairs; }
LIFE_ACT_HD int64_t act_rows(int64_t h) { return (h + kActRows - 1) / kActRows; }

// Up to three ranges of one axis, in cells [lo[i], hi[i]) and as the map
// indices [a[i], b[i]) holding them; hi[i] == lo[i]: empty.
struct ActSpan {
    int64_t lo[3], hi[3], a[3], b[3];
};

// The cells [lo, hi) of a periodic axis of `period` cells, `unit` cells per
// map cell (the last map cell may be partial), hi > lo.  A range as long as
// the axis is the whole axis; else the part below 0 wraps to the axis' end
// and the part beyond `period` to its start -- a last tile row shorter than m
// makes tile row 0's window reach two tile rows up, which is just a longer
// first part here.  (Fixed slots -- below 0, inside, beyond -- and no
// compaction: the kernel keeps them in registers.)
LIFE_ACT_HD ActSpan act_span(int64_t lo, int64_t hi, int64_t period, int64_t unit) {
    if (hi - lo >= period) {
        lo = 0;
        hi = period;
    }
    const int64_t x0[3] = {lo < 0 ? lo + period : 0, lo < 0 ? 0 : lo, 0};
    const int64_t x1[3] = {lo < 0 ? period : 0, hi > period ? period : hi, hi > period ? hi - period : 0};
    ActSpan s;
    for (int i = 0; i < 3; i++) {
        const bool on = x1[i] > x0[i];
        s.lo[i] = on ? x0[i] : 0;
        s.hi[i] = on ? x1[i] : 0;
        s.a[i] = on ? x0[i] / unit : 0;
        s.b[i] = on ? (x1[i] - 1) / unit + 1 : 0;
    }
    return s;
}
// the bits of map row r that range i of a row span covers (r in [a[i], b[i]))
LIFE_ACT_HD uint32_t act_row_bits(const ActSpan &s, int i, int64_t r) {
    const int64_t y0 = r * kActRows, lo = s.lo[i] > y0 ? s.lo[i] - y0 : 0,
                  hi = s.hi[i] < y0 + kActRows ? s.hi[i] - y0 : kActRows;
    if (hi <= lo) return 0u;
    return (hi - lo >= 32 ? 0xFFFFFFFFu : ((1u << (hi - lo)) - 1u)) << lo;
}

// Tile (tx, ty) of a pass of m generations over W pair columns x h rows,
// tiles of T owned rows (life::tile_geom without banded columns) x kActPairs
// pairs.  Owned: rows [ty T, min(ty T + T, h)), pairs [62 tx, min(62 tx + 62,
// W)), map column tx.  Its window: the owned rows plus m ghost rows at each
// end, the owned pairs plus one edge lane column at each side (m <= 32 cells
// is inside one 64-cell pair), both wrapped: pair 62 tx - 1 is the last pair
// of map column act_left_col, pair min(62 tx + 62, W) the first of act_right_col.
LIFE_ACT_HD int64_t act_own_end(int64_t t, int64_t T, int64_t n) { return (t + 1) * T < n ? (t + 1) * T : n; }
LIFE_ACT_HD ActSpan act_own_rows(int64_t ty, int64_t T, int64_t h) {
    return act_span(ty * T, act_own_end(ty, T, h), h, kActRows);
}
LIFE_ACT_HD ActSpan act_read_rows(int64_t ty, int64_t T, int m, int64_t h) {
    return act_span(ty * T - m, act_own_end(ty, T, h) + m, h, kActRows);
}
LIFE_ACT_HD ActSpan act_read_cols(int64_t tx, int64_t W) {
    return act_span(tx * kActPairs - 1, act_own_end(tx, kActPairs, W) + 1, W, kActPairs);
}
LIFE_ACT_HD int64_t act_left_col(int64_t tx, int64_t W) { return tx > 0 ? tx - 1 : act_cols(W) - 1; }
LIFE_ACT_HD int64_t act_right_col(int64_t tx, int64_t W) { return act_own_end(tx, kActPairs, W) < W ? tx + 1 : 0; }

// A tile's window may hold a live cell: some row of `rows` (act_read_rows) is
// set in its own column's mask, in the last-pair mask of the column on its
// left or in the first-pair mask of the column on its right.
LIFE_ACT_HD bool act_window_live(const uint32_t *map, int64_t W, const ActSpan &rows, int64_t tx) {
    const int64_t ncol = act_cols(W), cl = act_left_col(tx, W), cr = act_right_col(tx, W);
    for (int i = 0; i < 3; i++)
        for (int64_t r = rows.a[i]; r < rows.b[i]; r++) {
            const uint32_t v = map[act_word(r, tx, ncol, kActAny)] | map[act_word(r, cl, ncol, kActLast)] |
                               map[act_word(r, cr, ncol, kActFirst)];
            if (v & act_row_bits(rows, i, r)) return true;
        }
    return false;
}
// A tile's owned block may hold a live cell (`rows`: act_own_rows).
LIFE_ACT_HD bool act_own_live(const uint32_t *map, int64_t W, const ActSpan &rows, int64_t tx) {
    const int64_t ncol = act_cols(W);
    for (int i = 0; i < 3; i++)
        for (int64_t r = rows.a[i]; r < rows.b[i]; r++)
            if (map[act_word(r, tx, ncol, kActAny)] & act_row_bits(rows, i, r)) return true;
    return false;
}

}  // namespace life
