// life_kernels.h -- host-side launchers of the gfx950 Game-of-Life kernels.
//
// All launchers are asynchronous on `s` and return the hipError_t of the
// launch.  Buffers are the padded shard layout of life_layout (see
// include/life_mi355x.h and DESIGN.md "Data layout in HBM").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "life_host.h"
#include "life_mi355x.h"

namespace life {

// Region of owned cells a stencil launch updates: 16-byte units [u0,u1) of
// every padded row, owned rows [r0,r1) (0-based, padded row = r + 1).
struct Region {
    int64_t u0, u1, r0, r1;
};

// Kernel arguments of one stencil launch (by value).
struct StepArgs {
    const uint8_t *in;
    uint8_t *out;
    uint8_t *sink;  // >= 1 KiB scratch: stores of lanes outside the region land here
    int64_t pitch, xoff, units, w, h, ya;
    int64_t u0, u1, r0, r1, nbx;
    int32_t wrapy;
    int32_t xcd;  // 1: blocks renumbered into per-XCD row-major runs (step_kernel)
};

// Wrap flags: a periodic axis that lies entirely inside the shard (dims[d]
// == 1) is wrapped by the stencil itself (no apron, no fill kernel); the
// apron of a partitioned axis must hold the neighbours' cells.
struct Wrap {
    bool x, y;
};

// One generation over `reg`: reads `in`, writes `out`.  `rule` (here and in
// launch_tstep; bit encoding only): the words of a rule other than B3/S23
// (life::rule_words) -- the launch then runs the table-rule instance of the
// same kernel; null: B3/S23.
hipError_t launch_step(const life_layout &L, const uint8_t *in, uint8_t *out, uint8_t *sink,
                       const Region &reg, Wrap wrap, hipStream_t s, const RuleWords *rule = nullptr);

// Tuning knobs of the stencil (rows per lane, rows of loads in flight);
// defaults chosen by measurement, overridable by LIFE_STEP_ROWS / LIFE_STEP_DEPTH.
struct StepTuning {
    int rows, depth;
};
StepTuning step_tuning(bool bit);
void set_step_tuning(int kernel, int rows, int depth);  // kernel -1: both

// Temporally blocked stencil (layouts with generations_per_exchange = K > 1,
// either encoding): tiles of 62 lane columns (bit: 64-cell interleaved pairs;
// byte: 32-cell words) x `rows` rows (one workgroup each), m <= min(K, 32)
// generations per launch from `in` to `out`; a bit tile's window holds m
// ghost rows above and below (byte: K), so the tile height depends on m:
// tile_geom(L, m).
constexpr int kMaxRegions = 4;  // regions one temporal launch may hold
struct TileRegion {
    int64_t tx0, tx1, ty0, ty1;
};
struct TileGeom {
    int64_t lanes;  // owned lane columns per tile (62)
    int64_t cells;  // cells per lane column: 64 (bit pairs) or 32 (byte words)
    int64_t rows, ntx, nty;
    // nband > 0: tile column bcol runs as nband sub-columns of banded items
    // (life::band_split of the pairs it owns: groups of 2^gsh lanes, 64 >>
    // gsh tile rows per workgroup)
    int nband;
    BandCol band[kMaxBands];
    int64_t bcol;  // the banded column (ntx - 1), -1 without banding
};
// one_band: at most one sub-column, and only a column owning <= 30 pairs (the
// dataflow form's geometry; LIFE_BAND_SPLIT=0 gives it everywhere)
TileGeom tile_geom(const life_layout &L, int m, bool one_band = false);
// workgroups (items) one launch of region r takes: its full tiles, plus the
// banded items of every sub-column when it holds the banded column
int64_t region_items(const TileGeom &g, const TileRegion &r);
// tile rows per banded item of each sub-column of the tile columns [.., tx1)
// (none unless the region holds the banded column)
BandRows region_bands(const TileGeom &g, int64_t tx1);
int tile_ghost(const life_layout &L, int m);  // ghost rows per window end: m (bit), K or 1 (byte, m = 1)
// Rows a temporally blocked buffer is allocated beyond its layout's `rows`:
// the last tile's window (<= 8 waves x 96 byte rows, 16 x 24 bit rows) may
// read past the bottom apron without clamping.
constexpr int64_t kTemporalSlackRows = 8 * 96;
// Dataflow form of the tiles (tflow_kernel): `passes` launches of m
// generations over a single shard whose axes both wrap inside it, as ONE
// persistent launch (no drain between passes).  `head` (2 words: the queue
// head, then an error word the caller zeroes once and reads: 1 + an item
// whose dependency wait timed out, 0 if none) and `done`
// (ntx * nty words, tile_geom(L, m)) are device scratch the launch zeroes;
// flow 1: write-through (`sc1`) stores, 2: plain stores + release fence.
// Pass p reads `in` for even p and `out` for odd p: after it, the result is
// in `out` when passes is odd, else in `in`.
bool flow_ok(const life_layout &L, int m);
// work items of one dataflow pass (tiles, or tiles + banded items of a banded
// last column; the queue also holds no-op items that pad the last group of
// banded rows unless work_only)
int64_t flow_items_per_pass(const life_layout &L, int m, bool work_only = false);
// resident workgroups of L's dataflow kernel on this device (rule7: of its 7-gate arm, tflow7_kernel)
int flow_slots(const life_layout &L, bool rule7 = false);
// resident workgroups of L's per-launch tile kernel on this device (rule: of its table-rule instance)
// (rule7: of the 7-gate arm, tstep_bit7_kernel)
int tile_slots(const life_layout &L, bool rule = false, bool rule7 = false);
// ev0 / ev1 (optional): events stamped with the kernel dispatch's own start
// and end (hipExtLaunchKernel) -- no event packets between launches.
// One empty launch of the dataflow instance launch_tflow(L, m, flow) would use
// (and its occupancy query): the first launch of a kernel in a process costs
// ~140 us, which a device pays here at creation instead of inside its first
// dataflow step call.  `head`: the caller's scratch (2 words).
hipError_t prewarm_tflow(const life_layout &L, int m, int flow, unsigned int *head, hipStream_t s,
                         bool rule7 = false);
hipError_t launch_tflow(const life_layout &L, const uint8_t *in, uint8_t *out, int m, int64_t passes,
                        unsigned int *head, unsigned int *done, Wrap wrap, int flow, hipStream_t s,
                        hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, bool rule7 = false);
// Deep-halo passes (bit tiles, partitioned axes): the pass also advances the
// apron cells that stay valid for the next pass -- y rows [-y, 0) and
// [h, h + y) (the tile grid then spans h + 2y rows from owned row -y; the
// windows read at most y + m <= yapron rows above), and with x the apron
// pairs -1 and W are stored by the tile lanes that hold them.  A K-deep halo
// then feeds K generations (several passes) instead of one pass.
struct Extend {
    int64_t y = 0;
    bool x = false;
};
// Up to 4 disjoint tile regions in one launch; *valu_lane_ops (optional):
// the modelled VALU lane-ops of the launch as tiled (tstep_valu_per_tile_lane).
// Regions are in tile coordinates of tile_geom(extended_layout(L, ext), m).
// `concurrent`: items of another tile launch dispatched just before this one
// and running beside it (an exchange pass's ring beside its interior); the
// launch-tail plan of a one-region launch counts them as occupying slots
// (< 0: no launch-tail split).
hipError_t launch_tstep(const life_layout &L, const uint8_t *in, uint8_t *out, const TileRegion *r, int nreg,
                        int m, Wrap wrap, hipStream_t s,
                        double *valu_lane_ops = nullptr, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                        Extend ext = Extend{}, int64_t concurrent = 0, const RuleWords *rule = nullptr,
                        unsigned long long *pop = nullptr, bool rule7 = false);
// `rule7` (here, in launch_tflow and prewarm_tflow; LIFE_OPT_RULE7): the B3/S23
// bit tiles run their 7-gate arm (ConwayRule7, life_bitops.h: 20 VALU per pair
// row instead of 22) -- the kernels of a launch without `rule` and `pop`; the
// table-rule, census, skip-dead and byte tiles have one arm and ignore it.
// Census instances of the bit tiles (LIFE_OPT_POPULATION): with `pop` (here
// and in launch_tskip; bit shards of whole pairs, w % 64 == 0) every tile of
// the launch also adds the live cells it owns after each of the m generations
// to pop[stripe * kPopGens + g], g < m, the stripe chosen by the workgroup
// index -- kPopStripes stripes of kPopGens counters, 256 B each, so that the
// tiles' atomics spread over as many cache lines (LIFE_POP_STRIPES, compile
// time, A/B: profiles/population).  launch_pop_fold, stream-ordered behind
// every launch of the pass, stores the m sums over the stripes to trace[0, m)
// and leaves all counters zero; the counters start zeroed.
constexpr int kPopGens = 32;  // generations per pass at most (launch_tstep: m <= 32)
#ifndef LIFE_POP_STRIPES
#define LIFE_POP_STRIPES 64
#endif
constexpr int kPopStripes = LIFE_POP_STRIPES;
static_assert(kPopStripes >= 1 && (kPopStripes & (kPopStripes - 1)) == 0, "stripes: a power of two");
constexpr size_t kPopCounterBytes = (size_t)kPopStripes * kPopGens * sizeof(unsigned long long);
hipError_t launch_pop_fold(unsigned long long *cnt, unsigned long long *trace, int m, hipStream_t s);
// One skip-dead pass (LIFE_OPT_SKIP_DEAD) of m generations over a single bit
// shard whose axes both wrap in the stencil (w a multiple of 64), three
// stream-ordered steps on `s`: the plan kernel classes every tile of the
// plain tile grid from `src_map` (the activity map of `in`, life_act.h) and
// the old `dst_map` (that of `out`) into cls[0, skip_tiles(L, m)) and adds
// the counts of tiles run / cleared / skipped to cnt[0..2]; dst_map is
// zeroed; the tile launch runs, clears or skips each tile and marks in
// dst_map what it stored.  `rule`: as launch_tstep.
int64_t skip_tiles(const life_layout &L, int m);  // tiles of such a pass (grows as m does)
int64_t act_map_bytes(const life_layout &L);      // one buffer's activity map
hipError_t launch_tskip(const life_layout &L, const uint8_t *in, uint8_t *out, int m, const uint32_t *src_map,
                        uint32_t *dst_map, uint8_t *cls, unsigned long long *cnt, hipStream_t s,
                        const RuleWords *rule = nullptr, unsigned long long *pop = nullptr);
// Computes (and caches) the launch-tail plans launch_tstep will use for the
// whole-shard launches of layout L at m = 1 .. mmax generations (with
// ext_y: also every deep-halo extension 0 .. K - m), so that a step call
// does not pay the planner's search (~50 us per new shape) before its first
// launch.
void prewarm_tail_plans(const life_layout &L, int mmax, bool ext_y, bool rule = false, bool rule7 = false);
// The layout a deep-halo pass tiles: h + 2 ext.y rows starting ext.y rows
// into the top apron.
life_layout extended_layout(const life_layout &L, const Extend &ext);
int temporal_rows(bool bit);      // register rows per wave: bit pair rows 16/24, byte word rows 32/48
int tile_waves(bool bit);         // waves per tile workgroup: 8
// VALU instructions the lanes at one lane position of a tile's waves issue
// for m generations (the op-count model of life_kernels.hip tstep_kernel,
// checked against the SQ_INSTS_VALU counter in profiles/); x 64 lanes x tiles.
double tstep_valu_per_tile_lane(int m, bool byte, bool rule = false, bool pop = false);
// VALU instructions per pair row and generation the census instances add
// (two v_bcnt_u32_b32, each adding to the lane's count);
// life_mi355x.POP_VALU_PER_PAIR_ROW in the binding.
constexpr int kPopValuPerPairRow = 2;
// VALU instructions per pair row and generation of the table-rule tiles
// (trule_bit_kernel): 2 v_alignbit + 4 (two full adders) + 2 x 25 (the tail);
// B3/S23: 22.  life_mi355x.RULE_VALU_PER_PAIR_ROW in the binding.
constexpr int kRuleValuPerPairRow = 56;
void set_temporal_rows(int kernel, int nr);  // kernel -1: both encodings (values valid for each)

// LDS-resident path for small single-shard grids: all `gens` generations in
// one single-workgroup launch (in -> out; in may equal out).  Usable when
// small_lds_bytes(L) <= kSmallMaxLds.
constexpr int64_t kSmallMaxLds = 160 * 1024;
int64_t small_lds_bytes(const life_layout &L);
hipError_t launch_small(const life_layout &L, const uint8_t *in, uint8_t *out, int64_t gens, hipStream_t s);
// Register-resident variant (one 1024-lane workgroup, the grid in VGPRs):
// usable when reg_small_rows(L) > 0 (at most 64 words per row and a strip
// height R from its instance list dividing h with h/R strips fitting the
// workgroup's lane groups); in != out.
int reg_small_rows(const life_layout &L);
hipError_t launch_reg_small(const life_layout &L, const uint8_t *in, uint8_t *out, int64_t gens,
                            hipStream_t s);
// Windowed register-resident variant over several CUs: ceil(h / own)
// workgroups, each holding own + 2K rows (strip height R) in VGPRs for at
// most K generations per launch; in != out.  reg_win_plan returns blocks == 0
// when the shape does not allow it.
struct RegWinPlan {
    int R, K, ns, own, blocks;
};
RegWinPlan reg_win_plan(const life_layout &L, int R, int K);
// nat_in / nat_out: the launch reads / writes natural 32-cell words instead
// of the shard's encoding (the launches inside one call; ignored, for every
// launch alike, when a row cannot hold them)
hipError_t launch_reg_win(const life_layout &L, const RegWinPlan &p, const uint8_t *in, uint8_t *out, int gens,
                          hipStream_t s, bool nat_in, bool nat_out);

}  // namespace life
