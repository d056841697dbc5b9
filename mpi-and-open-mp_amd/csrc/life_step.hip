// life_step.hip -- life_dev_step: the schedule of a step call.  Per generation
// (life_cart.c:73-74):
//   life_step     -> stencil kernel(s) cur -> nxt            (life_kernels.hip)
//   life_exchange -> the halo of the new state               (life_halo.hip)
// Overlap: the stencil is split into the boundary ring and the interior; the
// ring runs first, the halo exchange of the NEW state runs behind it while
// the interior kernel runs on the second compute stream.  Which passes a
// call runs, and which of them exchange, is life::next_pass (life_plan.cpp).
#include <chrono>
#include <utility>

#include "life_act.h"
#include "life_dev_internal.h"
#include "life_env.h"

using namespace life::rt;

// LIFE_OPT_FLOW 3 takes the dataflow form when a pass holds fewer rounds of
// resident workgroups (flow_form).
constexpr double kFlowAutoRounds = 5.0;
// fewest passes a call runs in the dataflow form
constexpr int64_t kFlowMinPasses = 4;

// LIFE_OPT_POPULATION: generations one step call may record (8 B each per shard)
constexpr int64_t kPopMaxGens = 1 << 20;

namespace {

// ---- population trace (LIFE_OPT_POPULATION)
// The census instances of the bit tiles take every pass of the call (fast
// path): the bit encoding, a temporal layout, every shard whole pairs wide (a
// narrower last pair holds apron cells, which a popcount would take for the
// shard's own).  Every other device steps one generation per launch and runs
// the census kernel behind it (step_census).
bool pop_fast(const life_dev *d) {
    if (!d->population || d->kernel != LIFE_KERNEL_BIT || !temporal(d)) return false;
    for (const Shard &s : d->shards)
        if (s.lay.w % 64 != 0) return false;
    return true;
}
// the counters the tile launches of shard s add to (null: the plain instances)
unsigned long long *pop_of(const life_dev *d, const Shard &s) { return pop_fast(d) ? s.pop_cnt : nullptr; }

// The start of a recording call: the shards' counters (zeroed, on the compute
// stream) and room for `generations` counts.
int pop_begin(life_dev *d, int64_t generations) {
    d->pop_n = d->pop_pos = 0;
    d->pop_reduced = false;
    if (!d->population) return LIFE_OK;
    if (generations > kPopMaxGens) {
        set_err("LIFE_OPT_POPULATION: a step call records at most %lld generations (%lld asked)",
                (long long)kPopMaxGens, (long long)generations);
        return LIFE_EINVAL;
    }
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        if (!s.pop_cnt) HIPCHK(hipMalloc(&s.pop_cnt, life::kPopCounterBytes));
        if ((size_t)generations > s.pop_cap) {
            if (s.pop_trace) HIPCHK(hipFree(s.pop_trace));  // (waits for the device)
            s.pop_trace = nullptr;
            s.pop_cap = 0;
            HIPCHK(hipMalloc(&s.pop_trace, (size_t)generations * sizeof(unsigned long long)));
            s.pop_cap = (size_t)generations;
        }
        HIPCHK(hipMemsetAsync(s.pop_cnt, 0, life::kPopCounterBytes, s.stream));
    }
    d->pop_n = generations;
    return LIFE_OK;
}

// Behind a pass of m generations (every stream of it joined into the compute
// stream): the counters folded into the next m entries of each shard's trace.
int pop_fold(life_dev *d, int m) {
    if (d->pop_n == 0) return LIFE_OK;
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(life::launch_pop_fold(s.pop_cnt, s.pop_trace + d->pop_pos, m, s.stream));
    }
    d->pop_pos += m;
    return LIFE_OK;
}

// Launches one stencil region on `st`; when timing is on and `timed`,
// brackets it with HIP events on that stream and books its algorithmic bytes
// (1 B read + 1 B written per BYTE cell, 2 bits per BIT cell).
int launch_region(life_dev *d, Shard &s, const life::Region &r, bool timed, hipStream_t st) {
    Bracket b;
    CHK(bracket_begin(d, s, timed, 1, kExtNever, false, st, &b));
    HIPCHK(life::launch_step(s.lay, s.buf[s.cur], s.buf[s.cur ^ 1], s.sink, r, wrap_of(d), st, rule_of(d)));
    CHK(bracket_end(b, st));
    if (b.t) {  // (no timer counts it -- span-only timing, LIFE_TIMING_MODE=3: no booking)
        const bool bit = s.lay.kernel == LIFE_KERNEL_BIT;
        const int64_t cpu = bit ? 128 : 16;
        const int64_t xa = r.u0 * cpu, xb = r.u1 * cpu < s.lay.w ? r.u1 * cpu : s.lay.w;
        book(d, bit, (double)(xb - xa) * (double)(r.r1 - r.r0), 1.0, 1.0, 0.0);
    }
    return LIFE_OK;
}

// Launches up to 4 tile regions of the temporal stencil as ONE kernel on
// `st` (m generations, cur -> nxt), optionally timed.
int launch_tiles(life_dev *d, Shard &s, const life::TileRegion *r, int nreg, int m, bool timed, hipStream_t st,
                 life::Extend xt = life::Extend{}, int64_t concurrent = 0) {
    // events stamped by the dispatch itself: no event packets between the
    // launches of a multi-stream step (kTimeCall's one pair per call is for
    // single-stream calls)
    Bracket b;
    CHK(bracket_begin(d, s, timed, 1, kExtModeExt | kExtModeCall, false, st, &b));
    double valu = 0.0;
    HIPCHK(life::launch_tstep(s.lay, s.buf[s.cur], s.buf[s.cur ^ 1], r, nreg, m, wrap_of(d), st, &valu, b.ext_a,
                              b.ext_b, xt, concurrent, rule_of(d), pop_of(d, s), rule7_tiles(d)));
    if (rule7_tiles(d)) d->last_rule7 |= LIFE_RULE7_TILES;
    CHK(bracket_end(b, st));
    if (b.t) {  // (no timer counts it -- span-only timing, LIFE_TIMING_MODE=3: no booking)
        const life::TileGeom g = life::tile_geom(life::extended_layout(s.lay, xt), m);
        double cells = 0.0;
        for (int k = 0; k < nreg; k++) {
            // owned cells only (a deep-halo pass's apron rows are not counted)
            const int64_t xa = r[k].tx0 * g.lanes * g.cells, xb = std::min(r[k].tx1 * g.lanes * g.cells, s.lay.w);
            const int64_t ya = std::max(r[k].ty0 * g.rows - xt.y, (int64_t)0),
                          yb = std::min(r[k].ty1 * g.rows - xt.y, s.lay.h);
            if (xb > xa && yb > ya) cells += (double)(xb - xa) * (double)(yb - ya);
        }
        // valu as tiled: tiles, banded items, half-height tail tiles
        book(d, s.lay.kernel == LIFE_KERNEL_BIT, cells, (double)m, 1.0, valu);
    }
    return LIFE_OK;
}

// ---- pipelined passes (LIFE_OPT_PIPELINE; the plan: life::pipe_plan)
// A whole-grid launch per pass drains the chip at every pass boundary: its
// last round leaves slots idle (the half-height tail shortens that, DESIGN.md
// 5.6) and the next launch starts with every tile loading its window at once.
// Here a pass is R launches of row regions, alternating between the shard's
// two compute streams; a region of the next pass needs only its own and the
// two neighbouring regions of this pass, and the launch order rotates by one
// region per pass, so the next pass's first region fills the slots the last
// region of this pass frees.  No launch splits its tail: each ends beside
// the next one's start.  The very last launch of a call has nothing behind
// it and stays whole as well: giving it the half-height tail measured within
// the run-to-run spread at 2, 4 and 83 passes (profiles/pipeline, lasttail).
//
// The tile grid depends on the pass length m (tile height 8R - 2m), and a
// call's passes may differ by one generation (life::next_pass): each run of
// passes of equal m is pipelined on its own, with both streams joined and
// the rotation restarted between two runs (a call has at most two).

// LIFE_OPT_PIPELINE 1, either encoding: this many regions, when every region
// holds at least kPipeAutoRounds rounds of resident workgroups and the call
// at least kPipeAutoPasses passes (profiles/pipeline).
// Measured at 65536^2 (bit 8.65 rounds per pass, byte 13.6) and 32768 x 65536
// (bit, 4.3 rounds, dataflow form off); 3 regions lose 6-8 % (every launch
// then waits for the whole pass before it, and no tail is split), 6 and 8
// are level with 4; calls of 2 to 16 passes are within their run-to-run
// spread either way (+-5 %), those of 31 and 83 passes ahead in every run.
constexpr int kPipeAutoRegions = 4;
constexpr double kPipeAutoRounds = 1.0;
constexpr int64_t kPipeAutoPasses = 4;

// the banded items' tile rows of a whole-width region (regions align on the largest)
life::BandRows tile_bands(const life::TileGeom &g) { return life::region_bands(g, g.ntx); }

// stream2 starts after everything queued on stream / stream after everything on stream2
int fence_stream2(Shard &s) {
    HIPCHK(hipEventRecord(s.ev_entry, s.stream));
    HIPCHK(hipStreamWaitEvent(s.stream2, s.ev_entry, 0));
    return LIFE_OK;
}
int join_stream2(Shard &s) {
    HIPCHK(hipEventRecord(s.ev_int, s.stream2));
    HIPCHK(hipStreamWaitEvent(s.stream, s.ev_int, 0));
    return LIFE_OK;
}

// One pass of m generations of a pipelined call on the single shard s (cur ->
// nxt; the caller flips).  Booked as ONE launch of the whole grid.
int pipelined_pass(life_dev *d, Shard &s, int m) {
    auto &pc = d->pipe_call;
    const life::TileGeom g = life::tile_geom(s.lay, m);
    if (pc.m != m) {  // a new run of equal passes
        if (pc.m != 0) {
            CHK(join_stream2(s));
            CHK(fence_stream2(s));
        }
        pc.plan = life::pipe_plan(g.nty, tile_bands(g), pc.R, 2);
        pc.m = m;
        pc.pass = 0;
    }
    const life::PipePlan &P = pc.plan;
    if (P.R == 0) {  // no plan for this tile grid: one launch, the other stream idle
        const life::TileRegion all{0, g.ntx, 0, g.nty};
        return launch_tiles(d, s, &all, 1, m, true, s.stream);
    }
    Bracket b;  // the call's pair, or none (pipe_regions: no pass of a pipelined call takes a pair of its own)
    CHK(bracket_begin(d, s, true, 1, kExtNever, false, s.stream, &b));
    hipStream_t st[2] = {s.stream, s.stream2};
    double valu = 0.0;
    for (int j = 0; j < P.R; j++) {
        const int64_t i = pc.pass * P.R + j;
        const int r = (int)((pc.pass + j) % P.R);
        hipStream_t q = st[i % 2];
        if (pc.pass > 0)
            for (int w = 0; w < P.nwait[j]; w++)
                HIPCHK(hipStreamWaitEvent(q, s.ev_pipe[(i - P.wait[j][w]) % kPipeRing], 0));
        const life::TileRegion reg{0, g.ntx, P.ty[r], P.ty[r + 1]};
        double v = 0.0;
        HIPCHK(life::launch_tstep(s.lay, s.buf[s.cur], s.buf[s.cur ^ 1], &reg, 1, m, wrap_of(d), q, &v, nullptr,
                                  nullptr, life::Extend{}, -1, rule_of(d), nullptr, rule7_tiles(d)));
        if (rule7_tiles(d)) d->last_rule7 |= LIFE_RULE7_TILES;
        valu += v;
        if (P.record[j]) HIPCHK(hipEventRecord(s.ev_pipe[i % kPipeRing], q));
    }
    CHK(bracket_end(b, s.stream));
    if (b.t) book(d, s.lay.kernel == LIFE_KERNEL_BIT, (double)s.lay.w * (double)s.lay.h, (double)m, 1.0, valu);
    pc.pass++;
    return LIFE_OK;
}

// LIFE_INTERIOR_TAIL (0/1, default 0, read once; A/B knob): 1 = the
// exchange pass's interior launch takes the banded half-height tail, planned
// with the ring's tiles counted as holding their slots; 0 = as in round 5,
// only a full-width interior (a row strip's) splits, planned alone.  Off by default: in
// r06f's ABAB loopback lines it shortened the interior by 4-9 % but the halo
// behind the ring was exposed longer by as much (the half tiles take the
// slots the RCCL kernels would get once the ring drains), so
// the block did not get shorter.
bool interior_tail() { static const bool v = life::env::read(life::env::kInteriorTail) != 0; return v; }

// The overlapped schedule of one exchange block (round 5, profiles/r05/c-d
// kernel traces): the ring tiles, then the halo of their new state (pack,
// RCCL / copies, unpack) on the compute stream `stream`, back to back in one
// hardware queue; the interior tiles concurrently on `stream2`.  The block
// ends with ONE cross-queue wait, placed on the stream whose work is
// predicted to end first: a queue that reaches a wait whose event has
// already fired passes it at once, while one that must sleep on it woke
// ~20 us after the event on MI355X (the halo's end to the next pass, r05d).
// So the work carries on in the queue predicted to finish last: the halo's
// (`stream`, which then waits for the interior) when the block is under
// three rounds of tiles -- small shards, where ring + halo outlast the
// interior (RCCL loopback, r05e: 16384x32768 1.1 rounds, 32768^2 2.2 rounds
// +8 % on the halo side; 32768x65536 4.3 rounds +1.7 % on the interior's) --
// else the interior's (`stream2` waits for the halo and the two handles are
// swapped, so `stream` always names the one that carries on).

// Phase timing of one overlapped block (timing on): ring0 before the ring
// kernels on the compute stream, ring1 after them, halo0 / halo1 around the
// halo on the same stream; the interior kernel is bracketed on the second
// compute stream; `end` after the join on the stream that carries on.
int phase_begin(life_dev *d, Shard &s, PhaseEvents **pe) {
    *pe = nullptr;
    if (!d->timing || !d->phase_events) return LIFE_OK;
    int rc;
    *pe = phase_slot(s, &rc);
    if (!*pe) return rc;
    HIPCHK(hipEventRecord((*pe)->ring0, s.stream));
    return LIFE_OK;
}
int phase_ring(Shard &s, PhaseEvents *pe) {
    if (pe) {
        HIPCHK(hipEventRecord(pe->ring1, s.stream));
        HIPCHK(hipEventRecord(pe->halo0, s.stream));
    }
    return LIFE_OK;
}
// halo_side[si]: shard si carries on in its halo's stream (see carry_on_halo_side).
int phase_end(life_dev *d, const std::vector<PhaseEvents *> &pe, const std::vector<char> &halo_side) {
    for (size_t si = 0; si < d->shards.size(); ++si) {
        Shard &s = d->shards[si];
        HIPCHK(hipSetDevice(s.device));
        if (pe[si]) HIPCHK(hipEventRecord(pe[si]->halo1, s.stream));
        if (halo_side[si]) {
            HIPCHK(hipEventRecord(s.ev_int, s.stream2));
            HIPCHK(hipStreamWaitEvent(s.stream, s.ev_int, 0));
        } else {
            HIPCHK(hipEventRecord(s.ev_halo, s.stream));
            HIPCHK(hipStreamWaitEvent(s.stream2, s.ev_halo, 0));
            std::swap(s.stream, s.stream2);
        }
        if (pe[si]) HIPCHK(hipEventRecord(pe[si]->end, s.stream));
    }
    return LIFE_OK;
}
// The rule above: ring + interior tiles under three rounds of resident
// workgroups.
bool carry_on_halo_side(int64_t block_items, int slots) {
    return slots > 0 && block_items < 3 * (int64_t)slots;
}

// One block without overlap: `all(s)` launches every cell of shard s on its
// compute stream; then the buffers flip and, when `halo`, the new state's
// halo is exchanged on the compute streams, after the launch.
template <class All>
int whole_block(life_dev *d, bool halo, All all) {
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        CHK(all(s));
    }
    for (Shard &s : d->shards) s.cur ^= 1;
    return halo ? exchange(d, 0, false) : LIFE_OK;
}

// One overlapped block (the schedule above).  ring(s) launches the boundary
// ring of shard s on s.stream (untimed: the phase events cover it);
// interior(s, &halo_side) launches the interior on s.stream2 and may choose
// to carry on in the halo's stream (default: the interior's).
template <class Ring, class Interior>
int overlapped_block(life_dev *d, Ring ring, Interior interior) {
    std::vector<PhaseEvents *> pe(d->shards.size(), nullptr);
    std::vector<char> halo_side(d->shards.size(), 0);
    for (size_t si = 0; si < d->shards.size(); ++si) {
        Shard &s = d->shards[si];
        HIPCHK(hipSetDevice(s.device));
        // The interior (second stream) starts after everything on the compute
        // stream: phase_end joined the previous block into ONE stream
        // only (and may have swapped the handles), so without this fence the
        // next interior could start beside the previous interior (still
        // reading cur) or beside the previous ring + halo; a
        // deep-halo pass before this one is not joined into the other
        // streams either.
        HIPCHK(hipEventRecord(s.ev_entry, s.stream));
        HIPCHK(hipStreamWaitEvent(s.stream2, s.ev_entry, 0));
        CHK(phase_begin(d, s, &pe[si]));
        CHK(ring(s));
        CHK(phase_ring(s, pe[si]));
        if (pe[si]) HIPCHK(hipEventRecord(pe[si]->int0, s.stream2));
        CHK(interior(s, &halo_side[si]));
        if (pe[si]) HIPCHK(hipEventRecord(pe[si]->int1, s.stream2));
    }
    CHK(exchange(d, 1, false));  // halo of nxt, behind the ring on the compute streams
    CHK(phase_end(d, pe, halo_side));
    for (Shard &s : d->shards) s.cur ^= 1;
    return LIFE_OK;
}

// One pass (life::next_pass) of the temporally blocked stencil on every
// shard: m <= K generations, then one K-deep halo exchange.  Partitioned
// shards: the boundary ring (one multi-region launch) runs on the compute
// stream, the exchange of its new state behind it, and the interior
// concurrently on the second compute stream.  The ring holds every tile that
// produces a cell the exchange sends: rows [0, K) and [h-K, h), columns
// [0, xa) and [w-xa, w) (xa = the x-apron, one lane column).  A self-wrapped
// x axis (life::self_wrap_x) counts as partitioned: its "exchange" is the
// column copy.
int generation_block(life_dev *d, const life::PassPlan &p) {
    const bool rx = part(d, 0) || self_wrap_x(d), ry = part(d, 1);
    const int m = p.m;
    // Deep halo (bit tiles, partitioned axes, no self-wrapped x): the
    // exchange of a K-deep halo is skipped while the aprons still hold the
    // next pass's ghost cells -- this pass then also advances the apron cells
    // the next one reads (life::Extend) -- and runs after the pass whose
    // successor would outrun them.  A 20-generation call of two 10-generation
    // passes exchanges once instead of twice (life_cart.c:73-74 exchanges
    // every generation).
    // next_pass cuts a call into passes that end on the K boundary, so the
    // exchange runs (overlapped with this pass) when the aprons are used up,
    // or at the call's end when the next call's first pass could not fit.
    if (p.refill_first) CHK(exchange(d, 0, false));
    if (p.extend) {
        life::Extend xt;
        xt.y = ry ? p.ext : 0;
        xt.x = part(d, 0);
        CHK(whole_block(d, false, [&](Shard &s) -> int {
            const life::TileGeom g = life::tile_geom(life::extended_layout(s.lay, xt), m);
            const life::TileRegion all{0, g.ntx, 0, g.nty};
            return launch_tiles(d, s, &all, 1, m, true, s.stream, xt);
        }));
        d->since += m;
        return LIFE_OK;
    }
    if (!(rx || ry) || !d->overlap)
        // one launch of every tile; a partitioned shard without overlap
        // (LIFE_OPT_OVERLAP 0) then exchanges its halo on the compute
        // stream, after the launch
        return whole_block(d, rx || ry, [&](Shard &s) -> int {
            if (d->pipe_call.R > 0) return pipelined_pass(d, s, m);
            const life::TileGeom g = life::tile_geom(s.lay, m);
            const life::TileRegion all{0, g.ntx, 0, g.nty};
            return launch_tiles(d, s, &all, 1, m, true, s.stream);
        });
    // per shard: the ring's regions (ring) and the interior, set by the ring
    // callable for the interior one that follows it
    life::TileGeom g;
    life::TileRegion ring[4], inner;
    int n = 0;
    return overlapped_block(
        d,
        [&](Shard &s) -> int {
            const int64_t K = s.lay.generations_per_exchange;
            // grid of tiles: NX x NY, tile height uh; tile columns [0, ca) and
            // [cb, NX) hold the x-ring
            g = life::tile_geom(s.lay, m);
            const int64_t NX = g.ntx, NY = g.nty, uh = g.rows;
            int64_t ca = 0, cb = NX;
            if (rx) {  // the x-ring: tile columns holding cells [0, xa) and [w - xa, w)
                ca = 1;
                cb = std::max(std::min(((s.lay.w - s.lay.xapron) / g.cells) / g.lanes, NX), ca);
            }
            // unit rows [0, ra) and [rb, NY), unit columns [0, ca) and [cb, NX)
            int64_t ra = 0, rb = NY;
            if (ry) {
                ra = std::min((K + uh - 1) / uh, NY);
                rb = std::max(std::min((s.lay.h - K) / uh, NY), ra);
            }
            n = 0;
            if (ra > 0) ring[n++] = life::TileRegion{0, NX, 0, ra};
            if (rb < NY) ring[n++] = life::TileRegion{0, NX, rb, NY};
            if (rb > ra) {
                if (ca > 0) ring[n++] = life::TileRegion{0, ca, ra, rb};
                if (cb < NX) ring[n++] = life::TileRegion{cb, NX, ra, rb};
            }
            inner = life::TileRegion{ca, cb, ra, rb};
            return launch_tiles(d, s, ring, n, m, false, s.stream);
        },
        [&](Shard &s, char *halo_side) -> int {
            int64_t ring_items = 0;
            for (int k = 0; k < n; k++) ring_items += life::region_items(g, ring[k]);
            const int64_t items = life::region_items(g, inner) + ring_items;
            *halo_side = carry_on_halo_side(items, life::tile_slots(s.lay, d->table, rule7_tiles(d))) ? 1 : 0;
            // LIFE_INTERIOR_TAIL=1: the interior's launch-tail plan counts the
            // ring's tiles, dispatched just before it, as holding their slots
            // (16384 x 32768's 584 interior tiles beside 249 ring tiles are one
            // round plus a tail); default: only a row strip's full-width interior
            // splits its tail, planned alone (round 5)
            const int64_t conc = interior_tail() ? ring_items : (inner.tx0 == 0 && inner.tx1 == g.ntx ? 0 : -1);
            if (inner.ty1 > inner.ty0 && inner.tx1 > inner.tx0)
                return launch_tiles(d, s, &inner, 1, m, true, s.stream2, life::Extend{}, conc);
            return LIFE_OK;
        });
}

// One generation on every local shard (one-cell aprons).
int generation(life_dev *d) {
    const bool rx = part(d, 0), ry = part(d, 1);
    if (!d->overlap || !(rx || ry))
        return whole_block(d, true, [&](Shard &s) -> int {
            return launch_region(d, s, life::Region{0, s.lay.units, 0, s.lay.h}, true, s.stream);
        });
    // Ring first (cells whose 3x3 neighbourhood reaches a partitioned axis'
    // apron) on the compute stream, then the halo of the new state behind it;
    // the interior runs concurrently on the second compute stream.
    // One-generation launches are short: carry on in the interior's stream.
    auto interior_rows = [&](const Shard &s, int64_t *ra, int64_t *rb) {
        *ra = ry ? 1 : 0;
        *rb = ry ? s.lay.h - 1 : s.lay.h;
    };
    return overlapped_block(
        d,
        [&](Shard &s) -> int {
            const int64_t U = s.lay.units, H = s.lay.h;
            int64_t ra, rb;
            interior_rows(s, &ra, &rb);
            if (ry) {
                CHK(launch_region(d, s, life::Region{0, U, 0, 1}, false, s.stream));
                if (H > 1) CHK(launch_region(d, s, life::Region{0, U, H - 1, H}, false, s.stream));
            }
            if (rx && rb > ra) {
                CHK(launch_region(d, s, life::Region{0, 1, ra, rb}, false, s.stream));
                if (U > 1) CHK(launch_region(d, s, life::Region{U - 1, U, ra, rb}, false, s.stream));
            }
            return LIFE_OK;
        },
        [&](Shard &s, char *) -> int {
            const int64_t U = s.lay.units;
            int64_t ra, rb;
            interior_rows(s, &ra, &rb);
            const int64_t ua = rx ? 1 : 0, ub = rx ? U - 1 : U;
            if (rb > ra && ub > ua) return launch_region(d, s, life::Region{ua, ub, ra, rb}, true, s.stream2);
            return LIFE_OK;
        });
}

// A single-shard grid small enough for one CU's LDS runs every generation of
// the call in one resident-workgroup launch (life_kernels.hip, small_kernel).
// Mode 1 (default) windows the VGPR kernel over several CUs when one
// workgroup would need strips of 4 rows or more (p46gun_big 500^2: 10 rows,
// 212 -> 632 Gcell/s windowed); mode 3 windows whenever the shape allows.
life::RegWinPlan win_plan(const life_dev *d) {
    const life_layout &L = d->shards[0].lay;
    if (d->small_mode == 3 || (d->small_mode == 1 && life::reg_small_rows(L) >= 4))
        return life::reg_win_plan(L, d->win_rows, d->win_halo);
    return life::RegWinPlan{};
}

bool small_grid(const life_dev *d) {
    // (the resident kernels are B3/S23 only: under another rule the streaming kernels run; they record
    // no population either)
    if (d->population) return false;
    if (d->world != 1 || d->shards.size() != 1 || d->small_mode == 0 || d->loop != 0 || d->table) return false;
    const life_layout &L = d->shards[0].lay;
    if (win_plan(d).blocks > 0) return true;
    return (d->small_mode != 2 && life::reg_small_rows(L) > 0) ||
           life::small_lds_bytes(L) <= life::kSmallMaxLds;
}

int step_small(life_dev *d, int64_t generations) {
    Shard &s = d->shards[0];
    HIPCHK(hipSetDevice(s.device));
    // ONE event pair around the call's launches: events between the
    // windowed kernel's ~9 us launches measured 45 % slower (gaps)
    Bracket b;
    CHK(bracket_begin(d, s, true, 1, kExtNever, true, s.stream, &b));
    const life::RegWinPlan wp = win_plan(d);
    int launches = 1;
    if (wp.blocks > 0) {
        // K generations per launch, buffers swapped per launch; between the
        // launches of the call the grid stays in natural 32-cell words
        launches = 0;
        for (int64_t g = 0; g < generations; g += wp.K, ++launches) {
            const int m = (int)(generations - g < wp.K ? generations - g : wp.K);
            HIPCHK(life::launch_reg_win(s.lay, wp, s.buf[s.cur], s.buf[s.cur ^ 1], m, s.stream, g > 0,
                                        g + m < generations));
            s.cur ^= 1;
        }
    } else {
        if (d->small_mode != 2 && life::reg_small_rows(s.lay) > 0)
            HIPCHK(life::launch_reg_small(s.lay, s.buf[s.cur], s.buf[s.cur ^ 1], generations, s.stream));
        else
            HIPCHK(life::launch_small(s.lay, s.buf[s.cur], s.buf[s.cur ^ 1], generations, s.stream));
        s.cur ^= 1;
    }
    CHK(bracket_end(b, s.stream));
    if (b.t) {
        b.t->launches = launches;  // stats: mean per launch
        // CU-resident: HBM sees one import and one export of the grid per launch
        book(d, s.lay.kernel == LIFE_KERNEL_BIT, (double)s.lay.w * (double)s.lay.h, (double)generations,
             (double)launches, 0.0);
    }
    return LIFE_OK;
}

// The dataflow form a single-shard bit device runs its passes of m
// generations in (1 / 2, the hand-off forms), or 0 (per-launch tiles; always
// under a rule other than B3/S23: the dataflow tiles have no such instance).
int flow_form(const life_dev *d, int *m_out) {
    if (!d->flow || d->table || d->population || d->shards.size() != 1 || d->world != 1 || part(d, 0) || part(d, 1) || self_wrap_x(d) ||
        d->kernel != LIFE_KERNEL_BIT)
        return 0;
    const life_layout &L = d->shards[0].lay;
    const int m = max_pass_gens(d);
    *m_out = m;
    if (!life::flow_ok(L, m)) return 0;
    // automatic: the dataflow form (write-through hand-off) when a pass is
    // under kFlowAutoRounds rounds of resident workgroups -- 32768^2 (2.2
    // rounds of 768) +8 %, 32768 x 65536 (4.3) +1 %, 65536^2 (8.6) -3 %
    // (profiles/r05/a) -- except a pass of 1 to 1.5 rounds: it runs as one
    // full round plus the banded half-height tail (launch_tstep), its tiles
    // all finish together and the dataflow form has nothing to pipeline
    // (16384 x 32768, 833 tiles on 768 slots: per-launch tiles 83.2-83.8 T
    // against 73.7-75.2 T, profiles/r06/d; under one round the dataflow
    // form overlaps the passes in the idle slots)
    if (d->flow == 3) {
        const double rounds =
            (double)life::flow_items_per_pass(L, m) / (double)std::max(life::flow_slots(L, rule7_flow(d)), 1);
        return rounds < kFlowAutoRounds && !(rounds >= 1.0 && rounds < 1.5) ? 1 : 0;
    }
    return d->flow;
}

// Grows the shard's dataflow scratch (queue head, error word, per-tile pass
// counts) to the tile grid of m generations per pass.
int flow_scratch(Shard &s, int m) {
    const life::TileGeom g = life::tile_geom(s.lay, m);
    const size_t words = (size_t)(2 + g.ntx * g.nty);
    if (words <= s.flow_words) return LIFE_OK;
    if (s.flow) (void)hipFree(s.flow);
    s.flow = nullptr;
    s.flow_words = 0;
    if (hipSetDevice(s.device) != hipSuccess || hipMalloc(&s.flow, words * sizeof(unsigned int)) != hipSuccess ||
        hipMemsetAsync(s.flow, 0, 2 * sizeof(unsigned int), s.stream) != hipSuccess) {
        set_err("dataflow scratch (%zu words)", words);
        return LIFE_ENOMEM;
    }
    s.flow_words = words;
    return LIFE_OK;
}

// The whole passes of a step call of `generations` the dataflow form takes
// (0: none, the call runs per-launch tiles), in form *form, of *m generations
// each, at most *per of them per launch.
int64_t flow_passes(const life_dev *d, int64_t generations, int *form, int *m, int64_t *per) {
    *form = flow_form(d, m);
    if (*form == 0) return 0;
    const life_layout &L = d->shards[0].lay;
    const int64_t passes = generations / *m;
    // a call of 2-3 passes ran 0.58 ms per 10-generation pass against 0.42 for
    // the per-launch tiles (profiles/r03/r4d); the dataflow form pays from
    // about 4 passes (0.474 ms per 12-generation pass in long runs)
    if (passes < kFlowMinPasses) return 0;
    // The queue head is a 32-bit counter every resident workgroup bumps once
    // past the last item: split the passes so that items + grid stays below
    // 2^31 per launch (life::flow_chunk_passes), flipping the buffer parity
    // per chunk.
    *per = life::flow_chunk_passes(life::flow_items_per_pass(L, *m), life::flow_slots(L, rule7_flow(d)),
                                   d->flow_chunk);
    return *per < 1 ? 0 : passes;  // a grid too large for one pass per launch: per-launch tiles
}

// Whole passes of the dataflow tiles (life::launch_tflow) for a step call of
// `generations` on a single shard whose axes both wrap in the stencil;
// *done = the generations it queued (a multiple of the pass size m), 0 when
// the call takes the per-launch path.
int step_flow(life_dev *d, int64_t generations, int64_t *done) {
    *done = 0;
    int m = 0, form = 0;
    int64_t per = 0;
    const int64_t passes = flow_passes(d, generations, &form, &m, &per);
    if (passes == 0) return LIFE_OK;
    Shard &s = d->shards[0];
    const life_layout &L = s.lay;
    CHK(flow_scratch(s, m));
    HIPCHK(hipSetDevice(s.device));
    for (int64_t left = passes; left > 0;) {
        const int64_t n = std::min(left, per);
        Bracket b;
        CHK(bracket_begin(d, s, true, (int)n, kExtModeExt, false, s.stream, &b));  // stats: mean per pass
        HIPCHK(life::launch_tflow(L, s.buf[s.cur], s.buf[s.cur ^ 1], m, n, s.flow, s.flow + 2, wrap_of(d),
                                  form, s.stream, b.ext_a, b.ext_b, rule7_flow(d)));
        if (rule7_flow(d)) d->last_rule7 |= LIFE_RULE7_FLOW;
        CHK(bracket_end(b, s.stream));
        // work is booked only beside a timer that counts the launch (as
        // launch_tiles / launch_region: LIFE_TIMING_MODE=3 and span-only
        // timing book nothing, so bytes / updates per launch stay consistent)
        if (b.t)
            book(d, true, (double)L.w * (double)L.h, (double)n * (double)m, (double)n,
                 (double)n * (double)life::flow_items_per_pass(L, m, true) * 64.0 *
                     life::tstep_valu_per_tile_lane(m, false));
        if (n & 1) s.cur ^= 1;
        left -= n;
    }
    s.flow_used = true;
    *done = passes * m;
    return LIFE_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
void note_pass(life_dev *d, std::chrono::steady_clock::time_point t0) {
    const double ms = ms_since(t0);
    d->call_passes++;
    if (ms > d->call_pass_max_ms) d->call_pass_max_ms = ms;
}

// ---- skip-dead passes (LIFE_OPT_SKIP_DEAD; DESIGN.md 5.9, life_act.h)
// The device runs its passes this way: the option on, a single shard in a
// single process, both axes wrapped by the stencil (so w % 64 == 0), the bit
// encoding, a temporal layout, not the small-grid path.  Any rule
// life_dev_set_rule accepts (none is B0).
bool skip_dead_applies(const life_dev *d) {
    return d->skip_dead && d->shards.size() == 1 && d->world == 1 && !part(d, 0) && !part(d, 1) && !self_wrap_x(d) &&
           d->kernel == LIFE_KERNEL_BIT && temporal(d) && !small_grid(d);
}

// The shard's maps and counters (once), and room for the classes of `tiles` tiles.
int act_scratch(Shard &s, int64_t tiles) {
    const size_t bytes = (size_t)life::act_map_bytes(s.lay);
    if (!s.act_map[0]) {
        HIPCHK(hipMalloc(&s.act_map[0], 2 * bytes));
        s.act_map[1] = s.act_map[0] + bytes / sizeof(uint32_t);
    }
    if (!s.act_cnt) HIPCHK(hipMalloc(&s.act_cnt, 3 * sizeof(unsigned long long)));
    if ((size_t)tiles > s.act_cls_cap) {
        if (s.act_cls) HIPCHK(hipFree(s.act_cls));  // (waits for the device: no queued pass still reads it)
        s.act_cls = nullptr;
        s.act_cls_cap = 0;
        HIPCHK(hipMalloc(&s.act_cls, (size_t)tiles));
        s.act_cls_cap = (size_t)tiles;
    }
    return LIFE_OK;
}

// A step call of skip-dead passes on the single shard, all on its compute
// stream; nothing is read back and nothing waited for.  Invalid maps (an
// edit, a pass of another form or the option switched on since the last such
// pass) are rebuilt first: one streaming scan of the current buffer, and all
// ones for the other one, whose content is unknown (0xA5 on a fresh device
// under LIFE_POISON=1), so the first pass clears whatever it does not run.
int step_skip(life_dev *d, int64_t generations) {
    Shard &s = d->shards[0];
    const life_layout &L = s.lay;
    HIPCHK(hipSetDevice(s.device));
    const int K = L.generations_per_exchange, bmax = max_pass_gens(d);
    CHK(act_scratch(s, life::skip_tiles(L, bmax)));  // the shortest tiles of the call: the most
    HIPCHK(hipMemsetAsync(s.act_cnt, 0, 3 * sizeof(unsigned long long), s.stream));
    if (!d->act_valid) {
        HIPCHK(life::launch_act_scan(L, s.buf[s.cur], s.act_map[s.cur], s.stream));
        HIPCHK(hipMemsetAsync(s.act_map[s.cur ^ 1], 0xFF, (size_t)life::act_map_bytes(L), s.stream));
        d->act_valid = true;
    }
    d->last_path = LIFE_PATH_SKIP;
    for (int64_t g = 0; g < generations;) {
        const life::PassPlan p = life::next_pass(K, bmax, false, d->since, generations - g);
        const auto t0 = std::chrono::steady_clock::now();
        // one timed launch: the plan, the map clear and the tiles under one
        // bracket; the whole grid's cell-updates, but no bytes and no VALU ops
        // (the host does not know how many tiles ran: life_dev_activity)
        Bracket b;
        CHK(bracket_begin(d, s, true, 1, kExtNever, false, s.stream, &b));
        HIPCHK(life::launch_tskip(L, s.buf[s.cur], s.buf[s.cur ^ 1], p.m, s.act_map[s.cur], s.act_map[s.cur ^ 1],
                                  s.act_cls, s.act_cnt, s.stream, rule_of(d), pop_of(d, s)));
        CHK(bracket_end(b, s.stream));
        CHK(pop_fold(d, p.m));  // (outside the bracket: the pass stays one timed launch)
        if (b.t) book(d, true, (double)L.w * (double)L.h, (double)p.m, 0.0, 0.0);
        s.cur ^= 1;
        d->act_passes++;
        d->act_total += life::skip_tiles(L, p.m);
        note_pass(d, t0);
        g += p.m;
    }
    return LIFE_OK;
}

// A recording call of a device the census tiles do not take (pop_fast): one
// generation per launch, the census kernel behind each on the compute stream
// (count and checksum land in the first two counters; the fold stores the
// count and zeroes both).  Nothing is read back.
int step_census(life_dev *d, int64_t generations) {
    const bool tiles = temporal(d);
    d->last_path = tiles ? LIFE_PATH_TILES : LIFE_PATH_ONEGEN;
    const int K = d->shards[0].lay.generations_per_exchange;
    for (int64_t g = 0; g < generations; g++) {
        const auto t0 = std::chrono::steady_clock::now();
        if (tiles)
            CHK(generation_block(d, life::next_pass(K, max_pass_gens(d), deep_halo(d), d->since, 1)));
        else
            CHK(generation(d));
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            HIPCHK(life::launch_census(s.lay, d->nx, s.buf[s.cur], s.pop_cnt, s.stream));
        }
        CHK(pop_fold(d, 1));
        note_pass(d, t0);
    }
    return LIFE_OK;
}

// The launches of one step call (life_dev_step after its entry fence).
int step_body(life_dev *d, int64_t generations) {
    CHK(pop_begin(d, generations));
    if (skip_dead_applies(d)) return step_skip(d, generations);
    d->act_valid = false;  // a pass of any other form leaves the activity maps behind
    if (d->population && !pop_fast(d)) return step_census(d, generations);
    if (small_grid(d)) {
        d->last_path = LIFE_PATH_SMALL;
        constexpr int64_t kChunk = 1 << 20;  // generations per resident launch
        for (int64_t g = 0; g < generations; g += kChunk)
            CHK(step_small(d, generations - g < kChunk ? generations - g : kChunk));
        // the LDS kernel wraps inside the CU and leaves the buffer's aprons
        // stale: refresh them (a self-wrapped x axis; no-op otherwise)
        return exchange(d, 0, false);
    }
    if (temporal(d)) {
        int64_t done = 0;
        CHK(step_flow(d, generations, &done));
        d->last_path = done > 0 ? LIFE_PATH_FLOW : LIFE_PATH_TILES;
        const int K = d->shards[0].lay.generations_per_exchange;
        for (int64_t g = done; g < generations;) {
            const life::PassPlan p = life::next_pass(K, max_pass_gens(d), deep_halo(d), d->since, generations - g);
            const auto t0 = std::chrono::steady_clock::now();
            CHK(generation_block(d, p));
            CHK(pop_fold(d, p.m));
            note_pass(d, t0);
            g += p.m;
        }
        return LIFE_OK;
    }
    d->last_path = LIFE_PATH_ONEGEN;
    for (int64_t g = 0; g < generations; g++) {
        const auto t0 = std::chrono::steady_clock::now();
        CHK(generation(d));
        note_pass(d, t0);
    }
    return LIFE_OK;
}

// The row regions per pass this step call pipelines its per-launch tile
// passes in (pipelined_pass), 0 when it does not: LIFE_OPT_PIPELINE off; not
// a single shard wrapping both axes in the stencil; a small-grid or
// one-generation call; timing that gives every launch its own event pair or
// dispatch stamps (overlapping kernels have no time of their own; the call's
// one pair, span-only timing and no timing pipeline); fewer than 2 passes
// behind the dataflow form's share; no plan for the first pass's tile grid.
int pipe_regions(const life_dev *d, int64_t generations) {
    // (a recording call runs one launch per pass: pipelined passes overlap in time and would need a
    // counter set per pass in flight)
    if (d->pipe == 0 || d->population || d->shards.size() != 1 || d->world != 1 || part(d, 0) || part(d, 1) || self_wrap_x(d) ||
        !temporal(d) || small_grid(d) || skip_dead_applies(d))  // (skip-dead passes run whole, on one stream)
        return 0;
    if (d->timing && d->launch_events && timing_mode() != kTimeCall && timing_mode() != kTimeOff) return 0;
    int form = 0, fm = 0;
    int64_t per = 0;
    const int64_t rest = generations - flow_passes(d, generations, &form, &fm, &per) * fm;
    const int bmax = max_pass_gens(d);
    const int64_t passes = (rest + bmax - 1) / bmax;
    if (passes < 2) return 0;
    const life_layout &L = d->shards[0].lay;
    const life::TileGeom g = life::tile_geom(L, (int)((rest + passes - 1) / passes));
    int R = d->pipe;
    if (R == 1) {
        R = kPipeAutoRegions;
        const int slots = life::tile_slots(L, d->table, rule7_tiles(d));
        if (passes < kPipeAutoPasses || slots < 1 ||
            (double)life::region_items(g, life::TileRegion{0, g.ntx, 0, g.nty}) < kPipeAutoRounds * R * slots)
            return 0;
    }
    return life::pipe_plan(g.nty, tile_bands(g), R, 2).R;
}

// step_body, then the second compute stream of a pipelined call joined back
// into the first: what follows the call there (its closing event, the
// census, a gather, fill_random, the next call) stays ordered behind it.
int call_body(life_dev *d, int64_t generations) {
    const int rc = step_body(d, generations);
    const bool piped = d->pipe_call.R > 0;
    d->pipe_call.R = 0;
    if (rc == LIFE_OK && piped) CHK(join_stream2(d->shards[0]));
    return rc;
}

int step_call(life_dev *d, int64_t generations) {
    // Entry fence: the second compute stream and the comm stream start after
    // everything already queued on the compute stream (an asynchronous
    // fill_random and its halo fill, a small-grid launch, a gather's export),
    // which the overlapped schedule would otherwise race.  A single shard
    // with no partitioned or self-wrapped axis steps on the compute stream
    // alone: no fence (4 runtime calls off a ~1 ms call's critical path).
    // A pipelined call of such a shard uses the second compute stream too:
    // it is fenced here and joined back at the end (call_body), and is as good
    // as one stream to what brackets the call.
    const bool one_stream = d->shards.size() == 1 && !part(d, 0) && !part(d, 1) && !self_wrap_x(d);
    d->pipe_call.R = 0;
    if (one_stream) {
        HIPCHK(hipSetDevice(d->shards[0].device));
        d->pipe_call.R = pipe_regions(d, generations);
        d->pipe_call.m = 0;
        if (d->pipe_call.R > 0) CHK(fence_stream2(d->shards[0]));
    }
    for (Shard &s : d->shards) {
        if (one_stream) break;
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipEventRecord(s.ev_entry, s.stream));
        HIPCHK(hipStreamWaitEvent(s.stream2, s.ev_entry, 0));
        HIPCHK(hipStreamWaitEvent(s.comm_stream, s.ev_entry, 0));
    }
    // kTimeCall: one event pair around all launches of a single-stream call
    if (d->timing && one_stream && timing_mode() == kTimeCall && !small_grid(d) && temporal(d)) {
        Shard &s = d->shards[0];
        int rc;
        d->call_timer = timer_slot(s, &rc);
        if (!d->call_timer) return rc;
        d->call_timer->launches = 0;
        HIPCHK(hipEventRecord(d->call_timer->a, s.stream));
        rc = call_body(d, generations);
        TimedLaunch *t = d->call_timer;
        d->call_timer = nullptr;
        if (rc != LIFE_OK) {
            // drop the half-recorded pair (no event b): a later harvest
            // would fail on it and hide this call's error
            s.timers_used--;
            return rc;
        }
        HIPCHK(hipEventRecord(t->b, s.stream));
        s.span_a = t->a;  // the call's pair is its span
        s.span_b = t->b;
        d->call_spans = true;
        return LIFE_OK;
    }
    if (!d->timing) return call_body(d, generations);
    // timing on, any other call: one event at each end of the call on every
    // shard's compute stream (the entry fence above orders the other streams
    // after the first; every schedule joins them back into it at the end)
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        if (!s.own_a) HIPCHK(hipEventCreate(&s.own_a));
        if (!s.own_b) HIPCHK(hipEventCreate(&s.own_b));
        HIPCHK(hipEventRecord(s.own_a, s.stream));
    }
    CHK(call_body(d, generations));
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipEventRecord(s.own_b, s.stream));
        s.span_a = s.own_a;
        s.span_b = s.own_b;
    }
    d->call_spans = true;
    return LIFE_OK;
}

}  // namespace

// At creation: the scratch and one empty launch of the dataflow instance the
// device's first dataflow call will run, so that call does not pay the
// kernel's first launch (~140 us before configs[2]'s dataflow launch inside
// its timed call, profiles/r05/l trace_32768).
int life::rt::flow_prewarm(life_dev *d) {
    int m = 0;
    const int form = flow_form(d, &m);
    if (form == 0) return LIFE_OK;
    Shard &s = d->shards[0];
    CHK(flow_scratch(s, m));
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(life::prewarm_tflow(s.lay, m, form, s.flow, s.stream, rule7_flow(d)));
    HIPCHK(hipStreamSynchronize(s.stream));
    return LIFE_OK;
}

extern "C" {

int life_dev_step(life_dev *d, int64_t generations) {
    if (!d || generations < 0) return LIFE_EINVAL;
    if (generations == 0) {
        d->pop_n = d->pop_pos = 0;  // the last call recorded nothing
        return LIFE_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    d->call_passes = 0;
    d->call_pass_max_ms = 0.0;
    d->call_spans = false;
    d->act_passes = d->act_total = 0;
    d->last_rule7 = 0;
    const int rc = step_call(d, generations);
    d->call_host_ms = ms_since(t0);
    return rc;
}

int life_dev_last_path(life_dev *d) { return d ? d->last_path : LIFE_EINVAL; }

int life_dev_last_rule_arm(life_dev *d) { return d ? d->last_rule7 : LIFE_EINVAL; }

int life_dev_population(life_dev *d, int64_t *counts, int64_t max, int64_t *generations) {
    if (!d || max < 0 || (!counts && max > 0)) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    // a call that failed half way recorded pop_pos < pop_n generations
    const int64_t n = std::min(d->pop_n, d->pop_pos);
    if (generations) *generations = n;
    const int64_t take = std::min(n, max);
    if (take <= 0) return LIFE_OK;
    std::vector<unsigned long long> h((size_t)take);
    std::fill(counts, counts + take, (int64_t)0);
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        // rank mode: every rank's shard summed into every rank's trace, once (the census's all-reduce;
        // never executed with world > 1: one-GPU boxes)
        if (d->rank_mode && s.comm && !d->pop_reduced)
            NCCLCHK(ncclAllReduce(s.pop_trace, s.pop_trace, (size_t)n, ncclUint64, ncclSum, s.comm, s.stream));
        HIPCHK(hipMemcpyAsync(h.data(), s.pop_trace, (size_t)take * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              s.stream));
        CHK(bounded_sync(s, "population all-reduce", -1));
        for (int64_t g = 0; g < take; g++) counts[g] += (int64_t)h[(size_t)g];
    }
    d->pop_reduced = true;
    return LIFE_OK;
}

int life_dev_activity(life_dev *d, int64_t *passes, int64_t *tiles_run, int64_t *tiles_cleared, int64_t *tiles_total) {
    if (!d) return LIFE_EINVAL;
    unsigned long long cnt[3] = {0, 0, 0};
    if (d->act_passes > 0) {
        CHK(life_dev_sync(d));
        Shard &s = d->shards[0];
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipMemcpyAsync(cnt, s.act_cnt, sizeof cnt, hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    if (passes) *passes = d->act_passes;
    if (tiles_run) *tiles_run = (int64_t)cnt[0];
    if (tiles_cleared) *tiles_cleared = (int64_t)cnt[1];
    if (tiles_total) *tiles_total = d->act_total;
    return LIFE_OK;
}

}  // extern "C"
