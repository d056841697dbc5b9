// life_batch_kernels.h -- launchers of the batch unit (life_batch_kernels.hip):
// the two stencil tiers of life_batch_step and the batch's data movement.
// Every launcher is asynchronous on `s`.  `cells` is the batch storage of
// life::BatchPlan: universe u starts p.bytes * u bytes in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "life_host.h"

#pragma GCC visibility push(hidden)

namespace life {

// Wave tier: `gens` >= 1 generations of universes [0, count).  rule null:
// B3/S23.  settle: the detection of LIFE_BATCH_OPT_SETTLE, with settled[u] the
// universe's flag (-1, or the generation it settled at) and gen0 the batch's
// generation before this call; off, `settled` is not touched.
hipError_t launch_batch_wave(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                             const RuleWords *rule, bool settle, int64_t *settled, int64_t gen0, hipStream_t s);
// The survey forms of the wave tier, kernels of their own
// beside the uniform ones above.  rules non-null: a rule per universe, (birth,
// survive) pairs of 32-bit masks, universe u's at rules[2 u]; the wave expands
// its own into the table tail (`rule` is then ignored).  cycle: the detection
// of LIFE_BATCH_OPT_CYCLE with period[u] / found[u] the universe's pair (0 /
// -1, or the period and the generation it was found at); never with settle.
// One of rules and cycle must be set: the rest is launch_batch_wave's.
hipError_t launch_batch_survey(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                               const RuleWords *rule, const uint32_t *rules, bool settle, int64_t *settled, bool cycle,
                               int64_t *period, int64_t *found, int64_t gen0, hipStream_t s);
// Generations on the wave tier, a kernel family of its own:
// `decay` holds `planes` (1, 2 or 4) bit planes of d = s - 1 of the dying
// cells, each count * ny * p.words words, plane-major, beside the alive plane
// `cells`.  rules null: the uniform (birth, survive, states); else the table
// of life_batch_set_rules_gen, universe u's (birth | states << 16, survive) at
// rules[2 u], and every state count must fit `planes` (life::gen_planes).  The
// detectors are launch_batch_survey's, comparing every plane.
hipError_t launch_batch_gen(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, uint32_t *decay,
                            int planes, int64_t gens, uint32_t birth, uint32_t survive, uint32_t states,
                            const uint32_t *rules, bool settle, int64_t *settled, bool cycle, int64_t *period,
                            int64_t *found, int64_t gen0, hipStream_t s);
// Group tier (B3/S23): one workgroup per universe.
hipError_t launch_batch_group(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells,
                              int64_t gens, hipStream_t s);
// The recording forms of LIFE_BATCH_OPT_POPULATION, kernels of
// their own beside the ones above: the same call, and trace[u * gens + g] = the
// live cells of universe u after generation g + 1 of it, for every universe
// and generation whatever a detector does (the wave runs on).  `trace` holds
// count * gens entries, at most kBatchTraceEntries.  launch_batch_trace serves
// every two-state form of the wave tier (arguments as launch_batch_survey, but
// rules and cycle may both be unset), launch_batch_group_trace the group tier.
constexpr int64_t kBatchTraceEntries = (int64_t)1 << 30;
hipError_t launch_batch_trace(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                              const RuleWords *rule, const uint32_t *rules, bool settle, int64_t *settled, bool cycle,
                              int64_t *period, int64_t *found, int64_t gen0, uint32_t *trace, hipStream_t s);
hipError_t launch_batch_group_trace(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells,
                                    int64_t gens, uint32_t *trace, hipStream_t s);
// The onset forms of LIFE_BATCH_OPT_ONSET, kernels of their own
// again: cycle detection as above and, in the wave that finds a period, Brent's
// second phase from the universe's stored start state; onset[u] (-1 until
// then) becomes gen0 + min { m : S_m == S_(m+period) }.  launch_batch_onset
// serves the two-state forms (rule, rules as launch_batch_survey; trace
// non-null: the recording form of launch_batch_trace, in which the search
// records nothing), launch_batch_onset_gen Generations (arguments as
// launch_batch_gen).  Cycle detection is always on here, settle never.
hipError_t launch_batch_onset(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                              const RuleWords *rule, const uint32_t *rules, int64_t *period, int64_t *found,
                              int64_t *onset, int64_t gen0, uint32_t *trace, hipStream_t s);
hipError_t launch_batch_onset_gen(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells,
                                  uint32_t *decay, int planes, int64_t gens, uint32_t birth, uint32_t survive,
                                  uint32_t states, const uint32_t *rules, int64_t *period, int64_t *found,
                                  int64_t *onset, int64_t gen0, hipStream_t s);
// live[u] / sum[u] of universes [0, count): the live cells and the checksum of
// life_dev_checksum with the universe's own nx.
hipError_t launch_batch_census(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, const uint32_t *cells,
                               unsigned long long *live, unsigned long long *sum, hipStream_t s);
// n universes from `cells` on: dense bytes (ny * nx per universe) in and out
hipError_t launch_batch_import(const BatchPlan &p, int64_t nx, int64_t ny, int64_t n, const uint8_t *dense,
                               uint32_t *cells, hipStream_t s);
hipError_t launch_batch_export(const BatchPlan &p, int64_t nx, int64_t ny, int64_t n, const uint32_t *cells,
                               uint8_t *dense, hipStream_t s);
// The same with the state s of every cell in its byte, universes [first, first
// + n) of `count`: `cells` and `decay` are the bases of the alive plane and of
// the `planes` decay planes (0 .. 4; none: decay may be null).  The census
// counts s = 1 (live), s >= 2 (dying) and sums s * mix64.
hipError_t launch_batch_import_states(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, int64_t first,
                                      int64_t n, const uint8_t *dense, uint32_t *cells, uint32_t *decay, int planes,
                                      hipStream_t s);
hipError_t launch_batch_export_states(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, int64_t first,
                                      int64_t n, const uint32_t *cells, const uint32_t *decay, int planes,
                                      uint8_t *dense, hipStream_t s);
hipError_t launch_batch_census_states(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, const uint32_t *cells,
                                      const uint32_t *decay, int planes, unsigned long long *live,
                                      unsigned long long *dying, unsigned long long *sum, hipStream_t s);
// universe u = life_dev_fill_random(seed + u, thr32) of an nx x ny grid
hipError_t launch_batch_fill(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint64_t seed, uint32_t thr32,
                             uint32_t *cells, hipStream_t s);

}  // namespace life

#pragma GCC visibility pop
