// life_env.h -- every environment knob of the runtime: one table, three
// readers; the only file under csrc/ that calls getenv (no HIP types: g++
// alone compiles it with life_plan.cpp).  The value is parsed with atoi /
// atof; unset or outside the knob's range gives the default.  Knobs are read
// once per process by their user (a static there), except LIFE_POISON.
// INTEGRATION.md "Environment knobs" is the same table.
#pragma once
#include <limits.h>
#include <stdlib.h>

#include "life_mi355x.h"

namespace life {
namespace env {

struct IntKnob { const char *name; int dflt, lo, hi; };         // valid: lo <= v <= hi
struct FlagKnob { const char *name; int dflt; };                // 0 / 1; -1: unset means "per encoding"
struct RealKnob { const char *name; double dflt, lo, hi; };     // valid: lo < v <= hi

// `dflt`: the default of this read, for knobs whose default depends on the encoding
inline int read(const IntKnob &k, int dflt) {
    const char *e = getenv(k.name);
    const int v = e ? atoi(e) : dflt;
    return v >= k.lo && v <= k.hi ? v : dflt;
}
inline int read(const IntKnob &k) { return read(k, k.dflt); }
inline int read(const FlagKnob &k) {  // set: 1 if atoi reads non-zero, else 0
    const char *e = getenv(k.name);
    return e ? (atoi(e) != 0 ? 1 : 0) : k.dflt;
}
inline double read(const RealKnob &k) {
    const char *e = getenv(k.name);
    const double v = e ? atof(e) : k.dflt;
    return v > k.lo && v <= k.hi ? v : k.dflt;
}

// ---- one-generation stencil (life_kernels.hip launch_step): any integer is
// taken; rows other than 16 / 64 run the 32-row instance, depths other than
// 2 / 8 / 18 the 4-deep one
// rows per lane; default 16 for both encodings (profiles/r03/r5j tune_byte1.log)
constexpr IntKnob kStepRows{"LIFE_STEP_ROWS", 16, INT_MIN, INT_MAX};
// rows of loads in flight; default byte 8, bit 18 = the whole strip (profiles/r03/r5b tune_bit1.log)
constexpr IntKnob kStepDepth{"LIFE_STEP_DEPTH", 8, INT_MIN, INT_MAX};
// per-XCD runs of one-generation strips; unset: byte on, bit off (profiles/r03/r5f)
constexpr FlagKnob kXcdOrderOnegen{"LIFE_XCD_ORDER_ONEGEN", -1};
// ---- temporal tiles (life_kernels.hip)
// bit pair rows per wave, 16 or 24: the shapes with an instance (profiles/r05/a)
constexpr IntKnob kTemporalRows{"LIFE_TEMPORAL_ROWS", 24, 16, 24};
// byte word rows per wave, 32 or 48 (profiles/r02/r2w, r03/r4g)
constexpr IntKnob kTemporalRowsByte{"LIFE_TEMPORAL_ROWS_BYTE", 48, 32, 48};
// one ghost row for the byte tiles' step(1) launches; 0: K ghost rows (profiles/r02/ghost_ab.txt)
constexpr FlagKnob kByteOneGhost{"LIFE_BYTE_ONE_GHOST", 1};
// banded last tile column of the bit tiles; 0: full-width tiles (A/B knob, read by tests)
constexpr FlagKnob kBands{"LIFE_BANDS", 1};
// that column as up to two sub-columns (life::band_split); 0: one band, only when it owns <= 30 pairs (A/B knob)
constexpr FlagKnob kBandSplit{"LIFE_BAND_SPLIT", 1};
// the same for the dataflow form (A/B knob, read by tests)
constexpr FlagKnob kFlowBands{"LIFE_FLOW_BANDS", 1};
// bit tiles in per-XCD row-major runs; 0: dispatch order (profiles/r03/r5a)
constexpr FlagKnob kXcdOrder{"LIFE_XCD_ORDER", 1};
// the same for the byte tiles (profiles/r03/r5b, r5l)
constexpr FlagKnob kXcdOrderByte{"LIFE_XCD_ORDER_BYTE", 1};
// launch-tail split: 0 none, 1 the round-4 rule, 2 the list-scheduling model (profiles/r06/c)
constexpr IntKnob kTailSplit{"LIFE_TAIL_SPLIT", 2, 0, 2};
// ---- device runtime (life_dev.hip; LIFE_TIMING_MODE life_timing.hip, LIFE_INTERIOR_TAIL life_step.hip)
// generations per pass for both encodings; 0 = per encoding: bit 12, byte 32 (profiles/r03/r4g, r4d)
constexpr IntKnob kBlockGens{"LIFE_BLOCK_GENS", 0, 1, 32};
// default of LIFE_OPT_FLOW: 0 off, 1 / 2 the dataflow forms, 3 automatic (profiles/r02/flow_ab.txt, r03/r4g)
constexpr IntKnob kFlow{"LIFE_FLOW", 3, 0, 3};
// default of LIFE_OPT_DEEP_HALO
constexpr FlagKnob kDeepHalo{"LIFE_DEEP_HALO", 1};
// default of LIFE_OPT_PIPELINE: 0 off, 1 automatic, 3..16 that many row regions per pass (profiles/pipeline)
constexpr IntKnob kPipeline{"LIFE_PIPELINE", 1, 0, 16};
// default of LIFE_OPT_RULE7: bit 0 the per-launch bit tiles, bit 1 the dataflow tiles run B3/S23 in 7 gates
// per dword (ConwayRule7) instead of 8; 0: the 8-gate kernels everywhere (A/B knob; profiles/rule7)
constexpr IntKnob kRule7{"LIFE_RULE7", 3, 0, 3};
// timed launches: 0 one event pair per call, 1 per launch, 2 stamped by the dispatch, 3 no events (read by tests)
constexpr IntKnob kTimingMode{"LIFE_TIMING_MODE", 0, 0, 3};
// 1: allocations filled with 0xA5 instead of zeros; read at every life_dev_create* (tests set it in-process)
constexpr FlagKnob kPoison{"LIFE_POISON", 0};
// an exchange pass's interior splits its launch tail beside the ring (r06f ABAB lines)
constexpr FlagKnob kInteriorTail{"LIFE_INTERIOR_TAIL", 0};
// seconds before a rank-mode collective is declared dead
constexpr RealKnob kCommTimeoutS{"LIFE_COMM_TIMEOUT_S", 600.0, 0.0, 1e300};
// ---- layout (life_plan.cpp): every rank of a job must see the same value
// generations per halo exchange, bit: 1 / 8 / 12 / 16 / 24 / 32 (profiles/r03/r4g)
constexpr IntKnob kTemporalDepth{"LIFE_TEMPORAL_DEPTH", LIFE_TEMPORAL_DEPTH, 1, 32};
// the same, byte: 1 / 16 / 32, the ghost depths the byte tiles are built for (8 / 12 / 24 give 32)
constexpr IntKnob kTemporalDepthByte{"LIFE_TEMPORAL_DEPTH_BYTE", LIFE_TEMPORAL_DEPTH_BYTE, 1, 32};

}  // namespace env
}  // namespace life
