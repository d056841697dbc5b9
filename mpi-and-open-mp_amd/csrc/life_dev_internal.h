// life_dev_internal.h -- what the units of the device runtime share (life_dev.hip,
// life_halo.hip, life_step.hip, life_timing.hip, life_frames.hip): the
// life_dev and its shards, the error macros, the predicates every unit asks,
// and the few functions one unit calls in another.  Private to csrc/; nothing
// declared here is among the library's dynamic symbols.
#pragma once
#include <rccl/rccl.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "life_host.h"
#include "life_io.h"
#include "life_kernels.h"
#include "life_mi355x.h"

#pragma GCC visibility push(hidden)

namespace life {
namespace rt {

extern thread_local std::string g_err;  // life_last_error (life_dev.hip)
void set_err(const char *fmt, ...);

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            life::rt::set_err("%s:%d %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? LIFE_ENOMEM : LIFE_EHIP;                       \
        }                                                                                     \
    } while (0)

#define NCCLCHK(expr)                                                                         \
    do {                                                                                      \
        ncclResult_t r_ = (expr);                                                             \
        if (r_ != ncclSuccess) {                                                              \
            life::rt::set_err("%s:%d %s: %s", __FILE__, __LINE__, #expr, ncclGetErrorString(r_)); \
            return LIFE_ERCCL;                                                                \
        }                                                                                     \
    } while (0)

#define CHK(expr)                     \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != LIFE_OK) return rc_; \
    } while (0)

constexpr int kPipeRing = 2 * life::kPipeMaxRegions;

struct TimedLaunch {
    hipEvent_t a = nullptr, b = nullptr;
    int launches = 1;  // kernel launches between a and b (back-to-back on one stream)
};

// Event set of one overlapped block (timing on): ring kernels, interior
// kernel, halo exchange, and the whole block on the compute stream.
struct PhaseEvents {
    hipEvent_t ring0 = nullptr, ring1 = nullptr, int0 = nullptr, int1 = nullptr, halo0 = nullptr,
               halo1 = nullptr, end = nullptr;
};

// One copy of the LOCAL transport, resolved when the plan is set
// (plan_halos): receive op `dop` of this shard's plan takes the message of
// send op `sop` of local shard `src` (staging slots dslot / sslot).
struct LocalCopy {
    int phase, src, sop, sslot, dop, dslot;
    size_t bytes;
};

struct Shard {
    int rank = 0;    // global shard rank (Cartesian rank, row-major coords)
    int device = 0;
    life_layout lay{};
    uint8_t *buf[2] = {nullptr, nullptr};
    int cur = 0;
    hipStream_t stream = nullptr;   // compute: whole-block kernels, boundary ring
    hipStream_t stream2 = nullptr;  // compute: interior, concurrent with ring + halo
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_halo = nullptr, ev_sync = nullptr, ev_int = nullptr;
    hipEvent_t ev_entry = nullptr;  // life_dev_step entry fence (see there)
    // pipelined passes (life_step.hip): launch i records ev_pipe[i % kPipeRing]
    // when a later launch waits for it, at most 2 R - 1 <= kPipeRing - 1 launches on
    hipEvent_t ev_pipe[kPipeRing] = {};
    // device span of the last step call (timing on): own_a / own_b recorded at
    // the call's two ends, or the kTimeCall pair borrowed (span_a / span_b)
    hipEvent_t own_a = nullptr, own_b = nullptr, span_a = nullptr, span_b = nullptr;
    ncclComm_t comm = nullptr;
    uint8_t *col_send = nullptr, *col_recv = nullptr;  // 2*h bytes each
    unsigned long long *d_count = nullptr;  // census: live count, checksum
    unsigned long long *h_count = nullptr;  // pinned, 2 entries
    uint8_t *sink = nullptr;  // stencil stores of lanes outside a region
    uint8_t *stage = nullptr;  // gather staging (grows on demand)
    size_t stage_bytes = 0;
    unsigned int *flow = nullptr;  // dataflow tiles: queue head, error word, per-tile pass counts (grows on demand)
    size_t flow_words = 0;
    bool flow_used = false;  // a dataflow launch since the last sync checked its error word
    // skip-dead passes (LIFE_OPT_SKIP_DEAD; allocated by the first such call): act_map[i] is buf[i]'s
    // activity map (life_act.h), act_cls the tiles' classes of the current pass (grows on demand),
    // act_cnt the call's counters: tiles run, cleared, skipped
    uint32_t *act_map[2] = {nullptr, nullptr};
    uint8_t *act_cls = nullptr;
    size_t act_cls_cap = 0;
    unsigned long long *act_cnt = nullptr;
    // population trace (LIFE_OPT_POPULATION; allocated by the first such call): pop_cnt the striped
    // counters of the pass in flight (life_kernels.h kPopCounterBytes, zero between passes), pop_trace
    // the last call's counts of this shard, one per generation (grows on demand)
    unsigned long long *pop_cnt = nullptr, *pop_trace = nullptr;
    size_t pop_cap = 0;
    std::vector<life_halo_op> plan;
    bool corners = false;  // the plan exchanges the four corner blocks itself (fused, one phase)
    // resolved with the plan (plan_halos): every op's staging slot; LOCAL
    // transport: its copies in plan order, and the local shards each phase
    // waits for, by kind (SEND / RECV), each once
    std::vector<int> slot;
    std::vector<LocalCopy> copies;
    std::vector<int> waits[2][2];  // [phase][LIFE_HALO_SEND / LIFE_HALO_RECV]
    std::vector<TimedLaunch> timers;
    size_t timers_used = 0;
    std::vector<PhaseEvents> phases;
    size_t phases_used = 0;
};

}  // namespace rt
}  // namespace life

struct life_dev {
    int64_t nx = 0, ny = 0;
    int dims[2] = {1, 1};
    int world = 1;
    int kernel = LIFE_KERNEL_BYTE;
    int transport = LIFE_XPORT_LOCAL;
    bool rank_mode = false;
    bool timing = false;
    bool phase_events = true;  // timing on: also the overlapped schedule's phase events (life_dev_set_timing 1)
    bool launch_events = true;  // timing on: per-launch events of multi-stream calls (off: life_dev_set_timing 3)
    bool overlap = true;
    int block_gens = 0;  // tiles: generations per launch at most (LIFE_OPT_BLOCK_GENS; never 0 after creation)
    int small_mode = 1;  // grids that fit one CU: 0 off, 1 VGPR kernel else LDS kernel, 2 LDS kernel,
                        // 3 windowed VGPR kernel over several CUs (else as 1), 4 as 1 never windowed
    int win_rows = 0, win_halo = 0;  // windowed kernel: strip height R, halo rows K (0: automatic)
    int loop = 0;  // LIFE_OPT_LOOPBACK: axes (bit 0 x, bit 1 y) whose halos the one shard exchanges with itself
    int last_path = LIFE_PATH_NONE;  // life_dev_last_path
    bool deep = true;  // LIFE_OPT_DEEP_HALO: one K-deep exchange feeds several passes (creation: LIFE_DEEP_HALO)
    int since = 0;  // generations advanced since the aprons were last filled (deep halo)
    int flow = 0;  // LIFE_OPT_FLOW: single-shard bit tiles as one persistent dataflow launch per
                   // step call (1: write-through hand-off, 2: plain stores + release; 0 off; creation: LIFE_FLOW)
    int64_t flow_chunk = 0;  // LIFE_OPT_FLOW_CHUNK: passes per dataflow launch at most (0: automatic)
    // life_dev_set_rule: the masks, and for a rule other than B3/S23 (`table`) the words its kernels take
    uint32_t birth = life::kConwayBirth, survive = life::kConwaySurvive;
    bool table = false;
    life::RuleWords words{};
    // LIFE_OPT_RULE7: the forms whose B3/S23 bit tiles run the 7-gate arm (LIFE_RULE7_TILES | LIFE_RULE7_FLOW;
    // creation: LIFE_RULE7), and the forms that did in the last step call (life_dev_last_rule_arm)
    int rule7 = 0, last_rule7 = 0;
    int pipe = 0;  // LIFE_OPT_PIPELINE: 0 off, 1 automatic, R >= 3 regions whenever a plan exists (creation: LIFE_PIPELINE)
    // the current step call's pipelined passes (life_step.hip pipelined_pass): R = 0, none; the plan
    // and the pass count of the current run of passes of m generations (a new m: a new run)
    struct {
        int R = 0, m = 0;
        int64_t pass = 0;
        life::PipePlan plan;
    } pipe_call;
    // LIFE_OPT_SKIP_DEAD: the option; whether both activity maps describe their buffers (dropped by every
    // writer of the state that is not a skip-dead pass, life_act.h); the skip-dead passes of the last
    // step call and the tiles of their grids (life_dev_activity)
    bool skip_dead = false, act_valid = false;
    int64_t act_passes = 0, act_total = 0;
    // LIFE_OPT_POPULATION: the option; the generations the last step call recorded and those folded so
    // far; whether the shard traces were already summed over the ranks (life_dev_population)
    bool population = false, pop_reduced = false;
    int64_t pop_n = 0, pop_pos = 0;
    life::rt::TimedLaunch *call_timer = nullptr;  // kTimeCall: the pair bracketing the current step call
    std::vector<life::rt::Shard> shards;
    double acc_ms = 0.0;
    int64_t acc_launches = 0;
    double acc_bytes = 0.0;    // algorithmic HBM bytes of the timed launches
    double acc_updates = 0.0;  // cell-updates they performed
    double acc_valu = 0.0;     // VALU lane-ops they issue (model; 0 where not modelled)
    // overlapped blocks of partitioned shards: summed ms per phase (timing on)
    double ph_ring = 0.0, ph_int = 0.0, ph_halo = 0.0, ph_block = 0.0;
    int64_t ph_blocks = 0;
    // the last step call (life_dev_call_stats): host time inside it, its
    // passes and the longest one's host time, whether span events exist
    double call_host_ms = 0.0, call_pass_max_ms = 0.0;
    int64_t call_passes = 0;
    bool call_spans = false;
};

namespace life {
namespace rt {

// Axis a's apron is filled by a halo exchange (dims[a] > 1, or the loopback
// test mode, where the single shard is its own neighbour on both axes).
inline bool part(const life_dev *d, int a) { return d->dims[a] > 1 || ((d->loop >> a) & 1); }
// The shard wraps x itself (the x-apron is filled by launch_wrap_columns).
inline bool self_wrap_x(const life_dev *d) { return !(d->loop & 1) && life::self_wrap_x(d->shards[0].lay, d->dims[0]); }
// The table-rule kernels' words, null under B3/S23 (launch_step / launch_tstep).
inline const life::RuleWords *rule_of(const life_dev *d) { return d->table ? &d->words : nullptr; }
// The per-launch / dataflow tiles of this device run their 7-gate arm (LIFE_OPT_RULE7): B3/S23 bit tiles
// only (launch_tstep ignores it under a table rule; the census and skip-dead tiles have one arm).
inline bool rule7_tiles(const life_dev *d) {
    return (d->rule7 & LIFE_RULE7_TILES) && d->kernel == LIFE_KERNEL_BIT && !d->table && !d->population;
}
inline bool rule7_flow(const life_dev *d) {
    return (d->rule7 & LIFE_RULE7_FLOW) && d->kernel == LIFE_KERNEL_BIT && !d->table;
}
inline life::Wrap wrap_of(const life_dev *d) { return life::Wrap{!part(d, 0) && !self_wrap_x(d), !part(d, 1)}; }
inline bool temporal(const life_dev *d) { return d->shards[0].lay.generations_per_exchange > 1; }
// Deep halo applies (generation_block): bit tiles, a partitioned axis, no
// self-wrapped x.
inline bool deep_halo(const life_dev *d) {
    return d->deep && d->kernel == LIFE_KERNEL_BIT && temporal(d) && (part(d, 0) || part(d, 1)) && !self_wrap_x(d);
}
// Generations per pass of the temporal tiles at most: the apron depth K,
// the 32 wrong cells a tile's edge lanes absorb, the block size.
inline int max_pass_gens(const life_dev *d) {
    return std::min(std::min(d->shards[0].lay.generations_per_exchange, 32), d->block_gens);
}
inline Shard *find_local(life_dev *d, int rank) {
    for (Shard &s : d->shards)
        if (s.rank == rank) return &s;
    return nullptr;
}

// ---- life_dev.hip
int bounded_sync(Shard &s, const char *what, int peer, hipStream_t st = nullptr);

// ---- life_halo.hip
// Sets every shard's halo plan (life::halo_plan with d->loop) and resolves it:
// `corners`, the staging slots, the LOCAL transport's copies and wait lists.
int plan_halos(life_dev *d);
// Halo of buffer `which_rel` (0 = cur, 1 = nxt) on the compute streams.
// Every call fills the aprons K deep: the deep-halo count restarts.
int exchange(life_dev *d, int which_rel, bool on_comm);

// ---- life_step.hip
int flow_prewarm(life_dev *d);

// ---- life_timing.hip
// How timed stencil launches are bracketed (LIFE_TIMING_MODE, measurement
// knob): 0 one event pair around a single-stream step call's launches (the
// default: one hipEventRecord before the first launch, none between
// launches), 1 per launch with hipEventRecord, 2 per launch stamped by the
// dispatch itself (hipExtLaunchKernel), 3 no events.
enum TimingMode { kTimeCall = 0, kTimeRecord = 1, kTimeExt = 2, kTimeOff = 3 };
int timing_mode();
TimedLaunch *timer_slot(Shard &s, int *rc);
PhaseEvents *phase_slot(Shard &s, int *rc);
// The bracket of one timed launch (or, step_small: of a call's launches).
// t null: no timer counts it (timing off, span-only timing,
// LIFE_TIMING_MODE=3) -- the caller books nothing.  Else one of: the call's
// pair (kTimeCall, no events here), a fresh pair recorded on the stream
// around the launch, or a fresh pair handed to the launcher as ext_a / ext_b,
// stamped by the dispatch itself (hipExtLaunchKernel): no event packets
// between the launches of a multi-stream step.
struct Bracket {
    TimedLaunch *t = nullptr;
    bool record = false;
    hipEvent_t ext_a = nullptr, ext_b = nullptr;
};
constexpr unsigned kExtNever = 0, kExtModeExt = 1u << kTimeExt, kExtModeCall = 1u << kTimeCall;
// ext_modes: the timing modes in which the launcher can stamp the pair itself;
// own_pair: always a fresh recorded pair (not the call's, whatever the mode).
int bracket_begin(life_dev *d, Shard &s, bool timed, int launches, unsigned ext_modes, bool own_pair, hipStream_t st,
                  Bracket *b);
int bracket_end(const Bracket &b, hipStream_t st);
// Books the work of timed launches: `cells` owned cells advanced
// `generations` by `launches` passes over HBM.  The compulsory HBM bytes:
// each owned cell is read once and written once per pass (0.25 B per bit
// cell, 2 B per byte cell), not once per generation -- that is the point of
// the blocking.
void book(life_dev *d, bool bit, double cells, double generations, double launches, double valu);

}  // namespace rt
}  // namespace life

#pragma GCC visibility pop
