// life_dev.hip -- C-ABI runtime of the MI355X Game-of-Life hot path: the core
// unit (creation, the shards' memory, synchronisation, options, getters).
//
// One life_dev owns the shards this process drives.  Each shard = one block of
// the dims[0] x dims[1] periodic Cartesian partition, double-buffered in HBM
// with a one-cell apron, one HIP stream, and (RCCL transport) one RCCL
// communicator rank.  The runtime is host code only, one unit per concern
// around life_dev_internal.h:
//   life_dev.hip     create / destroy, shard allocation, sync / barrier,
//                    life_dev_configure, the info getters, life_tune*
//   life_halo.hip    the halo exchange: LOCAL copies and RCCL groups, resolved
//                    once per halo plan (replaces life_cart.c:225-279)
//   life_step.hip    life_dev_step: the overlapped ring / interior / halo
//                    block, the temporal passes (planned by life::next_pass,
//                    life_plan.cpp), the dataflow and small-grid paths
//   life_timing.hip  timer and phase events, the timing bracket, the stats
//   life_frames.hip  upload, the dense / VTK / LIFEBITS gather, census, the
//                    sparse readouts, life_measure_copy
// The kernels are in life_kernels.hip (stencils) and life_io.hip (data
// movement); the planning arithmetic is in life_plan.cpp (no HIP).
#include <stdarg.h>

#include <chrono>
#include <thread>

#include "life_dev_internal.h"
#include "life_env.h"

using namespace life::rt;

thread_local std::string life::rt::g_err;

void life::rt::set_err(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

// Tiles: generations per launch at most (the apron depth K allows up to K).
// Bit tiles hold m ghost rows per window end, so longer launches mean more
// ghost rows (2m of the 192-row pair window) but fewer window loads /
// stores: 12 measured best at 65536^2 (992 generations: 112.3-112.9 T; 10:
// 109.4-110.0, 14: 111.3-111.7, 16: 108.4; profiles/r03/r4g), and a
// 20-generation call then runs as two launches of 10 (97.1-97.5 T against
// 93.5-93.9 for one launch of 20; profiles/r03/r4d).  Byte tiles are HBM-bound below ~32 generations per
// pass: 32.  LIFE_BLOCK_GENS overrides both at load time; 0 = per encoding.
static const int kEnvBlockGens = life::env::read(life::env::kBlockGens);
// LIFE_FLOW (0/1/2/3) sets LIFE_OPT_FLOW's default at load time; default 3,
// automatic (round 5): the dataflow form where a pass is only a few rounds
// of resident workgroups, so that a launch per pass would idle the chip in
// its tail (life_step.hip flow_form), the per-launch tiles elsewhere.
// With the natural-word tiles (384-row windows, 20 generations per pass) the
// dataflow form won (65536^2 95 -> 100 T, profiles/r02/flow_ab.txt); the
// pair tiles are half as tall, their items half as long, and the per-item
// queue / dependency / write-through cost now outweighs the launch tails it
// saves: 992 generations at 65536^2, per-launch tiles 109.4-112.9 T against
// 104.2-108.5 T for the dataflow form at every pass size 10-16
// (profiles/r03/r4g).
static const int kEnvFlow = life::env::read(life::env::kFlow);
// LIFE_DEEP_HALO (0/1, default 1) sets LIFE_OPT_DEEP_HALO's default at load
// time (life_step.hip generation_block).
static const bool kEnvDeepHalo = life::env::read(life::env::kDeepHalo) != 0;
// LIFE_PIPELINE (0, 1, 3..16) sets LIFE_OPT_PIPELINE's default at load time
// (life_step.hip pipelined_pass); 2 is no value of the option
static const int kEnvPipeline = [] {
    const int v = life::env::read(life::env::kPipeline);
    return v == 2 ? life::env::kPipeline.dflt : v;
}();
// LIFE_RULE7 (0..3) sets LIFE_OPT_RULE7's default at load time: the forms
// (LIFE_RULE7_TILES | LIFE_RULE7_FLOW) whose B3/S23 bit tiles run the 7-gate
// arm (life_kernels.hip tstep_bit7_kernel / tflow7_kernel)
static const int kEnvRule7 = life::env::read(life::env::kRule7);
static int default_block_gens(int kernel) {
    return kEnvBlockGens ? kEnvBlockGens : (kernel == LIFE_KERNEL_BIT ? 12 : 32);
}

namespace {

// Allocation fill of every shard buffer (LIFE_POISON, read at each
// life_dev_create*): unset / 0 = zeros (a dead grid, what the reference's
// calloc gives); 1 = 0xA5 in both grid buffers (cells, aprons, pitch padding,
// slack rows), the column staging and the sink -- not a dead cell in either
// encoding, so a cell a kernel should have written but did not, or an apron
// read before its halo arrived, changes the result on every run instead of
// hiding behind a zeroed buffer that looks like a dead grid.
int alloc_fill_byte() { return life::env::read(life::env::kPoison) ? 0xA5 : 0; }

int shard_alloc(Shard &s) {
    HIPCHK(hipSetDevice(s.device));
    // The streams first: every fill below is ordered on the stream that later
    // uses the buffer (the null stream does not order against non-blocking
    // streams), and finished before the shard is handed out.
    // All three at priority 0: the comm and ring streams at the greatest
    // priority and the interior at the least kept the RCCL-loopback halo at
    // 0.23 ms beside the interior (86.5-91.2 T with, 90.0-90.8 T without) and
    // dropped the LOCAL 4-shard strong line 48.9 -> 34.4 T (profiles/r04/a).
    HIPCHK(hipStreamCreateWithPriority(&s.stream, hipStreamNonBlocking, 0));
    HIPCHK(hipStreamCreateWithPriority(&s.stream2, hipStreamNonBlocking, 0));
    HIPCHK(hipStreamCreateWithPriority(&s.comm_stream, hipStreamNonBlocking, 0));
    const int fill = alloc_fill_byte();
    const int64_t slack = s.lay.generations_per_exchange > 1 ? life::kTemporalSlackRows : 0;
    const size_t bytes = (size_t)(s.lay.pitch * (s.lay.rows + slack));
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipMalloc(&s.buf[i], bytes));
        HIPCHK(hipMemsetAsync(s.buf[i], fill, bytes, s.stream));
    }
    // (device-scope forms of these events, hipEventDisableSystemFence /
    // hipEventReleaseToDevice, measured flat: profiles/r06/h)
    HIPCHK(hipEventCreateWithFlags(&s.ev_int, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.ev_halo, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.ev_sync, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.ev_entry, hipEventDisableTiming));
    for (hipEvent_t &e : s.ev_pipe) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const size_t col_bytes = (size_t)life::column_stage_bytes(s.lay);
    HIPCHK(hipMalloc(&s.col_send, col_bytes));
    HIPCHK(hipMalloc(&s.col_recv, col_bytes));
    HIPCHK(hipMalloc(&s.d_count, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMalloc(&s.sink, 1024));
    HIPCHK(hipMemsetAsync(s.col_send, fill, col_bytes, s.stream));
    HIPCHK(hipMemsetAsync(s.col_recv, fill, col_bytes, s.stream));
    HIPCHK(hipMemsetAsync(s.d_count, 0, 2 * sizeof(unsigned long long), s.stream));
    HIPCHK(hipMemsetAsync(s.sink, fill, 1024, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipHostMalloc(&s.h_count, 2 * sizeof *s.h_count, hipHostMallocDefault));
    return LIFE_OK;
}

void shard_free(Shard &s) {
    (void)hipSetDevice(s.device);
    if (s.comm) (void)ncclCommDestroy(s.comm);
    for (auto &t : s.timers) {
        if (t.a) (void)hipEventDestroy(t.a);
        if (t.b) (void)hipEventDestroy(t.b);
    }
    for (auto &p : s.phases)
        for (hipEvent_t e : {p.ring0, p.ring1, p.int0, p.int1, p.halo0, p.halo1, p.end})
            if (e) (void)hipEventDestroy(e);
    for (uint8_t *p : {s.buf[0], s.buf[1], s.col_send, s.col_recv, s.sink, s.stage})
        if (p) (void)hipFree(p);
    if (s.flow) (void)hipFree(s.flow);
    if (s.act_map[0]) (void)hipFree(s.act_map[0]);  // one allocation holds both maps
    if (s.act_cls) (void)hipFree(s.act_cls);
    if (s.act_cnt) (void)hipFree(s.act_cnt);
    if (s.pop_cnt) (void)hipFree(s.pop_cnt);
    if (s.pop_trace) (void)hipFree(s.pop_trace);
    if (s.d_count) (void)hipFree(s.d_count);
    if (s.h_count) (void)hipHostFree(s.h_count);
    for (hipEvent_t e : {s.ev_halo, s.ev_sync, s.ev_int, s.ev_entry, s.own_a, s.own_b})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : s.ev_pipe)
        if (e) (void)hipEventDestroy(e);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    if (s.stream2) (void)hipStreamDestroy(s.stream2);
    if (s.comm_stream) (void)hipStreamDestroy(s.comm_stream);
}

// Seconds a rank-mode collective may take before it is declared dead
// (LIFE_COMM_TIMEOUT_S, default 600): a peer that died or never joined would
// otherwise leave this rank spinning in an RCCL kernel forever.
double comm_timeout_s() {
    static const double t = life::env::read(life::env::kCommTimeoutS);
    return t;
}

// Rank mode: a collective check that every rank passes the same `value`
// (an int64 max all-reduce of {value, -value}); bounded like the barrier.
int agree_all_ranks(life_dev *d, int value, const char *what) {
    for (Shard &s : d->shards) {
        if (!s.comm) continue;
        HIPCHK(hipSetDevice(s.device));
        int64_t *h = reinterpret_cast<int64_t *>(s.h_count);
        h[0] = value;
        h[1] = -(int64_t)value;
        HIPCHK(hipMemcpyAsync(s.d_count, h, 2 * sizeof(int64_t), hipMemcpyHostToDevice, s.stream));
        NCCLCHK(ncclAllReduce(s.d_count, s.d_count, 2, ncclInt64, ncclMax, s.comm, s.stream));
        HIPCHK(hipMemcpyAsync(h, s.d_count, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s.stream));
        CHK(bounded_sync(s, what, -1));
        const int64_t hi = h[0], lo = -h[1];
        if (hi != lo) {
            set_err("%s is collective in rank mode: ranks passed %lld .. %lld", what, (long long)lo, (long long)hi);
            return LIFE_EINVAL;
        }
    }
    return LIFE_OK;
}

// The life_dev both creators fill: dims given or chosen (life_dims_create),
// the options at their load-time defaults.  nullptr: the dims do not make
// `world` blocks.
life_dev *new_dev(int64_t nx, int64_t ny, int dims0, int dims1, int world, int kernel) {
    int dims[2] = {dims0, dims1};
    if (dims0 <= 0 || dims1 <= 0) life_dims_create(world, dims);
    if (dims[0] * dims[1] != world) return nullptr;
    life_dev *d = new life_dev;
    d->nx = nx;
    d->ny = ny;
    d->dims[0] = dims[0];
    d->dims[1] = dims[1];
    d->world = world;
    d->kernel = kernel;
    d->block_gens = default_block_gens(kernel);
    d->deep = kEnvDeepHalo;
    d->flow = kEnvFlow;
    d->pipe = kEnvPipeline;
    d->rule7 = kEnvRule7;
    return d;
}

// The shards of this process: layout, memory, then every halo plan (resolved
// against each other: life_halo.hip plan_halos).
int create_shards(life_dev *d, const std::vector<int> &ranks, const std::vector<int> &devices) {
    for (size_t i = 0; i < ranks.size(); i++) {
        d->shards.emplace_back();
        Shard &s = d->shards.back();
        s.rank = ranks[i];
        s.device = devices[i];
        const int rc = life_layout_query(d->nx, d->ny, d->dims[0], d->dims[1], s.rank, d->kernel, &s.lay);
        if (rc != LIFE_OK) {
            set_err("layout: nx=%lld ny=%lld dims=%dx%d rank %d kernel %d", (long long)d->nx,
                    (long long)d->ny, d->dims[0], d->dims[1], s.rank, d->kernel);
            return rc;
        }
    }
    for (Shard &s : d->shards) CHK(shard_alloc(s));
    return plan_halos(d);
}

// The launch-tail plans (life::tail_plan) of the passes this device's step
// calls will launch, computed up front: a plan's first search costs ~50 us of
// host time, which a timed call's first launch would otherwise wait for
// (deep-halo passes: every extension 0 .. K - m).
void tail_prewarm(const life_dev *d) {
    for (size_t i = 0; i < d->shards.size(); ++i) {
        bool seen = false;  // identical blocks share their plans (cached by shape)
        for (size_t j = 0; j < i; ++j)
            seen |= d->shards[j].lay.w == d->shards[i].lay.w && d->shards[j].lay.h == d->shards[i].lay.h;
        if (!seen) life::prewarm_tail_plans(d->shards[i].lay, max_pass_gens(d), part(d, 1), d->table, rule7_tiles(d));
    }
}

// The end of both creators: the device is destroyed on an error, else
// prewarmed and handed out.
int finish_create(life_dev *d, int rc, life_dev **out) {
    if (rc != LIFE_OK) {
        life_dev_destroy(d);
        return rc;
    }
    // not fatal: the first dataflow call allocates and launches as it would
    if (flow_prewarm(d) != LIFE_OK) (void)hipGetLastError();
    tail_prewarm(d);
    *out = d;
    return LIFE_OK;
}

// hipStreamSynchronize, but polling the stream for the first milliseconds:
// the blocking wait woke ~10 us after the last kernel ended (profiles/r03/r4d
// trace), 1 % of a 20-generation 65536^2 call.
hipError_t wait_stream(hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) return hipStreamSynchronize(st);
    }
}

}  // namespace

// hipStreamSynchronize with a deadline: polls the stream; on timeout aborts
// the shard's communicator (which ends RCCL kernels stuck on a missing peer)
// and fails with a message naming the operation.
int life::rt::bounded_sync(Shard &s, const char *what, int peer, hipStream_t st) {
    if (!st) st = s.stream;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return LIFE_OK;
        if (e != hipErrorNotReady) {
            set_err("%s (peer %d): %s", what, peer, hipGetErrorString(e));
            return LIFE_EHIP;
        }
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (dt > comm_timeout_s()) {
            if (s.comm) {
                (void)ncclCommAbort(s.comm);
                s.comm = nullptr;
            }
            set_err("%s: rank %d waited %.0f s for peer %d (LIFE_COMM_TIMEOUT_S); communicator aborted", what,
                    s.rank, dt, peer);
            return LIFE_ERCCL;
        }
        // busy-poll the first 20 ms (a step's end is seen within a few us,
        // as wait_stream), then back off to 1 ms naps
        if (dt > 0.02) std::this_thread::sleep_for(std::chrono::microseconds(1000));
    }
}

extern "C" {

const char *life_last_error(void) { return g_err.c_str(); }

int life_dev_create_ex(int64_t nx, int64_t ny, int nshards, int dims0, int dims1, int kernel,
                       int transport, life_dev **out) {
    if (!out || nx <= 0 || ny <= 0 || nshards <= 0) return LIFE_EINVAL;
    *out = nullptr;
    int ndev = 0;
    life_dev *d = new_dev(nx, ny, dims0, dims1, nshards, kernel);
    if (!d) {
        set_err("dims %dx%d != %d shards", dims0, dims1, nshards);
        return LIFE_EINVAL;
    }
    {
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0) {
            set_err("no HIP device: %s", hipGetErrorString(e));
            delete d;
            return LIFE_EHIP;
        }
    }
    std::vector<int> ranks, devices;
    for (int i = 0; i < nshards; i++) {
        ranks.push_back(i);
        devices.push_back(i % ndev);
    }
    const bool distinct = nshards <= ndev;
    if (transport == LIFE_XPORT_AUTO) transport = (distinct && nshards > 1) ? LIFE_XPORT_RCCL : LIFE_XPORT_LOCAL;
    if (transport == LIFE_XPORT_RCCL && !distinct) {
        set_err("RCCL transport needs one device per shard (%d shards, %d devices)", nshards, ndev);
        delete d;
        return LIFE_EINVAL;
    }
    d->transport = transport;
    int rc = create_shards(d, ranks, devices);
    // RCCL: one communicator rank per shard, all driven by this process
    // (ncclCommInitAll; the halo phases group every shard's sends / recvs in
    // one ncclGroupStart/End).  A single shard gets a one-device communicator
    // too, so LIFE_OPT_LOOPBACK runs this exact path on a one-GPU box.
    if (rc == LIFE_OK && transport == LIFE_XPORT_RCCL) {
        std::vector<ncclComm_t> comms(nshards);
        ncclResult_t r = ncclCommInitAll(comms.data(), nshards, devices.data());
        if (r != ncclSuccess) {
            set_err("ncclCommInitAll: %s", ncclGetErrorString(r));
            rc = LIFE_ERCCL;
        } else {
            for (int i = 0; i < nshards; i++) d->shards[i].comm = comms[i];
        }
    }
    if (rc == LIFE_OK && transport == LIFE_XPORT_LOCAL && nshards > 1) {
        for (int a = 0; a < ndev && a < nshards; a++)
            for (int b = 0; b < ndev && b < nshards; b++)
                if (a != b) {
                    (void)hipSetDevice(a);
                    (void)hipDeviceEnablePeerAccess(b, 0);  // already-enabled is fine
                }
        (void)hipGetLastError();
    }
    return finish_create(d, rc, out);
}

int life_dev_create(int64_t nx, int64_t ny, int nshards, int kernel, life_dev **out) {
    return life_dev_create_ex(nx, ny, nshards, 0, 0, kernel, LIFE_XPORT_AUTO, out);
}

int life_get_unique_id(uint8_t unique_id[128]) {
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    memcpy(unique_id, &id, sizeof id);
    return LIFE_OK;
}

int life_dev_create_rank(int64_t nx, int64_t ny, int kernel, int rank, int world, int dims0, int dims1,
                         const uint8_t unique_id[128], int device, life_dev **out) {
    if (!out || nx <= 0 || ny <= 0 || world <= 0 || rank < 0 || rank >= world) return LIFE_EINVAL;
    *out = nullptr;
    life_dev *d = new_dev(nx, ny, dims0, dims1, world, kernel);
    if (!d) return LIFE_EINVAL;
    d->rank_mode = true;
    d->transport = LIFE_XPORT_RCCL;
    int rc = create_shards(d, {rank}, {device});
    // A communicator whenever the caller hands a unique id, world 1 included
    // (then only the census all-reduce uses it; that is how a one-GPU box
    // exercises RCCL initialisation in the torchrun process set-up).
    if (rc == LIFE_OK && (world > 1 || unique_id)) {
        if (!unique_id) {
            rc = LIFE_EINVAL;
        } else {
            ncclUniqueId id;
            memcpy(&id, unique_id, sizeof id);
            (void)hipSetDevice(device);
            ncclResult_t r = ncclCommInitRank(&d->shards[0].comm, world, id, rank);
            if (r != ncclSuccess) {
                set_err("ncclCommInitRank(rank %d/%d): %s", rank, world, ncclGetErrorString(r));
                rc = LIFE_ERCCL;
            }
        }
    }
    return finish_create(d, rc, out);
}

void life_dev_destroy(life_dev *d) {
    if (!d) return;
    for (Shard &s : d->shards) {
        (void)hipSetDevice(s.device);
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.stream2) (void)hipStreamSynchronize(s.stream2);
        if (s.comm_stream) (void)hipStreamSynchronize(s.comm_stream);
    }
    for (Shard &s : d->shards) shard_free(s);
    delete d;
}

int life_device_count(void) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_err("hipGetDeviceCount: %s", hipGetErrorString(e));
        return LIFE_EHIP;
    }
    return n;
}

int life_dev_barrier(life_dev *d) {
    if (!d) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    if (d->rank_mode)
        for (Shard &s : d->shards)
            if (s.comm) {
                // an all-reduce every rank must join: no rank leaves before all arrived
                HIPCHK(hipSetDevice(s.device));
                NCCLCHK(ncclAllReduce(s.d_count, s.d_count, 1, ncclUint64, ncclSum, s.comm, s.stream));
                CHK(bounded_sync(s, "barrier all-reduce", -1));
            }
    return LIFE_OK;
}

int life_dev_sync(life_dev *d) {
    if (!d) return LIFE_EINVAL;
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        if (d->rank_mode && s.comm) {
            // a step's halo waits on RCCL peers: a peer that died must not
            // hang this rank (LIFE_COMM_TIMEOUT_S, then ncclCommAbort)
            CHK(bounded_sync(s, "sync: compute stream", -1, s.stream));
            CHK(bounded_sync(s, "sync: interior stream", -1, s.stream2));
            CHK(bounded_sync(s, "sync: halo stream", -1, s.comm_stream));
        } else {
            HIPCHK(wait_stream(s.stream));
            HIPCHK(wait_stream(s.stream2));
            HIPCHK(wait_stream(s.comm_stream));
        }
        if (s.flow_used) {
            // a dataflow launch whose dependency wait timed out (a broken
            // hand-off): its result cannot be trusted
            unsigned int err = 0;
            HIPCHK(hipMemcpyAsync(&err, s.flow + 1, sizeof err, hipMemcpyDeviceToHost, s.stream));
            HIPCHK(hipStreamSynchronize(s.stream));
            s.flow_used = false;
            if (err) {
                HIPCHK(hipMemsetAsync(s.flow + 1, 0, sizeof err, s.stream));
                HIPCHK(hipStreamSynchronize(s.stream));
                set_err("dataflow tiles: item %u waited too long for its neighbours (state is invalid)", err - 1);
                return LIFE_ESTATE;
            }
        }
    }
    return LIFE_OK;
}

int life_dev_layout(life_dev *d, int local_shard, life_layout *out) {
    if (!d || !out || local_shard < 0 || local_shard >= (int)d->shards.size()) return LIFE_EINVAL;
    *out = d->shards[local_shard].lay;
    return LIFE_OK;
}

int life_dev_world(life_dev *d, int *world, int *dims0, int *dims1, int *nlocal, int *transport) {
    if (!d) return LIFE_EINVAL;
    if (world) *world = d->world;
    if (dims0) *dims0 = d->dims[0];
    if (dims1) *dims1 = d->dims[1];
    if (nlocal) *nlocal = (int)d->shards.size();
    if (transport) *transport = d->transport;
    return LIFE_OK;
}

int life_dev_shard_info(life_dev *d, int local_shard, int *device, char pci_bus_id[64], int *rccl_nranks) {
    if (!d || local_shard < 0 || local_shard >= (int)d->shards.size()) return LIFE_EINVAL;
    const Shard &s = d->shards[local_shard];
    if (device) *device = s.device;
    if (pci_bus_id) HIPCHK(hipDeviceGetPCIBusId(pci_bus_id, 64, s.device));
    if (rccl_nranks) {
        int n = 0;
        if (s.comm) NCCLCHK(ncclCommCount(s.comm, &n));
        *rccl_nranks = n;
    }
    return LIFE_OK;
}

int life_dev_configure(life_dev *d, int option, int value) {
    if (!d) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    switch (option) {
    case LIFE_OPT_SMALL_GRID:
        if (value < 0 || value > 4) return LIFE_EINVAL;
        d->small_mode = value;
        return LIFE_OK;
    case LIFE_OPT_SMALL_WINDOW: {
        const int R = value >> 8, K = value & 255;  // R = 0 (value 0): automatic
        if (value != 0 && (K < 1 || R < 1 || R > 8 || R == 7)) return LIFE_EINVAL;
        // a window the shard cannot hold (own = strips*R - 2K rows < 1, or
        // >= h) would silently fall back to the unwindowed kernel: refuse it
        if (value != 0 && life::reg_win_plan(d->shards[0].lay, R, K).blocks == 0) {
            set_err("small-grid window R=%d K=%d does not fit this grid", R, K);
            return LIFE_EINVAL;
        }
        d->win_rows = R;
        d->win_halo = K;
        return LIFE_OK;
    }
    case LIFE_OPT_OVERLAP: d->overlap = value != 0; return LIFE_OK;
    case LIFE_OPT_BLOCK_GENS:
        if (value < 0 || value > 32) return LIFE_EINVAL;
        d->block_gens = value > 0 ? value : default_block_gens(d->kernel);
        tail_prewarm(d);
        return LIFE_OK;
    case LIFE_OPT_FLOW:
        if (value < 0 || value > 3) return LIFE_EINVAL;
        d->flow = value;
        return LIFE_OK;
    case LIFE_OPT_DEEP_HALO:
        if (value < 0 || value > 1) return LIFE_EINVAL;
        // Aprons valid only to the remaining depth K - since are refilled by
        // the next pass that needs more (life::next_pass).  But the option
        // decides which passes exchange, so in rank mode every rank must hold
        // the same value or their ncclSend / ncclRecv groups stop pairing up
        // (ADVICE r5): the call is collective there and checks agreement.
        if (d->rank_mode && d->world > 1) CHK(agree_all_ranks(d, value, "LIFE_OPT_DEEP_HALO"));
        d->deep = value != 0;
        return LIFE_OK;
    case LIFE_OPT_PIPELINE:
        if (value < 0 || value == 2 || value > life::kPipeMaxRegions) return LIFE_EINVAL;
        d->pipe = value;
        return LIFE_OK;
    case LIFE_OPT_RULE7:
        // accepted on every device; it acts on the B3/S23 bit tiles (rule7_tiles / rule7_flow)
        if (value < 0 || value > (LIFE_RULE7_TILES | LIFE_RULE7_FLOW)) return LIFE_EINVAL;
        d->rule7 = value;
        tail_prewarm(d);  // the tail plans count the slots of the kernel that will run
        return LIFE_OK;
    case LIFE_OPT_FLOW_CHUNK:
        if (value < 0) return LIFE_EINVAL;
        d->flow_chunk = value;
        return LIFE_OK;
    case LIFE_OPT_SKIP_DEAD:
        // accepted on every device; it acts where life_step.hip skip_dead_applies
        if (value < 0 || value > 1) return LIFE_EINVAL;
        if (value) d->act_valid = false;  // turning it on: the maps are rebuilt by the next step call
        d->skip_dead = value != 0;
        return LIFE_OK;
    case LIFE_OPT_POPULATION:
        // accepted on every device: census tiles where life_step.hip pop_fast, else a census per generation
        if (value < 0 || value > 1) return LIFE_EINVAL;
        d->population = value != 0;
        return LIFE_OK;
    case LIFE_OPT_LOOPBACK: {
        // 1: both axes, 2: x only, 3: y only (the axes a real partition of
        // N GPUs cuts: N = 2's {2, 1} cuts x only)
        if (value < 0 || value > 3) return LIFE_EINVAL;
        if (d->world != 1 || d->shards.size() != 1) {
            set_err("loopback needs a single-shard world (world %d, %zu local shards)", d->world, d->shards.size());
            return LIFE_EINVAL;
        }
        Shard &s = d->shards[0];
        // the aprons a partitioned axis needs: at least K rows / one x-apron
        // of columns to send
        if (value && (s.lay.h < s.lay.yapron || s.lay.w < s.lay.xapron)) {
            set_err("loopback: %lld x %lld cells < the %lld-column / %lld-row halo", (long long)s.lay.w,
                    (long long)s.lay.h, (long long)s.lay.xapron, (long long)s.lay.yapron);
            return LIFE_EINVAL;
        }
        if (value && d->transport == LIFE_XPORT_RCCL && !s.comm) {
            set_err("loopback over RCCL needs a communicator (life_dev_create_rank with a unique id, or "
                    "life_dev_create_ex with LIFE_XPORT_RCCL)");
            return LIFE_EINVAL;
        }
        // the current state's aprons are refreshed on the next step's first
        // exchange only: fill them now from the shard itself
        d->loop = value == 0 ? 0 : value == 1 ? 3 : value == 2 ? 1 : 2;
        CHK(plan_halos(d));
        CHK(exchange(d, 0, false));
        tail_prewarm(d);
        return life_dev_sync(d);
    }
    default: return LIFE_EINVAL;
    }
}

int life_dev_set_rule(life_dev *d, uint32_t birth, uint32_t survive) {
    if (!d) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    char name[24] = "";
    if ((birth | survive) & ~life::kRuleMask) {
        set_err("rule masks 0x%x / 0x%x: bits above 8", birth, survive);
        return LIFE_EINVAL;
    }
    life::rule_format(birth, survive, name);
    if (birth & 1u) {
        set_err("rule %s: B0 rules are not supported (dead padding and ghost rows must stay dead)", name);
        return LIFE_EINVAL;
    }
    const bool table = birth != life::kConwayBirth || survive != life::kConwaySurvive;
    if (table && d->kernel != LIFE_KERNEL_BIT) {
        set_err("rule %s: the byte encoding runs B3/S23 only (rules are a feature of LIFE_KERNEL_BIT)", name);
        return LIFE_EINVAL;
    }
    // every rank must evolve the same universe: collective in rank mode, as LIFE_OPT_DEEP_HALO
    if (d->rank_mode && d->world > 1) CHK(agree_all_ranks(d, (int)(birth | (survive << 9)), "life_dev_set_rule"));
    d->birth = birth;
    d->survive = survive;
    const bool changed = table != d->table;
    d->table = table;
    if (table) d->words = life::rule_words(birth, survive);
    if (changed) tail_prewarm(d);  // the tail plans of the kernel that will run (2 or 3 tiles per CU)
    return LIFE_OK;
}

int life_dev_get_rule(life_dev *d, uint32_t *birth, uint32_t *survive) {
    if (!d) return LIFE_EINVAL;
    if (birth) *birth = d->birth;
    if (survive) *survive = d->survive;
    return LIFE_OK;
}

int life_tune(int kernel, int rows, int depth) {
    if ((rows && rows != 16 && rows != 32 && rows != 64) ||
        (depth && depth != 2 && depth != 4 && depth != 8 && depth != 18) ||
        kernel < -1 || kernel > LIFE_KERNEL_BIT)
        return LIFE_EINVAL;
    life::set_step_tuning(kernel, rows, depth);
    return LIFE_OK;
}

int life_tune_temporal(int kernel, int rows) {
    const bool bit_ok = rows == 16 || rows == 24;
    const bool byte_ok = rows == 32 || rows == 48;
    if (kernel < -1 || kernel > LIFE_KERNEL_BIT) return LIFE_EINVAL;
    if (rows && ((kernel == LIFE_KERNEL_BIT && !bit_ok) || (kernel == LIFE_KERNEL_BYTE && !byte_ok) ||
                 (kernel == -1 && !bit_ok && !byte_ok)))
        return LIFE_EINVAL;
    life::set_temporal_rows(kernel, rows);
    return LIFE_OK;
}

}  // extern "C"
