// life_timing.hip -- event timing of the device runtime: the per-launch /
// per-call timer pairs and their bracket, the phase events of the overlapped
// schedule, the call spans, and the statistics read from them.
#include "life_dev_internal.h"
#include "life_env.h"

using namespace life::rt;

static const int kEnvTimingMode = life::env::read(life::env::kTimingMode);

namespace life {
namespace rt {

int timing_mode() { return kEnvTimingMode; }

TimedLaunch *timer_slot(Shard &s, int *rc) {
    *rc = LIFE_OK;
    if (s.timers_used == s.timers.size()) {
        TimedLaunch t;
        if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) {
            set_err("hipEventCreate failed");
            *rc = LIFE_EHIP;
            return nullptr;
        }
        s.timers.push_back(t);
    }
    s.timers[s.timers_used].launches = 1;
    return &s.timers[s.timers_used++];
}

// kTimeCall books the launch into the call's pair (no events here); the
// per-launch modes take a fresh pair.
int bracket_begin(life_dev *d, Shard &s, bool timed, int launches, unsigned ext_modes, bool own_pair, hipStream_t st,
                  Bracket *b) {
    *b = Bracket{};
    if (!d->timing || !timed) return LIFE_OK;
    if (d->call_timer && !own_pair) {
        d->call_timer->launches += launches;
        b->t = d->call_timer;
        return LIFE_OK;
    }
    if (!own_pair && (kEnvTimingMode == kTimeOff || !d->launch_events)) return LIFE_OK;
    int rc;
    b->t = timer_slot(s, &rc);
    if (!b->t) return rc;
    b->t->launches = launches;
    if ((ext_modes >> kEnvTimingMode) & 1u) {
        b->ext_a = b->t->a;
        b->ext_b = b->t->b;
    } else {
        b->record = true;
        HIPCHK(hipEventRecord(b->t->a, st));
    }
    return LIFE_OK;
}

int bracket_end(const Bracket &b, hipStream_t st) {
    if (b.record) HIPCHK(hipEventRecord(b.t->b, st));
    return LIFE_OK;
}

void book(life_dev *d, bool bit, double cells, double generations, double launches, double valu) {
    d->acc_bytes += launches * cells * (bit ? 0.25 : 2.0);
    d->acc_updates += cells * generations;
    d->acc_valu += valu;
}

PhaseEvents *phase_slot(Shard &s, int *rc) {
    *rc = LIFE_OK;
    if (s.phases_used == s.phases.size()) {
        PhaseEvents p;
        for (hipEvent_t *e : {&p.ring0, &p.ring1, &p.int0, &p.int1, &p.halo0, &p.halo1, &p.end})
            if (hipEventCreate(e) != hipSuccess) {
                set_err("hipEventCreate failed");
                *rc = LIFE_EHIP;
                return nullptr;
            }
        s.phases.push_back(p);
    }
    return &s.phases[s.phases_used++];
}

}  // namespace rt
}  // namespace life

static int harvest_timers(life_dev *d) {
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        for (size_t i = 0; i < s.timers_used; i++) {
            HIPCHK(hipEventSynchronize(s.timers[i].b));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, s.timers[i].a, s.timers[i].b));
            d->acc_ms += ms;
            d->acc_launches += s.timers[i].launches;
        }
        s.timers_used = 0;
    }
    return LIFE_OK;
}

static int harvest_phases(life_dev *d) {
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        for (size_t i = 0; i < s.phases_used; i++) {
            const PhaseEvents &p = s.phases[i];
            for (hipEvent_t e : {p.end, p.ring1, p.int1, p.halo1}) HIPCHK(hipEventSynchronize(e));
            float r = 0.f, n = 0.f, h = 0.f, b = 0.f;
            HIPCHK(hipEventElapsedTime(&r, p.ring0, p.ring1));
            HIPCHK(hipEventElapsedTime(&n, p.int0, p.int1));
            HIPCHK(hipEventElapsedTime(&h, p.halo0, p.halo1));
            HIPCHK(hipEventElapsedTime(&b, p.ring0, p.end));
            d->ph_ring += r;
            d->ph_int += n;
            d->ph_halo += h;
            d->ph_block += b;
            d->ph_blocks++;
        }
        s.phases_used = 0;
    }
    return LIFE_OK;
}

extern "C" {

int life_dev_set_timing(life_dev *d, int on) {
    if (!d) return LIFE_EINVAL;
    CHK(harvest_timers(d));
    CHK(harvest_phases(d));
    if (on)  // a few event pairs up front: no hipEventCreate inside a timed step call
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            int rc = LIFE_OK;
            while (s.timers.size() < 8 && timer_slot(s, &rc)) {
            }
            if (rc != LIFE_OK) return rc;
            s.timers_used = 0;
        }
    d->ph_ring = d->ph_int = d->ph_halo = d->ph_block = 0.0;
    d->ph_blocks = 0;
    d->timing = on != 0;
    d->phase_events = on == 1;
    d->launch_events = on != 3;
    d->acc_ms = 0.0;
    d->acc_launches = 0;
    d->acc_bytes = 0.0;
    d->acc_updates = 0.0;
    d->acc_valu = 0.0;
    return LIFE_OK;
}

int life_dev_phase_stats(life_dev *d, double *ring_ms, double *interior_ms, double *halo_ms, double *block_ms,
                         int64_t *blocks) {
    if (!d) return LIFE_EINVAL;
    CHK(harvest_phases(d));
    const double n = d->ph_blocks ? (double)d->ph_blocks : 1.0;
    if (ring_ms) *ring_ms = d->ph_ring / n;
    if (interior_ms) *interior_ms = d->ph_int / n;
    if (halo_ms) *halo_ms = d->ph_halo / n;
    if (block_ms) *block_ms = d->ph_block / n;
    if (blocks) *blocks = d->ph_blocks;
    return LIFE_OK;
}

int life_dev_call_stats(life_dev *d, double *host_enqueue_ms, double *pass_enqueue_max_ms, int64_t *passes,
                        double *device_span_ms) {
    if (!d) return LIFE_EINVAL;
    double span = 0.0;
    if (d->call_spans)
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            HIPCHK(hipEventSynchronize(s.span_b));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, s.span_a, s.span_b));
            span = std::max(span, (double)ms);
        }
    if (host_enqueue_ms) *host_enqueue_ms = d->call_host_ms;
    if (pass_enqueue_max_ms) *pass_enqueue_max_ms = d->call_pass_max_ms;
    if (passes) *passes = d->call_passes;
    if (device_span_ms) *device_span_ms = span;
    return LIFE_OK;
}

int life_dev_kernel_work(life_dev *d, double *cell_updates_per_launch, double *valu_ops_per_launch) {
    if (!d) return LIFE_EINVAL;
    CHK(harvest_timers(d));
    const double n = d->acc_launches ? (double)d->acc_launches : 1.0;
    if (cell_updates_per_launch) *cell_updates_per_launch = d->acc_updates / n;
    if (valu_ops_per_launch) *valu_ops_per_launch = d->acc_valu / n;
    return LIFE_OK;
}

int life_dev_kernel_stats(life_dev *d, double *avg_ms, int64_t *launches, double *bytes_per_launch) {
    if (!d) return LIFE_EINVAL;
    CHK(harvest_timers(d));
    const double n = d->acc_launches ? (double)d->acc_launches : 1.0;
    if (avg_ms) *avg_ms = d->acc_ms / n;
    if (launches) *launches = d->acc_launches;
    if (bytes_per_launch) *bytes_per_launch = d->acc_bytes / n;
    return LIFE_OK;
}

}  // extern "C"
