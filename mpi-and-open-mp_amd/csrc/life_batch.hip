// life_batch.hip -- the life_batch runtime (include/life_mi355x.h, DESIGN.md
// 5.11): `count` independent universes of one shape on one GPU, one stream.
// The plan is life::batch_plan (life_plan.cpp), the kernels are
// life_batch_kernels.hip.  Every call sets the batch's device and enqueues on
// its stream; the blocking ones wait for it.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "life_batch_kernels.h"
#include "life_dev_internal.h"

using namespace life::rt;

struct life_batch {
    int64_t nx = 0, ny = 0, count = 0;
    int device = 0;
    life::BatchPlan plan;
    hipStream_t stream = nullptr;
    uint32_t *cells = nullptr;
    int64_t *settled = nullptr;  // per universe: -1, or the generation LIFE_BATCH_OPT_SETTLE found it settled at
    unsigned long long *census = nullptr;  // live[count], checksum[count]
    bool census_valid = false;             // of the current states
    uint8_t *stage = nullptr;              // dense staging of upload / gather (grows on demand)
    size_t stage_bytes = 0;
    uint32_t birth = life::kConwayBirth, survive = life::kConwaySurvive;
    bool table = false;
    life::RuleWords words{};
    // "mixed" (life_batch_set_rules): (birth, survive) of universe u at rules[2 u]; null on a uniform batch
    uint32_t *rules = nullptr;
    bool settle = false;
    bool cycle = false;
    int64_t *cycles = nullptr;  // period[count], found[count] of LIFE_BATCH_OPT_CYCLE (from its first use)
    bool onset = false;
    int64_t *onsets = nullptr;  // per universe: -1, or the onset LIFE_BATCH_OPT_ONSET computed (from its first use)
    int64_t generation = 0;
    // Generations.  `states` is the uniform rule's; on a mixed batch `shadow` holds every
    // universe's and `hist` how many universes have each count.  `decay`: `planes` (0, 1, 2, 4) bit planes of d = s
    // - 1 of the dying cells, each as large as `cells`, plane-major; as many as the largest state count since the
    // batch last was two-state needs.
    uint32_t states = 2;
    std::vector<uint8_t> shadow;
    int64_t hist[life::kGenMaxStates + 1] = {};
    uint32_t *decay = nullptr;
    int planes = 0;
    unsigned long long *census_gen = nullptr;  // live[count], dying[count], checksum[count] of life_batch_census_gen
    // LIFE_BATCH_OPT_POPULATION: the trace of the last step call, count * trace_gens entries,
    // universe-major, in a buffer of trace_cap entries (grown to the largest call, released with the option)
    bool population = false;
    uint32_t *trace = nullptr;
    int64_t trace_cap = 0, trace_gens = 0;
};

namespace {

size_t words_of(const life_batch *b, int64_t n) { return (size_t)n * (size_t)(b->plan.bytes / 4); }

int stage_for(life_batch *b, size_t bytes) {
    if (b->stage_bytes >= bytes) return LIFE_OK;
    if (b->stage) HIPCHK(hipFree(b->stage));
    b->stage = nullptr;
    b->stage_bytes = 0;
    HIPCHK(hipMalloc(&b->stage, bytes));
    b->stage_bytes = bytes;
    return LIFE_OK;
}

int range_ok(const life_batch *b, int64_t first, int64_t n, const void *grids, const char *what) {
    if (first < 0 || n < 0 || first > b->count || n > b->count - first || (n > 0 && !grids)) {
        set_err("%s: universes [%lld, %lld + %lld) of %lld%s", what, (long long)first, (long long)first, (long long)n,
                (long long)b->count, n > 0 && !grids ? ", no grids" : "");
        return LIFE_EINVAL;
    }
    return LIFE_OK;
}

// settled flags of universes [first, first + n) back to -1, their cycle pairs to 0 / -1, their onsets to -1
int clear_settled(life_batch *b, int64_t first, int64_t n) {
    if (n < 1) return LIFE_OK;
    HIPCHK(hipMemsetAsync(b->settled + first, 0xFF, sizeof(int64_t) * (size_t)n, b->stream));
    if (b->cycles) {
        HIPCHK(hipMemsetAsync(b->cycles + first, 0, sizeof(int64_t) * (size_t)n, b->stream));
        HIPCHK(hipMemsetAsync(b->cycles + b->count + first, 0xFF, sizeof(int64_t) * (size_t)n, b->stream));
    }
    if (b->onsets) HIPCHK(hipMemsetAsync(b->onsets + first, 0xFF, sizeof(int64_t) * (size_t)n, b->stream));
    return LIFE_OK;
}

// the largest state count of the batch's universes, and the state count of one
uint32_t max_states(const life_batch *b) {
    if (b->shadow.empty()) return b->states;
    uint32_t c = life::kGenMaxStates;
    while (c > 2 && b->hist[c] == 0) --c;
    return c;
}
uint32_t states_of(const life_batch *b, int64_t u) { return b->shadow.empty() ? b->states : b->shadow[(size_t)u]; }

// the dying cells of universes [first, first + n) to dead, in every plane
int clear_decay(life_batch *b, int64_t first, int64_t n) {
    if (!b->decay || n < 1) return LIFE_OK;
    const size_t plane = words_of(b, b->count);
    for (int p = 0; p < b->planes; p++)
        HIPCHK(hipMemsetAsync(b->decay + (size_t)p * plane + words_of(b, first), 0, 4 * words_of(b, n), b->stream));
    return LIFE_OK;
}

// at least `need` decay planes: the new ones zero, the old ones kept (plane-major: they are a prefix)
int grow_decay(life_batch *b, int need) {
    if (b->planes >= need) return LIFE_OK;
    const size_t plane = 4 * words_of(b, b->count);
    uint32_t *grown = nullptr;
    HIPCHK(hipMalloc(&grown, plane * (size_t)need));
    hipError_t e = hipMemsetAsync(grown, 0, plane * (size_t)need, b->stream);
    if (e == hipSuccess && b->planes)
        e = hipMemcpyAsync(grown, b->decay, plane * (size_t)b->planes, hipMemcpyDeviceToDevice, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) {
        (void)hipFree(grown);
        HIPCHK(e);
    }
    if (b->decay) HIPCHK(hipFree(b->decay));
    b->decay = grown;
    b->planes = need;
    return LIFE_OK;
}

// the batch is two-state again: the planes are released
int drop_decay(life_batch *b) {
    if (!b->decay) return LIFE_OK;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipFree(b->decay));
    b->decay = nullptr;
    b->planes = 0;
    return LIFE_OK;
}

// bits above 8 and B0, as life_batch_set_rule refuses them; `at` >= 0: an entry of `call` (life_batch_set_rules
// or its _gen form)
int rule_ok(uint32_t birth, uint32_t survive, int64_t at, const char *call = "life_batch_set_rules") {
    char where[56] = "";
    if (at >= 0) snprintf(where, sizeof where, "%s: entry %lld: ", call, (long long)at);
    if ((birth | survive) & ~life::kRuleMask) {
        set_err("%srule masks 0x%x / 0x%x: bits above 8", where, birth, survive);
        return LIFE_EINVAL;
    }
    if (birth & 1u) {
        char name[24];
        life::rule_format(birth, survive, name);
        set_err("%srule %s: B0 rules are not supported (padding bits and idle lanes must stay dead)", where, name);
        return LIFE_EINVAL;
    }
    return LIFE_OK;
}

// the trace buffer is released (the stream may still write it)
int drop_trace(life_batch *b) {
    b->trace_gens = 0;
    if (!b->trace) return LIFE_OK;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipFree(b->trace));
    b->trace = nullptr;
    b->trace_cap = 0;
    return LIFE_OK;
}

// at least `entries` entries of trace; what an older buffer held is lost
int grow_trace(life_batch *b, int64_t entries) {
    if (b->trace_cap >= entries) return LIFE_OK;
    CHK(drop_trace(b));
    HIPCHK(hipMalloc(&b->trace, sizeof(uint32_t) * (size_t)entries));
    b->trace_cap = entries;
    return LIFE_OK;
}

// a rule of more than two states while LIFE_BATCH_OPT_POPULATION is on
int population_refuses(const char *call) {
    set_err("%s: LIFE_BATCH_OPT_POPULATION is on, and a population trace counts two-state universes only (turn it "
            "off before a Generations rule)", call);
    return LIFE_EINVAL;
}

// the table of a mixed batch is released: the batch is uniform again
int drop_rules(life_batch *b) {
    b->shadow.clear();
    b->shadow.shrink_to_fit();
    if (!b->rules) return LIFE_OK;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipFree(b->rules));
    b->rules = nullptr;
    return LIFE_OK;
}

void free_batch(life_batch *b) {
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->cells) (void)hipFree(b->cells);
    if (b->settled) (void)hipFree(b->settled);
    if (b->rules) (void)hipFree(b->rules);
    if (b->cycles) (void)hipFree(b->cycles);
    if (b->onsets) (void)hipFree(b->onsets);
    if (b->decay) (void)hipFree(b->decay);
    if (b->trace) (void)hipFree(b->trace);
    if (b->census) (void)hipFree(b->census);
    if (b->census_gen) (void)hipFree(b->census_gen);
    if (b->stage) (void)hipFree(b->stage);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int create(life_batch *b) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
        set_err("no HIP device: %s", hipGetErrorString(e));
        return LIFE_EHIP;
    }
    if (b->device < 0 || b->device >= ndev) {
        set_err("batch: device %d of %d", b->device, ndev);
        return LIFE_EHIP;
    }
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    const size_t bytes = (size_t)b->plan.bytes * (size_t)b->count;
    HIPCHK(hipMalloc(&b->cells, bytes));
    HIPCHK(hipMalloc(&b->settled, sizeof(int64_t) * (size_t)b->count));
    HIPCHK(hipMalloc(&b->census, 2 * sizeof(unsigned long long) * (size_t)b->count));
    HIPCHK(hipMemsetAsync(b->cells, 0, bytes, b->stream));
    CHK(clear_settled(b, 0, b->count));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

// states outside 2 .. 16, and more than two on a group-tier batch; `at` as rule_ok's
int states_ok(const life_batch *b, uint32_t birth, uint32_t survive, uint32_t states, int64_t at, const char *call) {
    char where[56] = "";
    if (at >= 0) snprintf(where, sizeof where, "%s: entry %lld: ", call, (long long)at);
    if (states < 2 || states > life::kGenMaxStates) {
        char name[24];
        life::rule_format(birth, survive, name);
        set_err("%srule %s with %u states (2 .. %u)", where, name, states, life::kGenMaxStates);
        return LIFE_EINVAL;
    }
    if (states > 2 && b->plan.tier != LIFE_BATCH_TIER_WAVE) {
        char name[32];
        life::rule_format_gen(birth, survive, states, name);
        set_err("%srule %s: a group-tier batch (%lld x %lld) has two states (Generations rules are a feature of the "
                "wave tier)", where, name, (long long)b->nx, (long long)b->ny);
        return LIFE_EINVAL;
    }
    return LIFE_OK;
}

// life_batch_set_rules (states null: two each) and life_batch_set_rules_gen
int set_rules(life_batch *b, int64_t first, int64_t n, const uint32_t *birth, const uint32_t *survive,
              const uint32_t *states, const char *call) {
    if (!b) return LIFE_EINVAL;
    CHK(range_ok(b, first, n, birth && survive ? (const void *)birth : nullptr, call));
    if (n == 0) return LIFE_OK;
    const bool wave = b->plan.tier == LIFE_BATCH_TIER_WAVE;
    uint32_t most = 2;
    for (int64_t k = 0; k < n; k++) {
        CHK(rule_ok(birth[k], survive[k], k, call));
        if (states) CHK(states_ok(b, birth[k], survive[k], states[k], k, call));
        if (states && states[k] > most) most = states[k];
        if (!wave && (birth[k] != life::kConwayBirth || survive[k] != life::kConwaySurvive)) {
            char name[24];
            life::rule_format(birth[k], survive[k], name);
            set_err("%s: entry %lld: rule %s: a group-tier batch (%lld x %lld) runs B3/S23 only "
                    "(rules are a feature of the wave tier)", call, (long long)k, name, (long long)b->nx,
                    (long long)b->ny);
            return LIFE_EINVAL;
        }
    }
    if (most > 2 && b->population) return population_refuses(call);
    HIPCHK(hipSetDevice(b->device));
    if (wave) {
        CHK(grow_decay(b, life::gen_planes(most)));
        // the first call lays the whole table down: the uniform rule, then the range
        const bool fresh = !b->rules;
        const int64_t lo = fresh ? 0 : first, m = fresh ? b->count : n;
        std::vector<uint32_t> host((size_t)(2 * m));
        uint32_t *table = b->rules;
        if (fresh) {
            HIPCHK(hipMalloc(&table, 2 * sizeof(uint32_t) * (size_t)b->count));
            for (int64_t u = 0; u < m; u++) {
                host[2 * u] = b->birth | b->states << 16;
                host[2 * u + 1] = b->survive;
            }
        }
        for (int64_t k = 0; k < n; k++) {
            host[2 * (first - lo + k)] = birth[k] | (states ? states[k] : 2u) << 16;
            host[2 * (first - lo + k) + 1] = survive[k];
        }
        // waited for: `host` leaves scope, and a table that did not arrive is not kept
        hipError_t e = hipMemcpyAsync(table + 2 * lo, host.data(), sizeof(uint32_t) * host.size(),
                                      hipMemcpyHostToDevice, b->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
        if (e != hipSuccess && fresh) (void)hipFree(table);
        HIPCHK(e);
        b->rules = table;
        if (fresh) {
            b->shadow.assign((size_t)b->count, (uint8_t)b->states);
            for (int64_t &h : b->hist) h = 0;
            b->hist[b->states] = b->count;
        }
        for (int64_t k = 0; k < n; k++) {
            uint8_t &c = b->shadow[(size_t)(first + k)];
            b->hist[c]--;
            c = (uint8_t)(states ? states[k] : 2u);
            b->hist[c]++;
        }
        CHK(clear_decay(b, first, n));
        return clear_settled(b, first, n);
    }
    return clear_settled(b, first, n);
}

int get_rules(life_batch *b, int64_t first, int64_t n, uint32_t *birth, uint32_t *survive, uint32_t *states,
              const char *call) {
    if (!b) return LIFE_EINVAL;
    CHK(range_ok(b, first, n, b, call));
    if (n == 0) return LIFE_OK;
    if (!b->rules) {
        for (int64_t k = 0; k < n; k++) {
            if (birth) birth[k] = b->birth;
            if (survive) survive[k] = b->survive;
            if (states) states[k] = b->states;
        }
        return LIFE_OK;
    }
    HIPCHK(hipSetDevice(b->device));
    std::vector<uint32_t> host((size_t)(2 * n));
    HIPCHK(hipMemcpyAsync(host.data(), b->rules + 2 * first, sizeof(uint32_t) * host.size(), hipMemcpyDeviceToHost,
                          b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int64_t k = 0; k < n; k++) {
        if (birth) birth[k] = host[2 * k] & 0xFFFFu;  // (the state count rides in the high half)
        if (survive) survive[k] = host[2 * k + 1];
        if (states) states[k] = host[2 * k] >> 16;
    }
    return LIFE_OK;
}

}  // namespace

extern "C" {

int life_batch_create(int64_t nx, int64_t ny, int64_t count, int device, life_batch **out) {
    if (!out) return LIFE_EINVAL;
    *out = nullptr;
    const life::BatchPlan p = life::batch_plan(nx, ny);
    if (p.tier == 0) {
        set_err("%s", p.why);
        return LIFE_EINVAL;
    }
    // one workgroup per universe (group tier) must fit the grid's x
    if (count < 1 || count > INT_MAX) {
        set_err("batch: count %lld (1 .. %d)", (long long)count, INT_MAX);
        return LIFE_EINVAL;
    }
    life_batch *b = new life_batch;
    b->nx = nx;
    b->ny = ny;
    b->count = count;
    b->device = device;
    b->plan = p;
    const int rc = create(b);
    if (rc != LIFE_OK) {
        free_batch(b);
        return rc;
    }
    *out = b;
    return LIFE_OK;
}

void life_batch_destroy(life_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    free_batch(b);
}

int life_batch_upload(life_batch *b, int64_t first, int64_t n, const uint8_t *grids) {
    if (!b) return LIFE_EINVAL;
    CHK(range_ok(b, first, n, grids, "life_batch_upload"));
    if (n == 0) return LIFE_OK;
    HIPCHK(hipSetDevice(b->device));
    const size_t bytes = (size_t)n * (size_t)(b->nx * b->ny);
    CHK(stage_for(b, bytes));
    // `grids` is the caller's pageable memory: the copy is waited for before
    // this call returns, so the caller may reuse it at once
    HIPCHK(hipMemcpyAsync(b->stage, grids, bytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(life::launch_batch_import(b->plan, b->nx, b->ny, n, b->stage, b->cells + words_of(b, first), b->stream));
    CHK(clear_decay(b, first, n));
    CHK(clear_settled(b, first, n));
    b->census_valid = false;
    if (n == b->count) b->generation = 0;
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_gather(life_batch *b, int64_t first, int64_t n, uint8_t *grids) {
    if (!b) return LIFE_EINVAL;
    CHK(range_ok(b, first, n, grids, "life_batch_gather"));
    if (n == 0) return LIFE_OK;
    HIPCHK(hipSetDevice(b->device));
    const size_t bytes = (size_t)n * (size_t)(b->nx * b->ny);
    CHK(stage_for(b, bytes));
    HIPCHK(life::launch_batch_export(b->plan, b->nx, b->ny, n, b->cells + words_of(b, first), b->stage, b->stream));
    HIPCHK(hipMemcpyAsync(grids, b->stage, bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_fill_random(life_batch *b, uint64_t seed, uint32_t thr32) {
    if (!b) return LIFE_EINVAL;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(life::launch_batch_fill(b->plan, b->nx, b->ny, b->count, seed, thr32, b->cells, b->stream));
    CHK(clear_decay(b, 0, b->count));
    CHK(clear_settled(b, 0, b->count));
    b->census_valid = false;
    b->generation = 0;
    return LIFE_OK;
}

int life_batch_set_rule(life_batch *b, uint32_t birth, uint32_t survive) {
    if (!b) return LIFE_EINVAL;
    CHK(rule_ok(birth, survive, -1));
    char name[24];
    life::rule_format(birth, survive, name);
    const bool conway = birth == life::kConwayBirth && survive == life::kConwaySurvive;
    if (!conway && b->plan.tier != LIFE_BATCH_TIER_WAVE) {
        set_err("rule %s: a group-tier batch (%lld x %lld) runs B3/S23 only (rules are a feature of the wave tier)", name,
                (long long)b->nx, (long long)b->ny);
        return LIFE_EINVAL;
    }
    HIPCHK(hipSetDevice(b->device));
    CHK(drop_rules(b));
    CHK(drop_decay(b));
    CHK(clear_settled(b, 0, b->count));
    b->birth = birth;
    b->survive = survive;
    b->states = 2;
    b->table = !conway;
    if (b->table) b->words = life::rule_words(birth, survive);
    return LIFE_OK;
}

int life_batch_get_rule(life_batch *b, uint32_t *birth, uint32_t *survive) {
    if (!b) return LIFE_EINVAL;
    if (b->rules) {
        set_err("life_batch_get_rule: the batch holds a rule per universe (life_batch_set_rules): ask "
                "life_batch_get_rules");
        return LIFE_ESTATE;
    }
    if (b->states > 2) {
        set_err("life_batch_get_rule: the batch runs a Generations rule of %u states (life_batch_set_rule_gen): ask "
                "life_batch_get_rule_gen", b->states);
        return LIFE_ESTATE;
    }
    if (birth) *birth = b->birth;
    if (survive) *survive = b->survive;
    return LIFE_OK;
}

int life_batch_set_rules(life_batch *b, int64_t first, int64_t n, const uint32_t *birth, const uint32_t *survive) {
    return set_rules(b, first, n, birth, survive, nullptr, "life_batch_set_rules");
}

int life_batch_get_rules(life_batch *b, int64_t first, int64_t n, uint32_t *birth, uint32_t *survive) {
    return get_rules(b, first, n, birth, survive, nullptr, "life_batch_get_rules");
}

int life_batch_set_rule_gen(life_batch *b, uint32_t birth, uint32_t survive, uint32_t states) {
    if (!b) return LIFE_EINVAL;
    CHK(rule_ok(birth, survive, -1));
    CHK(states_ok(b, birth, survive, states, -1, "life_batch_set_rule_gen"));
    if (states == 2) return life_batch_set_rule(b, birth, survive);
    if (b->population) return population_refuses("life_batch_set_rule_gen");
    HIPCHK(hipSetDevice(b->device));
    CHK(grow_decay(b, life::gen_planes(states)));
    CHK(drop_rules(b));
    CHK(clear_decay(b, 0, b->count));
    CHK(clear_settled(b, 0, b->count));
    b->birth = birth;
    b->survive = survive;
    b->states = states;
    b->table = true;  // (what a return to two states by life_batch_set_rule recomputes)
    b->words = life::rule_words(birth, survive);
    return LIFE_OK;
}

int life_batch_get_rule_gen(life_batch *b, uint32_t *birth, uint32_t *survive, uint32_t *states) {
    if (!b) return LIFE_EINVAL;
    if (b->rules) {
        set_err("life_batch_get_rule_gen: the batch holds a rule per universe (life_batch_set_rules): ask "
                "life_batch_get_rules_gen");
        return LIFE_ESTATE;
    }
    if (birth) *birth = b->birth;
    if (survive) *survive = b->survive;
    if (states) *states = b->states;
    return LIFE_OK;
}

int life_batch_set_rules_gen(life_batch *b, int64_t first, int64_t n, const uint32_t *birth, const uint32_t *survive,
                             const uint32_t *states) {
    if (!b) return LIFE_EINVAL;
    if (n > 0 && !states) {
        set_err("life_batch_set_rules_gen: no states");
        return LIFE_EINVAL;
    }
    return set_rules(b, first, n, birth, survive, states, "life_batch_set_rules_gen");
}

int life_batch_get_rules_gen(life_batch *b, int64_t first, int64_t n, uint32_t *birth, uint32_t *survive,
                             uint32_t *states) {
    return get_rules(b, first, n, birth, survive, states, "life_batch_get_rules_gen");
}

int life_batch_upload_states(life_batch *b, int64_t first, int64_t n, const uint8_t *grids) {
    if (!b) return LIFE_EINVAL;
    CHK(range_ok(b, first, n, grids, "life_batch_upload_states"));
    if (n == 0) return LIFE_OK;
    const size_t cells = (size_t)(b->nx * b->ny);
    for (int64_t k = 0; k < n; k++) {
        const uint32_t c = states_of(b, first + k);
        const uint8_t *g = grids + (size_t)k * cells;
        for (size_t i = 0; i < cells; i++)
            if (g[i] >= c) {
                set_err("life_batch_upload_states: universe %lld: cell (%lld, %lld) holds %u, its rule has %u states",
                        (long long)(first + k), (long long)(i % (size_t)b->nx), (long long)(i / (size_t)b->nx), g[i],
                        c);
                return LIFE_EINVAL;
            }
    }
    if (!b->decay) return life_batch_upload(b, first, n, grids);  // every byte is 0 or 1
    HIPCHK(hipSetDevice(b->device));
    const size_t bytes = (size_t)n * cells;
    CHK(stage_for(b, bytes));
    HIPCHK(hipMemcpyAsync(b->stage, grids, bytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(life::launch_batch_import_states(b->plan, b->nx, b->ny, b->count, first, n, b->stage, b->cells, b->decay,
                                            b->planes, b->stream));
    CHK(clear_settled(b, first, n));
    b->census_valid = false;
    if (n == b->count) b->generation = 0;
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_gather_states(life_batch *b, int64_t first, int64_t n, uint8_t *grids) {
    if (!b) return LIFE_EINVAL;
    CHK(range_ok(b, first, n, grids, "life_batch_gather_states"));
    if (n == 0) return LIFE_OK;
    if (!b->decay) return life_batch_gather(b, first, n, grids);
    HIPCHK(hipSetDevice(b->device));
    const size_t bytes = (size_t)n * (size_t)(b->nx * b->ny);
    CHK(stage_for(b, bytes));
    HIPCHK(life::launch_batch_export_states(b->plan, b->nx, b->ny, b->count, first, n, b->cells, b->decay, b->planes,
                                            b->stage, b->stream));
    HIPCHK(hipMemcpyAsync(grids, b->stage, bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_census_gen(life_batch *b, int64_t *live, int64_t *dying, uint64_t *checksum) {
    if (!b) return LIFE_EINVAL;
    HIPCHK(hipSetDevice(b->device));
    const size_t bytes = sizeof(unsigned long long) * (size_t)b->count;
    if (!b->census_gen) HIPCHK(hipMalloc(&b->census_gen, 3 * bytes));
    unsigned long long *d_live = b->census_gen, *d_dying = d_live + b->count, *d_sum = d_dying + b->count;
    // (not cached: a call costs one pass over the planes)
    HIPCHK(life::launch_batch_census_states(b->plan, b->nx, b->ny, b->count, b->cells, b->decay, b->planes, d_live,
                                            d_dying, d_sum, b->stream));
    if (live) HIPCHK(hipMemcpyAsync(live, d_live, bytes, hipMemcpyDeviceToHost, b->stream));
    if (dying) HIPCHK(hipMemcpyAsync(dying, d_dying, bytes, hipMemcpyDeviceToHost, b->stream));
    if (checksum) HIPCHK(hipMemcpyAsync(checksum, d_sum, bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_configure(life_batch *b, int option, int value) {
    if (!b) return LIFE_EINVAL;
    // (option 2 is unassigned)
    if ((option != LIFE_BATCH_OPT_SETTLE && option != LIFE_BATCH_OPT_CYCLE && option != LIFE_BATCH_OPT_POPULATION &&
         option != LIFE_BATCH_OPT_ONSET) ||
        (value != 0 && value != 1)) {
        set_err("life_batch_configure: option %d value %d", option, value);
        return LIFE_EINVAL;
    }
    if (option == LIFE_BATCH_OPT_POPULATION) {  // both tiers
        if (value && max_states(b) > 2) {
            set_err("LIFE_BATCH_OPT_POPULATION: the batch runs a Generations rule of %u states (life_batch_set_rule_gen "
                    "/ life_batch_set_rules_gen), and a population trace counts two-state universes only",
                    max_states(b));
            return LIFE_EINVAL;
        }
        if (!value) {
            HIPCHK(hipSetDevice(b->device));
            CHK(drop_trace(b));
        }
        b->population = value != 0;
        return LIFE_OK;
    }
    const bool settle = option == LIFE_BATCH_OPT_SETTLE, onset = option == LIFE_BATCH_OPT_ONSET;
    const char *name = settle ? "LIFE_BATCH_OPT_SETTLE" : onset ? "LIFE_BATCH_OPT_ONSET" : "LIFE_BATCH_OPT_CYCLE";
    if (b->plan.tier != LIFE_BATCH_TIER_WAVE) {
        set_err("%s: a group-tier batch (%lld x %lld) has no %s detection", name, (long long)b->nx, (long long)b->ny,
                settle ? "settle" : "cycle");
        return LIFE_EINVAL;
    }
    if (onset) {  // the second phase of the cycle detection: it acts with that option only
        if (value && !b->cycle) {
            set_err("%s: LIFE_BATCH_OPT_CYCLE is off (the onset is computed by the wave that finds the period: turn "
                    "that option on first)", name);
            return LIFE_EINVAL;
        }
        if (value && !b->onsets) {
            HIPCHK(hipSetDevice(b->device));
            HIPCHK(hipMalloc(&b->onsets, sizeof(int64_t) * (size_t)b->count));
            HIPCHK(hipMemsetAsync(b->onsets, 0xFF, sizeof(int64_t) * (size_t)b->count, b->stream));
        }
        b->onset = value != 0;
        return LIFE_OK;
    }
    if (value && (settle ? b->cycle : b->settle)) {
        set_err("%s: %s is on (two detectors for one wave: turn that one off first)", name,
                settle ? "LIFE_BATCH_OPT_CYCLE" : "LIFE_BATCH_OPT_SETTLE");
        return LIFE_EINVAL;
    }
    if (settle) {
        b->settle = value != 0;
        return LIFE_OK;
    }
    if (value && !b->cycles) {
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipMalloc(&b->cycles, 2 * sizeof(int64_t) * (size_t)b->count));
        // the new pairs to 0 / -1 (the settled flags are not this option's)
        const size_t bytes = sizeof(int64_t) * (size_t)b->count;
        HIPCHK(hipMemsetAsync(b->cycles, 0, bytes, b->stream));
        HIPCHK(hipMemsetAsync(b->cycles + b->count, 0xFF, bytes, b->stream));
    }
    b->cycle = value != 0;
    if (!b->cycle) b->onset = false;  // (nothing left to find an onset for)
    return LIFE_OK;
}

int life_batch_step(life_batch *b, int64_t generations) {
    if (!b) return LIFE_EINVAL;
    if (generations < 0 || generations > INT32_MAX) {
        set_err("life_batch_step: %lld generations (0 .. %d)", (long long)generations, INT32_MAX);
        return LIFE_EINVAL;
    }
    if (b->population && generations > life::kBatchTraceEntries / b->count) {
        set_err("life_batch_step: LIFE_BATCH_OPT_POPULATION would record %lld universes x %lld generations, more than "
                "%lld entries: split the call", (long long)b->count, (long long)generations,
                (long long)life::kBatchTraceEntries);
        return LIFE_EINVAL;
    }
    if (generations == 0) {
        b->trace_gens = 0;  // (a call that recorded nothing)
        return LIFE_OK;
    }
    HIPCHK(hipSetDevice(b->device));
    const uint32_t most = max_states(b);
    int64_t *const found = b->cycles ? b->cycles + b->count : nullptr;
    const bool onset = b->cycle && b->onset;  // (wave tier: the options are refused elsewhere)
    if (b->population) {  // (two-state: the option and the Generations rules refuse each other)
        CHK(grow_trace(b, b->count * generations));
        b->trace_gens = 0;
        if (onset)
            HIPCHK(life::launch_batch_onset(b->plan, b->nx, b->ny, b->count, b->cells, generations,
                                            b->table ? &b->words : nullptr, b->rules, b->cycles, found, b->onsets,
                                            b->generation, b->trace, b->stream));
        else if (b->plan.tier == LIFE_BATCH_TIER_WAVE)
            HIPCHK(life::launch_batch_trace(b->plan, b->nx, b->ny, b->count, b->cells, generations,
                                            b->table ? &b->words : nullptr, b->rules, b->settle, b->settled, b->cycle,
                                            b->cycles, found, b->generation, b->trace, b->stream));
        else
            HIPCHK(life::launch_batch_group_trace(b->plan, b->nx, b->ny, b->count, b->cells, generations, b->trace,
                                                  b->stream));
        b->trace_gens = generations;
    } else if (most > 2 && onset)
        HIPCHK(life::launch_batch_onset_gen(b->plan, b->nx, b->ny, b->count, b->cells, b->decay, life::gen_planes(most),
                                            generations, b->birth, b->survive, b->states, b->rules, b->cycles, found,
                                            b->onsets, b->generation, b->stream));
    else if (most > 2)  // (wave tier: no other takes such a rule)
        HIPCHK(life::launch_batch_gen(b->plan, b->nx, b->ny, b->count, b->cells, b->decay, life::gen_planes(most),
                                      generations, b->birth, b->survive, b->states, b->rules, b->settle, b->settled,
                                      b->cycle, b->cycles, b->cycles ? b->cycles + b->count : nullptr, b->generation,
                                      b->stream));
    else if (onset)
        HIPCHK(life::launch_batch_onset(b->plan, b->nx, b->ny, b->count, b->cells, generations,
                                        b->table ? &b->words : nullptr, b->rules, b->cycles, found, b->onsets,
                                        b->generation, nullptr, b->stream));
    else if (b->plan.tier == LIFE_BATCH_TIER_WAVE && (b->rules || b->cycle))
        HIPCHK(life::launch_batch_survey(b->plan, b->nx, b->ny, b->count, b->cells, generations,
                                         b->table ? &b->words : nullptr, b->rules, b->settle, b->settled, b->cycle,
                                         b->cycles, b->cycles ? b->cycles + b->count : nullptr, b->generation,
                                         b->stream));
    else if (b->plan.tier == LIFE_BATCH_TIER_WAVE)
        HIPCHK(life::launch_batch_wave(b->plan, b->nx, b->ny, b->count, b->cells, generations,
                                       b->table ? &b->words : nullptr, b->settle, b->settled, b->generation,
                                       b->stream));
    else
        HIPCHK(life::launch_batch_group(b->plan, b->nx, b->ny, b->count, b->cells, generations, b->stream));
    b->generation += generations;
    b->census_valid = false;
    return LIFE_OK;
}

int life_batch_census(life_batch *b, int64_t *live, uint64_t *checksum) {
    if (!b) return LIFE_EINVAL;
    HIPCHK(hipSetDevice(b->device));
    unsigned long long *d_live = b->census, *d_sum = b->census + b->count;
    if (!b->census_valid) {
        HIPCHK(life::launch_batch_census(b->plan, b->nx, b->ny, b->count, b->cells, d_live, d_sum, b->stream));
        b->census_valid = true;
    }
    const size_t bytes = sizeof(unsigned long long) * (size_t)b->count;
    if (live) HIPCHK(hipMemcpyAsync(live, d_live, bytes, hipMemcpyDeviceToHost, b->stream));
    if (checksum) HIPCHK(hipMemcpyAsync(checksum, d_sum, bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_population(life_batch *b, int64_t first, int64_t n, uint32_t *counts, int64_t *generations) {
    if (!b) return LIFE_EINVAL;
    CHK(range_ok(b, first, n, b, "life_batch_population"));
    const int64_t gens = b->population ? b->trace_gens : 0;
    if (generations) *generations = gens;
    if (!counts || n == 0 || gens == 0) return LIFE_OK;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(counts, b->trace + (size_t)first * (size_t)gens, sizeof(uint32_t) * (size_t)(n * gens),
                          hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_settled(life_batch *b, int64_t *generation) {
    if (!b || !generation) return LIFE_EINVAL;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(generation, b->settled, sizeof(int64_t) * (size_t)b->count, hipMemcpyDeviceToHost,
                          b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_cycles(life_batch *b, int64_t *period, int64_t *generation) {
    if (!b) return LIFE_EINVAL;
    if (!b->cycles) {  // LIFE_BATCH_OPT_CYCLE was never on
        for (int64_t u = 0; u < b->count; u++) {
            if (period) period[u] = 0;
            if (generation) generation[u] = -1;
        }
        return LIFE_OK;
    }
    HIPCHK(hipSetDevice(b->device));
    const size_t bytes = sizeof(int64_t) * (size_t)b->count;
    if (period) HIPCHK(hipMemcpyAsync(period, b->cycles, bytes, hipMemcpyDeviceToHost, b->stream));
    if (generation) HIPCHK(hipMemcpyAsync(generation, b->cycles + b->count, bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_onsets(life_batch *b, int64_t *generation) {
    if (!b || !generation) return LIFE_EINVAL;
    if (!b->onsets) {  // LIFE_BATCH_OPT_ONSET was never on
        for (int64_t u = 0; u < b->count; u++) generation[u] = -1;
        return LIFE_OK;
    }
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(generation, b->onsets, sizeof(int64_t) * (size_t)b->count, hipMemcpyDeviceToHost,
                          b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

int life_batch_generation(life_batch *b, int64_t *generation) {
    if (!b || !generation) return LIFE_EINVAL;
    *generation = b->generation;
    return LIFE_OK;
}

int life_batch_sync(life_batch *b) {
    if (!b) return LIFE_EINVAL;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    return LIFE_OK;
}

}  // extern "C"
