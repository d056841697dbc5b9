// life_batch_kernels.hip -- the kernels of life_batch (gfx950): many
// independent small periodic universes of one shape, stepped in one launch
// (DESIGN.md 5.11).
//
// Storage (the batch's own): natural 32-cell words, bit k of word j = cell
// 32j + k, W = ceil(nx/32) words per row, ny rows, universes W * ny words
// apart; no aprons, no pair interleave: every wrap happens in the kernels.
// The bits at and beyond nx of a row's last word are zero after every writer.
// A step call reads a universe into registers once and writes it back in place
// at the end: exactly one wave (wave tier) or workgroup (group tier) owns it.
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>

#include "life_batch_kernels.h"
#include "life_bitops.h"

namespace life {
namespace {

constexpr uint32_t kKeepMux = ((0xF0 & 0xCC) | (~0xCC & 0xAA)) & 0xFF;  // (a & b) | (c & ~b)

// The x wrap of a row whose last word holds q = nx - 32 (W - 1) cells, 1 <= q
// <= 32 (lane-uniform).  Word 0's left neighbour word must carry cell nx - 1 at
// bit 31: the last word shifted up by lsh.  The last word takes cell 0 at bit
// q before the sums (qs; above it: don't-care bits, masked off by `keep` after
// the rule), and word 0 as its right neighbour word when q == 32.
struct XWrap {
    uint32_t keep, lsh, qs;
    __device__ __forceinline__ explicit XWrap(int nx, int W) {
        const int q = nx - 32 * (W - 1);
        keep = q < 32 ? (1u << q) - 1u : 0xFFFFFFFFu;
        lsh = (uint32_t)((32 - q) & 31);
        qs = (uint32_t)(q & 31);
    }
};

template <class RP>
__device__ __forceinline__ RP make_rule(const RuleWords &w);
template <>
__device__ __forceinline__ ConwayRule make_rule<ConwayRule>(const RuleWords &) {
    return ConwayRule{};
}
template <>
__device__ __forceinline__ TableRule make_rule<TableRule>(const RuleWords &w) {
    return TableRule(w);
}

// ------------------------------------------------------------------ wave tier
// One universe per wave, one row per lane (ny <= 64), the row's W <= 4 words in
// registers.  A generation: per word the 2-bit horizontal sums (the neighbour
// words are the lane's own registers: two funnel shifts and a full adder; the
// x wrap as XWrap), the sums of the rows above and below by ds_bpermute from
// the lanes (y - 1) mod ny and (y + 1) mod ny (four per word), the rule.  No
// LDS allocation, no barrier: the waves of a workgroup never meet.  Lanes at
// and beyond ny hold zeros and read themselves, so they stay zero under any
// rule without B0 and a wave-wide vote sees the universe alone.
struct BWArgs {
    uint32_t *cells;
    int64_t *settled;
    int64_t count, gen0;
    int32_t nx, ny, gens;
    RuleWords rule;
    const uint2 *rules;        // per-universe forms: (birth, survive) of universe u
    int64_t *period, *found;   // cycle detection: 0 / -1, or the period and the generation it was found at
    uint32_t *trace;           // the recording forms: a.gens entries per universe, universe-major
};

// what a wave watches its universe for (LIFE_BATCH_OPT_SETTLE, LIFE_BATCH_OPT_CYCLE)
enum Detector { kNoDetector = 0, kSettle = 1, kCycle = 2 };

// The sum of x over the 64 lanes (every lane enabled), wave-uniform: four
// row_shr adds leave a row's total in its lane 15, row_bcast:15 and
// row_bcast:31 carry the totals up to lane 63.
// (a lane the control or the row mask leaves without a source adds zero)
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_from(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xf, true);
}
// the totals of the four 16-lane rows, each in its lane 15
__device__ __forceinline__ uint32_t row_totals(uint32_t x) {
    x += dpp_from<0x111, 0xf>(x);  // row_shr:1
    x += dpp_from<0x112, 0xf>(x);  // row_shr:2
    x += dpp_from<0x114, 0xf>(x);  // row_shr:4
    x += dpp_from<0x118, 0xf>(x);  // row_shr:8
    return x;
}
__device__ __forceinline__ uint32_t wave_total(uint32_t x) {
    x = row_totals(x);
    x += dpp_from<0x142, 0xa>(x);  // row_bcast:15 into rows 1 and 3
    x += dpp_from<0x143, 0xc>(x);  // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// The population trace of a wave (LIFE_BATCH_OPT_POPULATION):
// the live cells of its universe after every generation, kept in registers and
// flushed every kTraceFlush generations.  A wave-tier total is at most 128 x
// 64 = 8192, so two generations ride the halves of one dword through one
// wave_total: the lanes' counts of an even pending generation wait in `half`,
// the odd one joins them above bit 16, and lane k keeps the totals of pending
// generations 2 k and 2 k + 1 in `pend`.
constexpr int kTraceFlush = 128;

struct WaveTrace {
    uint32_t *at;  // the next entry to flush
    uint32_t half = 0, pend = 0;
    int k = 0;  // pending generations (wave-uniform)
    int lane;
    __device__ __forceinline__ WaveTrace(uint32_t *to, int lane_) : at(to), lane(lane_) {}
    __device__ __forceinline__ void flush() {
        if (2 * lane < k) at[2 * lane] = pend & 0xFFFFu;
        if (2 * lane + 1 < k) at[2 * lane + 1] = pend >> 16;
        at += k;
        k = 0;
    }
    __device__ __forceinline__ void pair(uint32_t both) {
        const uint32_t total = wave_total(both);
        if (lane == k >> 1) pend = total;
    }
    // after a generation: `count` the live cells of this lane's row
    __device__ __forceinline__ void record(uint32_t count) {
        if (k & 1)
            pair(half | count << 16);
        else
            half = count;
        if (++k == kTraceFlush) flush();
    }
    __device__ __forceinline__ void finish() {
        if (k & 1) pair(half);
        flush();
    }
};

// One generation of K states held side by side in the same lanes, chain c's row
// in x[c W, c W + W): the definition of a generation for every two-state wave
// kernel.  K = 2 (the onset search) steps two independent
// states in one pass -- sums, lane moves and rules of both issued together --
// so one chain's ds_bpermute latency has the other's VALU to hide behind.
template <int W, int K, class RP>
__device__ __forceinline__ void wave_generations(uint32_t *x, const int addr_up, const int addr_dn, const XWrap &xw,
                                                 const RP &rp) {
    uint32_t s0[K * W], s1[K * W];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const uint32_t *v = x + c * W;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t l = j == 0 ? v[W - 1] << xw.lsh : v[j - 1];
            const uint32_t r = j == W - 1 ? v[0] : v[j + 1];
            uint32_t m = v[j];
            if (j == W - 1) m = b3<kKeepMux>(m, xw.keep, v[0] << xw.qs);
            BitEnc::fa(__builtin_amdgcn_alignbit(m, l, 31), m, __builtin_amdgcn_alignbit(r, m, 1), s0[c * W + j],
                       s1[c * W + j]);
        }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const int i = c * W + j;
            const uint32_t a0 = bperm(addr_up, s0[i]), a1 = bperm(addr_up, s1[i]);
            const uint32_t d0 = bperm(addr_dn, s0[i]), d1 = bperm(addr_dn, s1[i]);
            x[i] = rp(a0, a1, s0[i], s1[i], d0, d1, x[i]);
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) x[c * W + W - 1] &= xw.keep;
}

// The whole life of a wave that owns universe u: load, a.gens generations under
// rp (fewer when the detector lets it leave early), store.  Shared by every
// wave-tier kernel.  POP: the recording forms.  Every generation of the call is
// computed and its live count recorded, whatever the detector finds or found
// in an earlier call: it flags what it flags without POP and the wave runs on.
template <int W, int DET, bool POP = false, class RP>
__device__ __forceinline__ void wave_body(const BWArgs &a, const int64_t u, const int lane, const RP &rp) {
    constexpr bool SETTLE = DET == kSettle, CYCLE = DET == kCycle;
    const int ny = a.ny;
    const bool active = lane < ny;
    const int up = !active ? lane : lane == 0 ? ny - 1 : lane - 1;
    const int dn = !active ? lane : lane + 1 == ny ? 0 : lane + 1;
    const int addr_up = up << 2, addr_dn = dn << 2;
    const XWrap xw(a.nx, W);
    uint32_t *row = a.cells + ((size_t)u * (size_t)ny + (size_t)lane) * W;

    uint32_t v[W];
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = active ? row[j] : 0u;

    int gens = a.gens;
    bool detect = false;
    if (SETTLE) {
        detect = a.settled[u] < 0;
        if (!detect && !POP) gens &= 1;  // settled in an earlier call: the state has period 1 or 2
    }
    uint32_t p1[SETTLE ? W : 1], p2[SETTLE ? W : 1];  // S_(g-1), S_(g-2)
    if (SETTLE) {
#pragma unroll
        for (int j = 0; j < W; ++j) p1[j] = p2[j] = v[j];
    }
    // Brent, restarted per call: T the checkpoint, lam generations since it, the
    // next one when lam reaches power (all wave-uniform)
    uint32_t T[CYCLE ? W : 1];
    uint32_t power = 1, lam = 0;
    if (CYCLE) {
        // (the same for every lane: tell the compiler so, and the loops below branch on scalars)
        const uint32_t known = __builtin_amdgcn_readfirstlane((uint32_t)a.period[u]);
        detect = known == 0u;
        if (!detect && !POP) gens = (int)((uint32_t)gens % known);  // found in an earlier call
#pragma unroll
        for (int j = 0; j < W; ++j) T[j] = v[j];
    }
    WaveTrace tr(POP ? a.trace + (size_t)u * (size_t)a.gens : nullptr, lane);
    // (wave_generations<W, 1> spelled out: the instances of this body keep the code they were measured with)
    auto generation = [&]() {
        uint32_t s0[W], s1[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t l = j == 0 ? v[W - 1] << xw.lsh : v[j - 1];
            const uint32_t r = j == W - 1 ? v[0] : v[j + 1];
            uint32_t c = v[j];
            if (j == W - 1) c = b3<kKeepMux>(c, xw.keep, v[0] << xw.qs);
            BitEnc::fa(__builtin_amdgcn_alignbit(c, l, 31), c, __builtin_amdgcn_alignbit(r, c, 1), s0[j], s1[j]);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t a0 = bperm(addr_up, s0[j]), a1 = bperm(addr_up, s1[j]);
            const uint32_t d0 = bperm(addr_dn, s0[j]), d1 = bperm(addr_dn, s1[j]);
            v[j] = rp(a0, a1, s0[j], s1[j], d0, d1, v[j]);
        }
        v[W - 1] &= xw.keep;
        if (POP) {
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) c += __popc(v[j]);
            tr.record(c);
        }
    };
    if (CYCLE) {
        // The detecting generations, then the rest without: what is recorded is
        // written between the two loops, so neither holds a memory access.
        int rest = gens, g = 1;
        if (detect) {
            for (; g <= gens; ++g) {
                generation();
                ++lam;
                uint32_t diff = 0;
#pragma unroll
                for (int j = 0; j < W; ++j) diff |= v[j] ^ T[j];
                if (__builtin_amdgcn_ballot_w64(diff != 0u) == 0ull) break;  // S_g == T: the minimal period is lam
                if (lam == power) {
#pragma unroll
                    for (int j = 0; j < W; ++j) T[j] = v[j];
                    power <<= 1;
                    lam = 0;
                }
            }
            rest = 0;
            if (g <= gens) {
                if (lane == 0) {
                    a.period[u] = (int64_t)lam;
                    a.found[u] = a.gen0 + g;
                }
                rest = POP ? gens - g : (int)((uint32_t)(gens - g) % lam);
            }
        }
        for (g = 0; g < rest; ++g) generation();
    }
    for (int g = 1; !CYCLE && g <= gens; ++g) {
        generation();
        if (SETTLE && detect) {
            if (g >= 2) {
                uint32_t diff = 0;
#pragma unroll
                for (int j = 0; j < W; ++j) diff |= v[j] ^ p2[j];
                if (__builtin_amdgcn_ballot_w64(diff != 0u) == 0ull) {  // S_g == S_(g-2), the whole wave agrees
                    if (lane == 0) a.settled[u] = a.gen0 + g;
                    detect = false;
                    if (!POP) gens = g + ((gens - g) & 1);
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) {
                p2[j] = p1[j];
                p1[j] = v[j];
            }
        }
    }
    if (POP) tr.finish();
    if (!active) return;
#pragma unroll
    for (int j = 0; j < W; ++j) row[j] = v[j];
}

// The uniform forms without cycle detection: one rule for the launch.
template <int W, class RP, bool SETTLE>
__global__ __launch_bounds__(64 * kBatchWaves) void batch_wave_kernel(BWArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + (int64_t)(threadIdx.x >> 6);
    if (u >= a.count) return;  // the whole wave
    const RP rp = make_rule<RP>(a.rule);
    wave_body<W, SETTLE ? kSettle : kNoDetector>(a, u, lane, rp);
}

template <int W, class RP>
hipError_t launch_wave(const BWArgs &a, bool settle, unsigned blocks, hipStream_t s) {
    if (settle)
        batch_wave_kernel<W, RP, true><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    else
        batch_wave_kernel<W, RP, false><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    return hipGetLastError();
}

// The survey forms: cycle detection under a uniform rule, and a
// rule per universe under any detector.  A per-universe wave reads its two
// masks once, before the generation loop, and expands them into the ten
// leaves of TableRule by life::rule_leaf -- the host's own definition -- so a
// B3/S23 universe of a mixed batch runs the table too.
enum SurveyRule { kSurveyConway = 0, kSurveyTable = 1, kSurveyPerUniverse = 2 };

// TableRule of universe u's own masks
__device__ __forceinline__ TableRule universe_rule(const uint2 *rules, int64_t u) {
    const uint2 m = rules[u];
    RuleWords w;
#pragma unroll
    for (int q = 0; q < 10; ++q) {
        const RuleLeaf leaf = rule_leaf(m.x, m.y, q / 5, q % 5);
        w.a[q / 5][q % 5] = leaf.a;
        w.b[q / 5][q % 5] = leaf.b;
    }
    return TableRule(w);
}

template <int W, int RULE, int DET>
__global__ __launch_bounds__(64 * kBatchWaves) void batch_survey_kernel(BWArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + (int64_t)(threadIdx.x >> 6);
    if (u >= a.count) return;  // the whole wave
    if (RULE == kSurveyConway)
        wave_body<W, DET>(a, u, lane, ConwayRule{});
    else if (RULE == kSurveyTable)
        wave_body<W, DET>(a, u, lane, TableRule(a.rule));
    else
        wave_body<W, DET>(a, u, lane, universe_rule(a.rules, u));
}

template <int W>
hipError_t launch_survey(const BWArgs &a, int rule, int det, unsigned blocks, hipStream_t s) {
#define LIFE_BS(R, D) batch_survey_kernel<W, R, D><<<blocks, 64 * kBatchWaves, 0, s>>>(a)
    if (rule == kSurveyPerUniverse) {
        if (det == kCycle)
            LIFE_BS(kSurveyPerUniverse, kCycle);
        else if (det == kSettle)
            LIFE_BS(kSurveyPerUniverse, kSettle);
        else
            LIFE_BS(kSurveyPerUniverse, kNoDetector);
    } else if (det != kCycle) {
        return hipErrorInvalidValue;  // the uniform forms without cycle detection are batch_wave_kernel's
    } else if (rule == kSurveyTable) {
        LIFE_BS(kSurveyTable, kCycle);
    } else {
        LIFE_BS(kSurveyConway, kCycle);
    }
#undef LIFE_BS
    return hipGetLastError();
}

// The recording forms: every two-state form of the wave tier,
// the uniform ones included, with the population trace of wave_body on.
template <int W, int RULE, int DET>
__global__ __launch_bounds__(64 * kBatchWaves) void batch_trace_kernel(BWArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + (int64_t)(threadIdx.x >> 6);
    if (u >= a.count) return;  // the whole wave
    if (RULE == kSurveyConway)
        wave_body<W, DET, true>(a, u, lane, ConwayRule{});
    else if (RULE == kSurveyTable)
        wave_body<W, DET, true>(a, u, lane, TableRule(a.rule));
    else
        wave_body<W, DET, true>(a, u, lane, universe_rule(a.rules, u));
}

template <int W, int RULE>
hipError_t launch_trace(const BWArgs &a, int det, unsigned blocks, hipStream_t s) {
    if (det == kCycle)
        batch_trace_kernel<W, RULE, kCycle><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    else if (det == kSettle)
        batch_trace_kernel<W, RULE, kSettle><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    else
        batch_trace_kernel<W, RULE, kNoDetector><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    return hipGetLastError();
}

// The onset forms (LIFE_BATCH_OPT_ONSET): the cycle-detecting
// wave_body plus Brent's second phase.  At detection v == T == S_g and the
// universe's rows still hold S_0 (a wave stores once, at the end).  T keeps
// S_g; v reloads S_0; B = S_0 advanced lam generations; then v and B walk
// together until they are equal, after mu = min { m : S_m == S_(m+lam) }
// generations.  Both loops are counted: lam, and g - lam for the walk (S_(g-lam)
// == S_g lies on the cycle, so mu <= g - lam, which is what is recorded should
// the bound ever be reached).  The search sits between the detecting loop and
// the rest loop, where period / found are written anyway, and records nothing
// in a population trace.  Cost: one more state copy, W words.
// (The wave's index in its workgroup is the same in every lane.  Told so, the compiler keeps u, the universe's
// masks and the twenty leaf words expanded from them in scalar registers: the second chain's state takes the
// vector registers that frees.)
__device__ __forceinline__ int64_t wave_of_group() {
    return (int64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

struct BOArgs {
    BWArgs w;
    int64_t *onset;  // -1, or the absolute generation at which the universe entered its cycle
};

template <int W, bool POP, class RP>
__device__ __forceinline__ void onset_body(const BOArgs &o, const int64_t u, const int lane, const RP &rp) {
    const BWArgs &a = o.w;
    const int ny = a.ny;
    const bool active = lane < ny;
    const int up = !active ? lane : lane == 0 ? ny - 1 : lane - 1;
    const int dn = !active ? lane : lane + 1 == ny ? 0 : lane + 1;
    const int addr_up = up << 2, addr_dn = dn << 2;
    const XWrap xw(a.nx, W);
    uint32_t *row = a.cells + ((size_t)u * (size_t)ny + (size_t)lane) * W;

    uint32_t s[2 * W];  // v, and behind it the second chain of the search
    uint32_t *const v = s, *const B = s + W;
    uint32_t T[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        T[j] = v[j] = active ? row[j] : 0u;
        B[j] = 0u;
    }
    int gens = a.gens;
    uint32_t power = 1, lam = 0;
    const uint32_t known = __builtin_amdgcn_readfirstlane((uint32_t)a.period[u]);
    const bool detect = known == 0u;
    if (!detect && !POP) gens = (int)((uint32_t)gens % known);  // found in an earlier call
    WaveTrace tr(POP ? a.trace + (size_t)u * (size_t)a.gens : nullptr, lane);
    auto generation = [&]() {
        wave_generations<W, 1>(v, addr_up, addr_dn, xw, rp);
        if (POP) {
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) c += __popc(v[j]);
            tr.record(c);
        }
    };
    int rest = gens, g = 1;
    if (detect) {
        for (; g <= gens; ++g) {
            generation();
            ++lam;
            uint32_t diff = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) diff |= v[j] ^ T[j];
            if (__builtin_amdgcn_ballot_w64(diff != 0u) == 0ull) break;  // S_g == T: the minimal period is lam
            if (lam == power) {
#pragma unroll
                for (int j = 0; j < W; ++j) T[j] = v[j];
                power <<= 1;
                lam = 0;
            }
        }
        rest = 0;
        if (g <= gens) {
#pragma unroll
            for (int j = 0; j < W; ++j) B[j] = v[j] = active ? row[j] : 0u;  // S_0
            for (uint32_t i = 0; i < lam; ++i) wave_generations<W, 1>(B, addr_up, addr_dn, xw, rp);
            const int bound = g - (int)lam;
            int mu = bound;
            for (int m = 0; m < bound; ++m) {
                uint32_t diff = 0;
#pragma unroll
                for (int j = 0; j < W; ++j) diff |= v[j] ^ B[j];
                if (__builtin_amdgcn_ballot_w64(diff != 0u) == 0ull) {  // S_m == S_(m+lam)
                    mu = m;
                    break;
                }
                wave_generations<W, 2>(s, addr_up, addr_dn, xw, rp);
            }
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = T[j];  // S_g again
            if (lane == 0) {
                a.period[u] = (int64_t)lam;
                a.found[u] = a.gen0 + g;
                o.onset[u] = a.gen0 + mu;
            }
            rest = POP ? gens - g : (int)((uint32_t)(gens - g) % lam);
        }
    }
    for (g = 0; g < rest; ++g) generation();
    if (POP) tr.finish();
    if (!active) return;
#pragma unroll
    for (int j = 0; j < W; ++j) row[j] = v[j];
}

template <int W, int RULE, bool POP>
__global__ __launch_bounds__(64 * kBatchWaves) void batch_onset_kernel(BOArgs o) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + wave_of_group();
    if (u >= o.w.count) return;  // the whole wave
    if (RULE == kSurveyConway)
        onset_body<W, POP>(o, u, lane, ConwayRule{});
    else if (RULE == kSurveyTable)
        onset_body<W, POP>(o, u, lane, TableRule(o.w.rule));
    else
        onset_body<W, POP>(o, u, lane, universe_rule(o.w.rules, u));
}

template <int W, int RULE>
hipError_t launch_onset(const BOArgs &o, unsigned blocks, hipStream_t s) {
    if (o.w.trace)
        batch_onset_kernel<W, RULE, true><<<blocks, 64 * kBatchWaves, 0, s>>>(o);
    else
        batch_onset_kernel<W, RULE, false><<<blocks, 64 * kBatchWaves, 0, s>>>(o);
    return hipGetLastError();
}

// ----------------------------------------------------------------- group tier
// One universe per workgroup: the technique of the small-grid register kernel
// (life_kernels.hip rsmall_kernel without its window) on the batch storage.
// A wave is split into 64 / Wp lane groups (Wp = W rounded up to a power of
// two), each a strip of R consecutive rows, one word column per lane; ns = ny
// / R strips.  Per generation a lane computes the sums of its R rows
// (neighbour words by ds_bpermute inside the group, the x wrap as XWrap),
// publishes those of its first and last row in LDS, one barrier, reads the
// strip above's last and the strip below's first (periodic in y), and applies
// B3/S23 to its rows.  The exchange is double-buffered by the generation's
// parity: a slot is rewritten two generations later, behind the next barrier.
//
// POP, the recording form: after a generation every thread
// counts its R rows and each wave leaves its total in `part`, double-buffered
// by the same parity.  Behind the barrier of the next generation (the one
// after the loop for the last) wave 0 adds the waves' totals up and one lane
// stores the entry: the loop keeps its one barrier.  Totals reach 2048 x 512.
struct BGArgs {
    uint32_t *cells;
    int32_t nx, ny, W, lgWp, gens, ns;
    uint32_t *trace;  // the recording form: a.gens entries per universe, universe-major
};

constexpr int kBatchGroupWaves = kBatchGroupThreads / 64;

template <int R, bool POP>
__device__ __forceinline__ void group_body(const BGArgs &a) {
    __shared__ uint32_t xch[2][4][kBatchGroupThreads];  // [parity][top s0/s1, bottom s0/s1][thread]
    __shared__ uint32_t part[POP ? 2 : 1][POP ? kBatchGroupWaves : 1];  // [parity][wave]: live cells of a generation
    const int t = (int)threadIdx.x;
    const int Wp = 1 << a.lgWp, W = a.W;
    const int j = t & (Wp - 1);  // word column
    const int st = t >> a.lgWp;  // strip
    const bool active = st < a.ns && j < W;
    const int base = (t & 63) & ~(Wp - 1);  // first lane of this lane group
    const int jl = j == 0 ? W - 1 : j - 1, jr = j + 1 >= W ? 0 : j + 1;
    const int addr_l = (base + jl) << 2, addr_r = (base + jr) << 2;
    const XWrap xw(a.nx, W);
    const bool last = j == W - 1;
    const uint32_t keep = last ? xw.keep : 0xFFFFFFFFu;
    const uint32_t lsh = j == 0 ? xw.lsh : 0u;
    const int sa = st == 0 ? a.ns - 1 : st - 1, sb = st + 1 >= a.ns ? 0 : st + 1;
    const int ta = ((sa << a.lgWp) + j) & (kBatchGroupThreads - 1), tb = ((sb << a.lgWp) + j) & (kBatchGroupThreads - 1);
    uint32_t *uni = a.cells + (size_t)blockIdx.x * (size_t)W * (size_t)a.ny;
    const int y0 = st * R;

    uint32_t v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = active ? uni[(size_t)(y0 + r) * W + j] : 0u;
    auto hsum = [&](uint32_t c, uint32_t &s0, uint32_t &s1) {
        const uint32_t l = bperm(addr_l, c) << lsh;
        const uint32_t rw = bperm(addr_r, c);
        c = b3<kKeepMux>(c, keep, rw << xw.qs);  // the last word gets cell 0 at bit q
        BitEnc::fa(__builtin_amdgcn_alignbit(c, l, 31), c, __builtin_amdgcn_alignbit(rw, c, 1), s0, s1);
    };
    // wave 0 behind a barrier: entry g of the trace from the waves' totals in part[g & 1]
    uint32_t *const entries = POP ? a.trace + (size_t)blockIdx.x * (size_t)a.gens : nullptr;
    const int waves = (int)(blockDim.x >> 6);
    auto publish = [&](int g) {
        if (t >= 64) return;
        const uint32_t sum = row_totals(t < waves ? part[g & 1][t & (kBatchGroupWaves - 1)] : 0u);
        if (t == kBatchGroupWaves - 1) entries[g] = sum;
    };
    for (int g = 0; g < a.gens; ++g) {
        const int par = g & 1;
        uint32_t h0[R], h1[R];
        hsum(v[0], h0[0], h1[0]);
        if (R > 1) hsum(v[R - 1], h0[R - 1], h1[R - 1]);
        xch[par][0][t] = h0[0];
        xch[par][1][t] = h1[0];
        xch[par][2][t] = h0[R - 1];
        xch[par][3][t] = h1[R - 1];
        __syncthreads();
        if (POP && g > 0) publish(g - 1);
        const uint32_t a0 = xch[par][2][ta], a1 = xch[par][3][ta];
        const uint32_t d0 = xch[par][0][tb], d1 = xch[par][1][tb];
#pragma unroll
        for (int r = 1; r < R - 1; ++r) hsum(v[r], h0[r], h1[r]);
#pragma unroll
        for (int r = 1; r < R - 1; ++r)
            v[r] = BitEnc::rule1(h0[r - 1], h1[r - 1], h0[r], h1[r], h0[r + 1], h1[r + 1], v[r]) & keep;
        if (R == 1) {
            v[0] = BitEnc::rule1(a0, a1, h0[0], h1[0], d0, d1, v[0]) & keep;
        } else {
            v[0] = BitEnc::rule1(a0, a1, h0[0], h1[0], h0[1], h1[1], v[0]) & keep;
            v[R - 1] = BitEnc::rule1(h0[R - 2], h1[R - 2], h0[R - 1], h1[R - 1], d0, d1, v[R - 1]) & keep;
        }
        if (POP) {
            uint32_t c = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) c += __popc(v[r]);
            c = wave_total(active ? c : 0u);  // (a thread without a strip computes on what it reads, and is never stored)
            if ((t & 63) == 0) part[par][t >> 6] = c;
        }
    }
    if (POP) {
        __syncthreads();
        publish(a.gens - 1);
    }
    if (!active) return;
#pragma unroll
    for (int r = 0; r < R; ++r) uni[(size_t)(y0 + r) * W + j] = v[r];
}

template <int R>
__global__ __launch_bounds__(kBatchGroupThreads) void batch_group_kernel(BGArgs a) {
    group_body<R, false>(a);
}

// (a name of its own: the instances above are counted by theirs)
template <int R>
__global__ __launch_bounds__(kBatchGroupThreads) void batch_trace_group_kernel(BGArgs a) {
    group_body<R, true>(a);
}

// ------------------------------------------------------------- data movement
// (the definitions of life_io.hip's fill and census, per universe)
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t cell_mix(uint64_t v) {
    v *= 0x9E3779B97F4A7C15ull;
    return v ^ (v >> 29);
}

// cells of word j of an nx-wide row
__device__ __forceinline__ int row_cells(int64_t nx, int64_t j) { return nx - 32 * j < 32 ? (int)(nx - 32 * j) : 32; }

// One thread per word, grid-stride: word i = (universe, row, word column).
struct WordAt {
    int64_t u, y, j;
    __device__ __forceinline__ WordAt(int64_t i, int64_t W, int64_t ny) : u(i / (W * ny)), y(i / W % ny), j(i % W) {}
};

__global__ void batch_import_kernel(const uint8_t *dense, uint32_t *cells, int64_t words, int64_t nx, int64_t ny,
                                    int64_t W) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
        const WordAt at(i, W, ny);
        const uint8_t *src = dense + ((size_t)at.u * (size_t)ny + (size_t)at.y) * (size_t)nx + 32 * at.j;
        const int n = row_cells(nx, at.j);
        uint32_t x = 0;
        for (int k = 0; k < n; ++k) x |= (uint32_t)(src[k] != 0) << k;
        cells[i] = x;
    }
}

__global__ void batch_export_kernel(const uint32_t *cells, uint8_t *dense, int64_t words, int64_t nx, int64_t ny,
                                    int64_t W) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
        const WordAt at(i, W, ny);
        uint8_t *dst = dense + ((size_t)at.u * (size_t)ny + (size_t)at.y) * (size_t)nx + 32 * at.j;
        const int n = row_cells(nx, at.j);
        const uint32_t x = cells[i];
        for (int k = 0; k < n; ++k) dst[k] = (uint8_t)((x >> k) & 1u);
    }
}

__global__ void batch_fill_kernel(uint32_t *cells, int64_t words, int64_t nx, int64_t ny, int64_t W, uint64_t seed,
                                  uint32_t thr) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
        const WordAt at(i, W, ny);
        const uint64_t key = splitmix64(seed + (uint64_t)at.u);
        const uint64_t base = (uint64_t)(at.y * nx + 32 * at.j);
        const int n = row_cells(nx, at.j);
        uint32_t x = 0;
        for (int k = 0; k < n; ++k) x |= (uint32_t)((uint32_t)(splitmix64(key ^ (base + (uint64_t)k)) >> 32) < thr) << k;
        cells[i] = x;
    }
}

// One wave per universe: its lanes walk the universe's words.
__global__ __launch_bounds__(64 * kBatchWaves) void batch_census_kernel(const uint32_t *cells, unsigned long long *live,
                                                                        unsigned long long *sum, int64_t count,
                                                                        int64_t nx, int64_t ny, int64_t W) {
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + (int64_t)(threadIdx.x >> 6);
    if (u >= count) return;
    const uint32_t *uni = cells + (size_t)u * (size_t)(W * ny);
    const int64_t q = nx - 32 * (W - 1);
    unsigned long long c = 0, x = 0;
    for (int64_t i = threadIdx.x & 63u; i < W * ny; i += 64) {
        const int64_t y = i / W, j = i % W;
        uint32_t bits = uni[i];
        if (j == W - 1 && q < 32) bits &= (1u << q) - 1u;  // (zero already: no writer leaves padding bits)
        c += __popc(bits);
        const uint64_t base = (uint64_t)(y * nx + 32 * j) + 1u;
        while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1u;
            x += cell_mix(base + (uint64_t)b);
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        c += __shfl_xor(c, s);
        x += __shfl_xor(x, s);
    }
    if ((threadIdx.x & 63u) == 0) {
        live[u] = c;
        sum[u] = x;
    }
}

// ---------------------------------------------------- Generations (wave tier)
// DESIGN.md 5.13.  A cell state s in [0, C): the alive plane A (s == 1) is the
// batch storage, d = s - 1 of a dying cell (else 0) is held in P more bit
// planes of the same word layout, plane p of universe u `plane` words after
// plane p - 1.  Only A is summed: the funnel shifts and the four ds_bpermute
// per word are wave_body's, and so is the rule -- n = TableRule(sums, A) is the
// Life-like successor of a cell that is dead or alive.  Per word then, with
// `dying` the OR of the d planes:
//   A'  = n & ~dying                      (a dying cell is not reborn)
//   d'  = dying ? (d == C - 2 ? 0 : d + 1) : (A & ~n & (C > 2)) ? 1 : 0
// C - 2 and C > 2 are wave-uniform words expanded before the generation loop
// beside the rule's leaves, so a C = 2 universe of a mixed batch never starts
// to decay, and one kernel serves a uniform rule (from the launch arguments)
// and a rule per universe (from the table).  Lanes at and beyond ny and the
// padding bits hold zeros in every plane: A is zero there, so nothing starts.
constexpr uint32_t kGenStart = (0xF0 & ~0xCC & 0xAA) & 0xFF;      // a & ~b & c: alive, not surviving, the rule decays
constexpr uint32_t kGenAndNot = (0xF0 & ~(0xCC | 0xAA)) & 0xFF;   // a & ~(b | c)
constexpr uint32_t kGenOrXor = (0xF0 | (0xCC ^ 0xAA)) & 0xFF;     // a | (b ^ c)
constexpr uint32_t kGenOrAnd = ((0xF0 | 0xCC) & 0xAA) & 0xFF;     // (a | b) & c
constexpr uint32_t kGenXorAnd = ((0xF0 ^ 0xCC) & 0xAA) & 0xFF;    // (a ^ b) & c
constexpr uint32_t kGenAndNotOr = ((0xF0 & ~0xCC) | 0xAA) & 0xFF; // (a & ~b) | c
constexpr uint32_t kGenOr3 = (0xF0 | 0xCC | 0xAA) & 0xFF;
constexpr uint32_t kGenAnd3 = (0xF0 & 0xCC & 0xAA) & 0xFF;

struct BNArgs {
    uint32_t *cells, *decay;
    int64_t plane;  // words between two decay planes
    int64_t *settled;
    int64_t count, gen0;
    int32_t nx, ny, gens;
    uint32_t birth, survive;  // the uniform rule, as a table entry (rules null)
    const uint2 *rules;       // (birth | states << 16, survive) of universe u
    int64_t *period, *found;
};

// One generation of K Generations states side by side, as wave_generations:
// chain c in x[c N, c N + N), N = W (1 + P), its alive words first and plane p
// of d at W (1 + p).  `decays` and L: "the universe decays at all" and bit p of
// C - 2, each spread over a word.
template <int W, int P, int K>
__device__ __forceinline__ void gen_generations(uint32_t *x, const int addr_up, const int addr_dn, const XWrap &xw,
                                                const TableRule &rp, const uint32_t decays, const uint32_t (&L)[P]) {
    constexpr int N = W * (1 + P);
    uint32_t s0[K * W], s1[K * W];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const uint32_t *v = x + c * N;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t l = j == 0 ? v[W - 1] << xw.lsh : v[j - 1];
            const uint32_t r = j == W - 1 ? v[0] : v[j + 1];
            uint32_t m = v[j];
            if (j == W - 1) m = b3<kKeepMux>(m, xw.keep, v[0] << xw.qs);
            BitEnc::fa(__builtin_amdgcn_alignbit(m, l, 31), m, __builtin_amdgcn_alignbit(r, m, 1), s0[c * W + j],
                       s1[c * W + j]);
        }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            uint32_t *v = x + c * N;
            const int i = c * W + j;
            const uint32_t a0 = bperm(addr_up, s0[i]), a1 = bperm(addr_up, s1[i]);
            const uint32_t d0 = bperm(addr_dn, s0[i]), d1 = bperm(addr_dn, s1[i]);
            const uint32_t alive = v[j];
            const uint32_t n = rp(a0, a1, s0[i], s1[i], d0, d1, alive);
            uint32_t *d = &v[W + j];  // plane p at d[W p]
            const uint32_t start = b3<kGenStart>(alive, n, decays);
            if (P == 1) {  // d is 0 or 1 = C - 2: a dying cell dies, 2 v_bitop3
                v[j] = b3<kGenAndNot>(n, d[0], d[0]);
                d[0] = start;
            } else if (P == 2) {  // 6 and a v_xor
                v[j] = b3<kGenAndNot>(n, d[0], d[W]);
                const uint32_t more = b3<kGenOrXor>(d[0] ^ L[0], d[W], L[1]);     // d != C - 2
                const uint32_t go = b3<kGenOrAnd>(d[0], d[W], more);              // dying, and not for the last time
                const uint32_t t1 = b3<kGenXorAnd>(d[W], d[0], go);
                d[0] = b3<kGenAndNotOr>(go, d[0], start);
                d[W] = t1;
            } else {  // 12, a v_xor and a v_and
                const uint32_t low = b3<kGenOr3>(d[0], d[W], d[2 * W]);
                v[j] = b3<kGenAndNot>(n, low, d[3 * W]);
                uint32_t more = b3<kGenOrXor>(d[0] ^ L[0], d[W], L[1]);
                more = b3<kGenOrXor>(more, d[2 * W], L[2]);
                more = b3<kGenOrXor>(more, d[3 * W], L[3]);
                const uint32_t go = b3<kGenOrAnd>(low, d[3 * W], more);
                const uint32_t c2 = d[0] & d[W], c3 = b3<kGenAnd3>(d[0], d[W], d[2 * W]);  // the ripple of d + 1
                const uint32_t t1 = b3<kGenXorAnd>(d[W], d[0], go);
                d[0] = b3<kGenAndNotOr>(go, d[0], start);
                d[W] = t1;
                d[2 * W] = b3<kGenXorAnd>(d[2 * W], c2, go);
                d[3 * W] = b3<kGenXorAnd>(d[3 * W], c3, go);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) x[c * N + W - 1] &= xw.keep;  // (the d planes need none: nothing starts where A is zero)
}

template <int W, int P, int DET>
__global__ __launch_bounds__(64 * kBatchWaves) void batch_gen_kernel(BNArgs a) {
    constexpr bool SETTLE = DET == kSettle, CYCLE = DET == kCycle;
    constexpr int N = W * (1 + P);  // state words of a lane: v[j] alive, v[W (1 + p) + j] plane p of d
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + (int64_t)(threadIdx.x >> 6);
    if (u >= a.count) return;  // the whole wave
    uint2 m = make_uint2(a.birth, a.survive);
    if (a.rules) m = a.rules[u];
    const TableRule rp = universe_rule(&m, 0);  // (the leaves read bits 0 .. 8 of a mask: the state count rides above)
    // d of the last dying state, bit p spread over a word, and "this universe decays at all"
    const uint32_t states = m.x >> 16;
    const uint32_t top = states > 2u ? states - 2u : 0u;
    const uint32_t decays = states > 2u ? 0xFFFFFFFFu : 0u;
    uint32_t L[P];
#pragma unroll
    for (int p = 0; p < P; ++p) L[p] = (top >> p) & 1u ? 0xFFFFFFFFu : 0u;

    const int ny = a.ny;
    const bool active = lane < ny;
    const int up = !active ? lane : lane == 0 ? ny - 1 : lane - 1;
    const int dn = !active ? lane : lane + 1 == ny ? 0 : lane + 1;
    const int addr_up = up << 2, addr_dn = dn << 2;
    const XWrap xw(a.nx, W);
    const size_t at = ((size_t)u * (size_t)ny + (size_t)lane) * W;

    uint32_t v[N];
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = active ? a.cells[at + j] : 0u;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < W; ++j) v[W * (1 + p) + j] = active ? a.decay[(size_t)p * (size_t)a.plane + at + j] : 0u;

    int gens = a.gens;
    bool detect = false;
    if (SETTLE) {
        detect = a.settled[u] < 0;
        if (!detect) gens &= 1;  // settled in an earlier call: the state has period 1 or 2
    }
    uint32_t p1[SETTLE ? N : 1], p2[SETTLE ? N : 1];  // S_(g-1), S_(g-2), every plane
    if (SETTLE) {
#pragma unroll
        for (int i = 0; i < N; ++i) p1[i] = p2[i] = v[i];
    }
    uint32_t T[CYCLE ? N : 1];  // Brent's checkpoint, every plane (wave_body)
    uint32_t power = 1, lam = 0;
    if (CYCLE) {
        const uint32_t known = __builtin_amdgcn_readfirstlane((uint32_t)a.period[u]);
        detect = known == 0u;
        if (!detect) gens = (int)((uint32_t)gens % known);  // found in an earlier call
#pragma unroll
        for (int i = 0; i < N; ++i) T[i] = v[i];
    }
    // (gen_generations<W, P, 1> spelled out: the instances of this kernel keep the code they were measured with)
    auto generation = [&]() {
        uint32_t s0[W], s1[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t l = j == 0 ? v[W - 1] << xw.lsh : v[j - 1];
            const uint32_t r = j == W - 1 ? v[0] : v[j + 1];
            uint32_t c = v[j];
            if (j == W - 1) c = b3<kKeepMux>(c, xw.keep, v[0] << xw.qs);
            BitEnc::fa(__builtin_amdgcn_alignbit(c, l, 31), c, __builtin_amdgcn_alignbit(r, c, 1), s0[j], s1[j]);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t a0 = bperm(addr_up, s0[j]), a1 = bperm(addr_up, s1[j]);
            const uint32_t d0 = bperm(addr_dn, s0[j]), d1 = bperm(addr_dn, s1[j]);
            const uint32_t alive = v[j];
            const uint32_t n = rp(a0, a1, s0[j], s1[j], d0, d1, alive);
            uint32_t *d = &v[W + j];  // plane p at d[W p]
            const uint32_t start = b3<kGenStart>(alive, n, decays);
            if (P == 1) {  // d is 0 or 1 = C - 2: a dying cell dies, 2 v_bitop3
                v[j] = b3<kGenAndNot>(n, d[0], d[0]);
                d[0] = start;
            } else if (P == 2) {  // 6 and a v_xor
                v[j] = b3<kGenAndNot>(n, d[0], d[W]);
                const uint32_t more = b3<kGenOrXor>(d[0] ^ L[0], d[W], L[1]);     // d != C - 2
                const uint32_t go = b3<kGenOrAnd>(d[0], d[W], more);              // dying, and not for the last time
                const uint32_t t1 = b3<kGenXorAnd>(d[W], d[0], go);
                d[0] = b3<kGenAndNotOr>(go, d[0], start);
                d[W] = t1;
            } else {  // 12, a v_xor and a v_and
                const uint32_t low = b3<kGenOr3>(d[0], d[W], d[2 * W]);
                v[j] = b3<kGenAndNot>(n, low, d[3 * W]);
                uint32_t more = b3<kGenOrXor>(d[0] ^ L[0], d[W], L[1]);
                more = b3<kGenOrXor>(more, d[2 * W], L[2]);
                more = b3<kGenOrXor>(more, d[3 * W], L[3]);
                const uint32_t go = b3<kGenOrAnd>(low, d[3 * W], more);
                const uint32_t c2 = d[0] & d[W], c3 = b3<kGenAnd3>(d[0], d[W], d[2 * W]);  // the ripple of d + 1
                const uint32_t t1 = b3<kGenXorAnd>(d[W], d[0], go);
                d[0] = b3<kGenAndNotOr>(go, d[0], start);
                d[W] = t1;
                d[2 * W] = b3<kGenXorAnd>(d[2 * W], c2, go);
                d[3 * W] = b3<kGenXorAnd>(d[3 * W], c3, go);
            }
        }
        v[W - 1] &= xw.keep;  // (the d planes need none: nothing starts where A is zero)
    };
    auto differs = [&](const uint32_t *than) {
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) diff |= v[i] ^ than[i];
        return __builtin_amdgcn_ballot_w64(diff != 0u) != 0ull;
    };
    if (CYCLE) {
        // as wave_body: the detecting generations, then the rest; what is recorded is written between the loops
        int rest = gens, g = 1;
        if (detect) {
            for (; g <= gens; ++g) {
                generation();
                ++lam;
                if (!differs(T)) break;  // S_g == T in every plane: the minimal period is lam
                if (lam == power) {
#pragma unroll
                    for (int i = 0; i < N; ++i) T[i] = v[i];
                    power <<= 1;
                    lam = 0;
                }
            }
            rest = 0;
            if (g <= gens) {
                if (lane == 0) {
                    a.period[u] = (int64_t)lam;
                    a.found[u] = a.gen0 + g;
                }
                rest = (int)((uint32_t)(gens - g) % lam);
            }
        }
        for (g = 0; g < rest; ++g) generation();
    }
    for (int g = 1; !CYCLE && g <= gens; ++g) {
        generation();
        if (SETTLE && detect) {
            if (g >= 2 && !differs(p2)) {  // S_g == S_(g-2), the whole wave agrees
                if (lane == 0) a.settled[u] = a.gen0 + g;
                detect = false;
                gens = g + ((gens - g) & 1);
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
                p2[i] = p1[i];
                p1[i] = v[i];
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < W; ++j) a.cells[at + j] = v[j];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < W; ++j) a.decay[(size_t)p * (size_t)a.plane + at + j] = v[W * (1 + p) + j];
}

template <int W, int P>
hipError_t launch_gen(const BNArgs &a, int det, unsigned blocks, hipStream_t s) {
    if (det == kCycle)
        batch_gen_kernel<W, P, kCycle><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    else if (det == kSettle)
        batch_gen_kernel<W, P, kSettle><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    else
        batch_gen_kernel<W, P, kNoDetector><<<blocks, 64 * kBatchWaves, 0, s>>>(a);
    return hipGetLastError();
}

// The onset form of Generations: batch_gen_kernel's cycle
// detection plus the second phase of onset_body, every plane loaded, stepped
// and compared.  One more state copy: W (1 + P) words.
struct BMArgs {
    BNArgs n;
    int64_t *onset;
};

template <int W, int P>
__global__ __launch_bounds__(64 * kBatchWaves) void batch_onset_gen_kernel(BMArgs o) {
    constexpr int N = W * (1 + P);
    const BNArgs &a = o.n;
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + wave_of_group();
    if (u >= a.count) return;  // the whole wave
    uint2 m = make_uint2(a.birth, a.survive);
    if (a.rules) m = a.rules[u];
    const TableRule rp = universe_rule(&m, 0);
    const uint32_t states = m.x >> 16;
    const uint32_t top = states > 2u ? states - 2u : 0u;
    const uint32_t decays = states > 2u ? 0xFFFFFFFFu : 0u;
    uint32_t L[P];
#pragma unroll
    for (int p = 0; p < P; ++p) L[p] = (top >> p) & 1u ? 0xFFFFFFFFu : 0u;

    const int ny = a.ny;
    const bool active = lane < ny;
    const int up = !active ? lane : lane == 0 ? ny - 1 : lane - 1;
    const int dn = !active ? lane : lane + 1 == ny ? 0 : lane + 1;
    const int addr_up = up << 2, addr_dn = dn << 2;
    const XWrap xw(a.nx, W);
    const size_t at = ((size_t)u * (size_t)ny + (size_t)lane) * W;

    uint32_t s[2 * N];  // v, and behind it the second chain of the search
    uint32_t *const v = s, *const B = s + N;
    auto load = [&]() {  // the universe's stored state, S_0 until the wave's one store
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = active ? a.cells[at + j] : 0u;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int j = 0; j < W; ++j)
                v[W * (1 + p) + j] = active ? a.decay[(size_t)p * (size_t)a.plane + at + j] : 0u;
    };
    load();
    uint32_t T[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T[i] = v[i];
        B[i] = 0u;
    }
    int gens = a.gens;
    uint32_t power = 1, lam = 0;
    const uint32_t known = __builtin_amdgcn_readfirstlane((uint32_t)a.period[u]);
    const bool detect = known == 0u;
    if (!detect) gens = (int)((uint32_t)gens % known);  // found in an earlier call
    auto generation = [&]() { gen_generations<W, P, 1>(v, addr_up, addr_dn, xw, rp, decays, L); };
    auto differs = [&](const uint32_t *than) {
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) diff |= v[i] ^ than[i];
        return __builtin_amdgcn_ballot_w64(diff != 0u) != 0ull;
    };
    int rest = gens, g = 1;
    if (detect) {
        for (; g <= gens; ++g) {
            generation();
            ++lam;
            if (!differs(T)) break;  // S_g == T in every plane: the minimal period is lam
            if (lam == power) {
#pragma unroll
                for (int i = 0; i < N; ++i) T[i] = v[i];
                power <<= 1;
                lam = 0;
            }
        }
        rest = 0;
        if (g <= gens) {
            load();
#pragma unroll
            for (int i = 0; i < N; ++i) B[i] = v[i];
            for (uint32_t i = 0; i < lam; ++i) gen_generations<W, P, 1>(B, addr_up, addr_dn, xw, rp, decays, L);
            const int bound = g - (int)lam;
            int mu = bound;
            for (int k = 0; k < bound; ++k) {
                if (!differs(B)) {  // S_k == S_(k+lam)
                    mu = k;
                    break;
                }
                gen_generations<W, P, 2>(s, addr_up, addr_dn, xw, rp, decays, L);
            }
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = T[i];  // S_g again
            if (lane == 0) {
                a.period[u] = (int64_t)lam;
                a.found[u] = a.gen0 + g;
                o.onset[u] = a.gen0 + mu;
            }
            rest = (int)((uint32_t)(gens - g) % lam);
        }
    }
    for (g = 0; g < rest; ++g) generation();
    if (!active) return;
#pragma unroll
    for (int j = 0; j < W; ++j) a.cells[at + j] = v[j];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < W; ++j) a.decay[(size_t)p * (size_t)a.plane + at + j] = v[W * (1 + p) + j];
}

// The data movement of the states: one thread per word position of the alive
// plane, which walks the `planes` decay planes at the same offset.
// d of the cell at bit k of four plane words
__device__ __forceinline__ uint32_t plane_bits(const uint32_t (&d)[4], int k) {
    return ((d[0] >> k) & 1u) | ((d[1] >> k) & 1u) << 1 | ((d[2] >> k) & 1u) << 2 | ((d[3] >> k) & 1u) << 3;
}

__global__ void batch_import_states_kernel(const uint8_t *dense, uint32_t *cells, uint32_t *decay, int64_t plane,
                                           int planes, int64_t words, int64_t nx, int64_t ny, int64_t W) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
        const WordAt at(i, W, ny);
        const uint8_t *src = dense + ((size_t)at.u * (size_t)ny + (size_t)at.y) * (size_t)nx + 32 * at.j;
        const int n = row_cells(nx, at.j);
        uint32_t x = 0, d[4] = {0, 0, 0, 0};
        for (int k = 0; k < n; ++k) {
            const uint32_t s = src[k];
            x |= (uint32_t)(s == 1u) << k;
            const uint32_t e = s > 1u ? s - 1u : 0u;
#pragma unroll
            for (int p = 0; p < 4; ++p) d[p] |= ((e >> p) & 1u) << k;
        }
        cells[i] = x;
        for (int p = 0; p < planes; ++p) decay[(size_t)p * (size_t)plane + i] = d[p];
    }
}

__global__ void batch_export_states_kernel(const uint32_t *cells, const uint32_t *decay, int64_t plane, int planes,
                                           uint8_t *dense, int64_t words, int64_t nx, int64_t ny, int64_t W) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
        const WordAt at(i, W, ny);
        uint8_t *dst = dense + ((size_t)at.u * (size_t)ny + (size_t)at.y) * (size_t)nx + 32 * at.j;
        const int n = row_cells(nx, at.j);
        const uint32_t x = cells[i];
        uint32_t d[4] = {0, 0, 0, 0};
        for (int p = 0; p < planes; ++p) d[p] = decay[(size_t)p * (size_t)plane + i];
        for (int k = 0; k < n; ++k) {
            const uint32_t e = plane_bits(d, k);
            dst[k] = (uint8_t)(e ? e + 1u : (x >> k) & 1u);
        }
    }
}

// One wave per universe, as batch_census_kernel: s = 1 counted in live, s >= 2 in dying, s * cell_mix in sum.
__global__ __launch_bounds__(64 * kBatchWaves) void batch_census_states_kernel(
    const uint32_t *cells, const uint32_t *decay, int64_t plane, int planes, unsigned long long *live,
    unsigned long long *dying, unsigned long long *sum, int64_t count, int64_t nx, int64_t ny, int64_t W) {
    const int64_t u = (int64_t)blockIdx.x * kBatchWaves + (int64_t)(threadIdx.x >> 6);
    if (u >= count) return;
    const size_t uni = (size_t)u * (size_t)(W * ny);
    const int64_t q = nx - 32 * (W - 1);
    unsigned long long c = 0, dy = 0, x = 0;
    for (int64_t i = threadIdx.x & 63u; i < W * ny; i += 64) {
        const int64_t y = i / W, j = i % W;
        const uint32_t keep = j == W - 1 && q < 32 ? (1u << q) - 1u : 0xFFFFFFFFu;  // (zero already beyond it)
        const uint32_t alive = cells[uni + i] & keep;
        uint32_t d[4] = {0, 0, 0, 0};
        for (int p = 0; p < planes; ++p) d[p] = decay[(size_t)p * (size_t)plane + uni + i] & keep;
        uint32_t bits = alive | d[0] | d[1] | d[2] | d[3];
        c += __popc(alive);
        dy += __popc(bits & ~alive);
        const uint64_t base = (uint64_t)(y * nx + 32 * j) + 1u;
        while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1u;
            const uint32_t e = plane_bits(d, b);
            x += (uint64_t)(e ? e + 1u : 1u) * cell_mix(base + (uint64_t)b);
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        c += __shfl_xor(c, s);
        dy += __shfl_xor(dy, s);
        x += __shfl_xor(x, s);
    }
    if ((threadIdx.x & 63u) == 0) {
        live[u] = c;
        dying[u] = dy;
        sum[u] = x;
    }
}

unsigned word_blocks(int64_t words) { return (unsigned)std::min<int64_t>((words + 255) / 256, 1 << 20); }
unsigned wave_blocks(int64_t count) { return (unsigned)((count + kBatchWaves - 1) / kBatchWaves); }
// one workgroup per universe, or per kBatchWaves universes: the grid's x must hold them
bool grid_ok(int64_t blocks) { return blocks >= 1 && blocks <= INT_MAX; }

}  // namespace

hipError_t launch_batch_wave(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                             const RuleWords *rule, bool settle, int64_t *settled, int64_t gen0, hipStream_t s) {
    if (p.tier != LIFE_BATCH_TIER_WAVE || gens < 1 || gens > INT32_MAX || (settle && !settled) ||
        !grid_ok((count + kBatchWaves - 1) / kBatchWaves))
        return hipErrorInvalidValue;
    BWArgs a{};
    a.cells = cells;
    a.settled = settled;
    a.count = count;
    a.gen0 = gen0;
    a.nx = (int32_t)nx;
    a.ny = (int32_t)ny;
    a.gens = (int32_t)gens;
    if (rule) a.rule = *rule;
    const unsigned blocks = wave_blocks(count);
    switch (p.words) {
#define LIFE_BW(N) \
    case N: return rule ? launch_wave<N, TableRule>(a, settle, blocks, s) : launch_wave<N, ConwayRule>(a, settle, blocks, s);
        LIFE_BW(1) LIFE_BW(2) LIFE_BW(3) LIFE_BW(4)
#undef LIFE_BW
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_batch_survey(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                               const RuleWords *rule, const uint32_t *rules, bool settle, int64_t *settled, bool cycle,
                               int64_t *period, int64_t *found, int64_t gen0, hipStream_t s) {
    if (p.tier != LIFE_BATCH_TIER_WAVE || gens < 1 || gens > INT32_MAX || (settle && !settled) || (settle && cycle) ||
        (cycle && (!period || !found)) || (!rules && !cycle) || !grid_ok((count + kBatchWaves - 1) / kBatchWaves))
        return hipErrorInvalidValue;
    BWArgs a{};
    a.cells = cells;
    a.settled = settled;
    a.count = count;
    a.gen0 = gen0;
    a.nx = (int32_t)nx;
    a.ny = (int32_t)ny;
    a.gens = (int32_t)gens;
    if (rule) a.rule = *rule;
    a.rules = reinterpret_cast<const uint2 *>(rules);
    a.period = period;
    a.found = found;
    const int r = rules ? kSurveyPerUniverse : rule ? kSurveyTable : kSurveyConway;
    const int det = cycle ? kCycle : settle ? kSettle : kNoDetector;
    const unsigned blocks = wave_blocks(count);
    switch (p.words) {
    case 1: return launch_survey<1>(a, r, det, blocks, s);
    case 2: return launch_survey<2>(a, r, det, blocks, s);
    case 3: return launch_survey<3>(a, r, det, blocks, s);
    case 4: return launch_survey<4>(a, r, det, blocks, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_batch_trace(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                              const RuleWords *rule, const uint32_t *rules, bool settle, int64_t *settled, bool cycle,
                              int64_t *period, int64_t *found, int64_t gen0, uint32_t *trace, hipStream_t s) {
    if (p.tier != LIFE_BATCH_TIER_WAVE || gens < 1 || gens > INT32_MAX || (settle && !settled) || (settle && cycle) ||
        (cycle && (!period || !found)) || !trace || count * gens > kBatchTraceEntries ||
        !grid_ok((count + kBatchWaves - 1) / kBatchWaves))
        return hipErrorInvalidValue;
    BWArgs a{};
    a.cells = cells;
    a.settled = settled;
    a.count = count;
    a.gen0 = gen0;
    a.nx = (int32_t)nx;
    a.ny = (int32_t)ny;
    a.gens = (int32_t)gens;
    if (rule) a.rule = *rule;
    a.rules = reinterpret_cast<const uint2 *>(rules);
    a.period = period;
    a.found = found;
    a.trace = trace;
    const int r = rules ? kSurveyPerUniverse : rule ? kSurveyTable : kSurveyConway;
    const int det = cycle ? kCycle : settle ? kSettle : kNoDetector;
    const unsigned blocks = wave_blocks(count);
    switch (p.words * 4 + r) {
#define LIFE_BT(N) \
    case N * 4 + kSurveyConway: return launch_trace<N, kSurveyConway>(a, det, blocks, s); \
    case N * 4 + kSurveyTable: return launch_trace<N, kSurveyTable>(a, det, blocks, s); \
    case N * 4 + kSurveyPerUniverse: return launch_trace<N, kSurveyPerUniverse>(a, det, blocks, s);
        LIFE_BT(1) LIFE_BT(2) LIFE_BT(3) LIFE_BT(4)
#undef LIFE_BT
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_batch_onset(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                              const RuleWords *rule, const uint32_t *rules, int64_t *period, int64_t *found,
                              int64_t *onset, int64_t gen0, uint32_t *trace, hipStream_t s) {
    if (p.tier != LIFE_BATCH_TIER_WAVE || gens < 1 || gens > INT32_MAX || !period || !found || !onset ||
        (trace && count * gens > kBatchTraceEntries) || !grid_ok((count + kBatchWaves - 1) / kBatchWaves))
        return hipErrorInvalidValue;
    BOArgs o{};
    BWArgs &a = o.w;
    a.cells = cells;
    a.count = count;
    a.gen0 = gen0;
    a.nx = (int32_t)nx;
    a.ny = (int32_t)ny;
    a.gens = (int32_t)gens;
    if (rule) a.rule = *rule;
    a.rules = reinterpret_cast<const uint2 *>(rules);
    a.period = period;
    a.found = found;
    a.trace = trace;
    o.onset = onset;
    const int r = rules ? kSurveyPerUniverse : rule ? kSurveyTable : kSurveyConway;
    const unsigned blocks = wave_blocks(count);
    switch (p.words * 4 + r) {
#define LIFE_BO(N) \
    case N * 4 + kSurveyConway: return launch_onset<N, kSurveyConway>(o, blocks, s); \
    case N * 4 + kSurveyTable: return launch_onset<N, kSurveyTable>(o, blocks, s); \
    case N * 4 + kSurveyPerUniverse: return launch_onset<N, kSurveyPerUniverse>(o, blocks, s);
        LIFE_BO(1) LIFE_BO(2) LIFE_BO(3) LIFE_BO(4)
#undef LIFE_BO
    default: return hipErrorInvalidValue;
    }
}

namespace {

hipError_t launch_group(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, int64_t gens,
                        uint32_t *trace, hipStream_t s) {
    if (p.tier != LIFE_BATCH_TIER_GROUP || gens < 1 || gens > INT32_MAX || !grid_ok(count)) return hipErrorInvalidValue;
    BGArgs a{};
    a.cells = cells;
    a.nx = (int32_t)nx;
    a.ny = (int32_t)ny;
    a.W = p.words;
    a.lgWp = p.lg_wp;
    a.gens = (int32_t)gens;
    a.ns = p.strips;
    a.trace = trace;
    // only the waves that own strips (the barrier counts the launched waves)
    const unsigned threads = 64u * (unsigned)p.waves_per_group;
    if (threads > (unsigned)kBatchGroupThreads) return hipErrorInvalidValue;
    switch (p.rows) {
#define LIFE_BG(N) \
    case N: \
        if (trace) \
            batch_trace_group_kernel<N><<<(unsigned)count, threads, 0, s>>>(a); \
        else \
            batch_group_kernel<N><<<(unsigned)count, threads, 0, s>>>(a); \
        break;
        LIFE_BG(1) LIFE_BG(2) LIFE_BG(3) LIFE_BG(4) LIFE_BG(5) LIFE_BG(6) LIFE_BG(8) LIFE_BG(10) LIFE_BG(12)
        LIFE_BG(16) LIFE_BG(20) LIFE_BG(25) LIFE_BG(32)
#undef LIFE_BG
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_group(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells,
                              int64_t gens, hipStream_t s) {
    return launch_group(p, nx, ny, count, cells, gens, nullptr, s);
}

hipError_t launch_batch_group_trace(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells,
                                    int64_t gens, uint32_t *trace, hipStream_t s) {
    if (!trace || count * gens > kBatchTraceEntries) return hipErrorInvalidValue;
    return launch_group(p, nx, ny, count, cells, gens, trace, s);
}

hipError_t launch_batch_census(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, const uint32_t *cells,
                               unsigned long long *live, unsigned long long *sum, hipStream_t s) {
    if (!grid_ok((count + kBatchWaves - 1) / kBatchWaves)) return hipErrorInvalidValue;
    batch_census_kernel<<<wave_blocks(count), 64 * kBatchWaves, 0, s>>>(cells, live, sum, count, nx, ny, p.words);
    return hipGetLastError();
}

hipError_t launch_batch_import(const BatchPlan &p, int64_t nx, int64_t ny, int64_t n, const uint8_t *dense,
                               uint32_t *cells, hipStream_t s) {
    const int64_t words = n * ny * p.words;
    if (words < 1) return hipSuccess;
    batch_import_kernel<<<word_blocks(words), 256, 0, s>>>(dense, cells, words, nx, ny, p.words);
    return hipGetLastError();
}

hipError_t launch_batch_export(const BatchPlan &p, int64_t nx, int64_t ny, int64_t n, const uint32_t *cells,
                               uint8_t *dense, hipStream_t s) {
    const int64_t words = n * ny * p.words;
    if (words < 1) return hipSuccess;
    batch_export_kernel<<<word_blocks(words), 256, 0, s>>>(cells, dense, words, nx, ny, p.words);
    return hipGetLastError();
}

hipError_t launch_batch_fill(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint64_t seed, uint32_t thr32,
                             uint32_t *cells, hipStream_t s) {
    const int64_t words = count * ny * p.words;
    if (words < 1) return hipSuccess;
    batch_fill_kernel<<<word_blocks(words), 256, 0, s>>>(cells, words, nx, ny, p.words, seed, thr32);
    return hipGetLastError();
}

hipError_t launch_batch_gen(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells, uint32_t *decay,
                            int planes, int64_t gens, uint32_t birth, uint32_t survive, uint32_t states,
                            const uint32_t *rules, bool settle, int64_t *settled, bool cycle, int64_t *period,
                            int64_t *found, int64_t gen0, hipStream_t s) {
    if (p.tier != LIFE_BATCH_TIER_WAVE || gens < 1 || gens > INT32_MAX || (settle && !settled) || (settle && cycle) ||
        (cycle && (!period || !found)) || !decay || !grid_ok((count + kBatchWaves - 1) / kBatchWaves))
        return hipErrorInvalidValue;
    BNArgs a{};
    a.cells = cells;
    a.decay = decay;
    a.plane = count * ny * p.words;
    a.settled = settled;
    a.count = count;
    a.gen0 = gen0;
    a.nx = (int32_t)nx;
    a.ny = (int32_t)ny;
    a.gens = (int32_t)gens;
    a.birth = birth | states << 16;
    a.survive = survive;
    a.rules = reinterpret_cast<const uint2 *>(rules);
    a.period = period;
    a.found = found;
    const int det = cycle ? kCycle : settle ? kSettle : kNoDetector;
    const unsigned blocks = wave_blocks(count);
    switch (p.words * 8 + planes) {
#define LIFE_BN(N) \
    case N * 8 + 1: return launch_gen<N, 1>(a, det, blocks, s); \
    case N * 8 + 2: return launch_gen<N, 2>(a, det, blocks, s); \
    case N * 8 + 4: return launch_gen<N, 4>(a, det, blocks, s);
        LIFE_BN(1) LIFE_BN(2) LIFE_BN(3) LIFE_BN(4)
#undef LIFE_BN
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_batch_onset_gen(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, uint32_t *cells,
                                  uint32_t *decay, int planes, int64_t gens, uint32_t birth, uint32_t survive,
                                  uint32_t states, const uint32_t *rules, int64_t *period, int64_t *found,
                                  int64_t *onset, int64_t gen0, hipStream_t s) {
    if (p.tier != LIFE_BATCH_TIER_WAVE || gens < 1 || gens > INT32_MAX || !period || !found || !onset || !decay ||
        !grid_ok((count + kBatchWaves - 1) / kBatchWaves))
        return hipErrorInvalidValue;
    BMArgs o{};
    BNArgs &a = o.n;
    a.cells = cells;
    a.decay = decay;
    a.plane = count * ny * p.words;
    a.count = count;
    a.gen0 = gen0;
    a.nx = (int32_t)nx;
    a.ny = (int32_t)ny;
    a.gens = (int32_t)gens;
    a.birth = birth | states << 16;
    a.survive = survive;
    a.rules = reinterpret_cast<const uint2 *>(rules);
    a.period = period;
    a.found = found;
    o.onset = onset;
    const unsigned blocks = wave_blocks(count);
    switch (p.words * 8 + planes) {
#define LIFE_BM(N, Q) \
    case N * 8 + Q: \
        batch_onset_gen_kernel<N, Q><<<blocks, 64 * kBatchWaves, 0, s>>>(o); \
        return hipGetLastError();
        LIFE_BM(1, 1) LIFE_BM(1, 2) LIFE_BM(1, 4) LIFE_BM(2, 1) LIFE_BM(2, 2) LIFE_BM(2, 4)
        LIFE_BM(3, 1) LIFE_BM(3, 2) LIFE_BM(3, 4) LIFE_BM(4, 1) LIFE_BM(4, 2) LIFE_BM(4, 4)
#undef LIFE_BM
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_batch_import_states(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, int64_t first,
                                      int64_t n, const uint8_t *dense, uint32_t *cells, uint32_t *decay, int planes,
                                      hipStream_t s) {
    const int64_t words = n * ny * p.words, skip = first * ny * p.words;
    if (words < 1) return hipSuccess;
    if (planes < 0 || planes > 4 || (planes && !decay)) return hipErrorInvalidValue;
    batch_import_states_kernel<<<word_blocks(words), 256, 0, s>>>(dense, cells + skip, planes ? decay + skip : nullptr,
                                                                  count * ny * p.words, planes, words, nx, ny, p.words);
    return hipGetLastError();
}

hipError_t launch_batch_export_states(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, int64_t first,
                                      int64_t n, const uint32_t *cells, const uint32_t *decay, int planes,
                                      uint8_t *dense, hipStream_t s) {
    const int64_t words = n * ny * p.words, skip = first * ny * p.words;
    if (words < 1) return hipSuccess;
    if (planes < 0 || planes > 4 || (planes && !decay)) return hipErrorInvalidValue;
    batch_export_states_kernel<<<word_blocks(words), 256, 0, s>>>(cells + skip, planes ? decay + skip : nullptr,
                                                                  count * ny * p.words, planes, dense, words, nx, ny,
                                                                  p.words);
    return hipGetLastError();
}

hipError_t launch_batch_census_states(const BatchPlan &p, int64_t nx, int64_t ny, int64_t count, const uint32_t *cells,
                                      const uint32_t *decay, int planes, unsigned long long *live,
                                      unsigned long long *dying, unsigned long long *sum, hipStream_t s) {
    if (!grid_ok((count + kBatchWaves - 1) / kBatchWaves) || planes < 0 || planes > 4 || (planes && !decay))
        return hipErrorInvalidValue;
    batch_census_states_kernel<<<wave_blocks(count), 64 * kBatchWaves, 0, s>>>(cells, decay, count * ny * p.words,
                                                                               planes, live, dying, sum, count, nx, ny,
                                                                               p.words);
    return hipGetLastError();
}

}  // namespace life
