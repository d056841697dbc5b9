// life_plan.cpp -- host-only partition, layout and halo plan (no HIP calls,
// callable without a GPU).
//
// Replaces the reference's MPI Cartesian set-up and exchange schedule:
//   MPI_Dims_create / MPI_Cart_create / MPI_Cart_coords  life_cart.c:117-121
//   decomposition()                                      life_cart.c:217-223
//   exchange_columns / exchange_rows / exchange_corners  life_cart.c:225-279
// The corner messages are dropped: columns go first, then rows of width+2
// carry the freshly received column apron (the corners) along.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "life_env.h"
#include "life_host.h"
#include "life_mi355x.h"
#include "life_tile_decode.h"

namespace {
constexpr int64_t kXoff = 128;  // owned x = 0 starts 128 B into a padded row
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline int cart_rank(int c0, int c1, int dims1) { return c0 * dims1 + c1; }
}  // namespace

extern "C" {

void life_decomposition(int64_t n, int p, int k, int64_t *start, int64_t *stop) {
    const int64_t l = n / p;  // life_cart.c:218
    *start = l * k;
    *stop = *start + l;
    if (k == p - 1) *stop = n;  // the last block takes the remainder (:221-222)
}

void life_dims_create(int n, int dims[2]) {
    // MPI_Dims_create(n, 2, {0,0}): most balanced factor pair, non-increasing.
    int d1 = 1;
    for (int f = 1; (int64_t)f * f <= n; f++)
        if (n % f == 0) d1 = f;
    dims[0] = n / d1;
    dims[1] = d1;
}

int life_dims_choose(int64_t nx, int64_t ny, int n, int policy, int dims[2]) {
    if (!dims || n < 1 || nx <= 0 || ny <= 0) return LIFE_EINVAL;
    switch (policy) {
    case LIFE_PARTITION_CART: life_dims_create(n, dims); break;
    case LIFE_PARTITION_ROWS: dims[0] = 1, dims[1] = n; break;
    case LIFE_PARTITION_COLS: dims[0] = n, dims[1] = 1; break;
    case LIFE_PARTITION_AUTO:
        // the shortest strip (the decomposition remainder goes to the last)
        if (ny / n >= LIFE_AUTO_MIN_STRIP_ROWS)
            dims[0] = 1, dims[1] = n;
        else
            life_dims_create(n, dims);
        break;
    default: return LIFE_EINVAL;
    }
    if (nx < dims[0] || ny < dims[1]) return LIFE_EINVAL;
    return LIFE_OK;
}

// Generations per halo exchange of the temporally blocked layout, per
// encoding: LIFE_TEMPORAL_DEPTH (bit) / LIFE_TEMPORAL_DEPTH_BYTE, or 8 / 12 /
// 16 / 24 / 32 from the environment variables of the same names (read once; every rank
// of a job must see the same values); 1 selects the one-generation layouts
// (a measurement knob: the HBM-bound kernels).  The byte encoding moves 8x
// the bytes per cell, so it amortises each HBM pass over more generations.
static int env_depth(const life::env::IntKnob &k) {
    const int v = life::env::read(k);
    return v == 1 || v == 8 || v == 12 || v == 16 || v == 24 || v == 32 ? v : k.dflt;
}
static int temporal_depth(int kernel) {
    static const int kbit = env_depth(life::env::kTemporalDepth);
    static const int kbyte = [] {  // the byte tiles are built for 16 or 32 ghost rows
        const int v = env_depth(life::env::kTemporalDepthByte);
        return v == 1 || v == 16 ? v : 32;
    }();
    return kernel == LIFE_KERNEL_BIT ? kbit : kbyte;
}

// The temporally blocked stencil keeps one lane column of x-apron -- 64
// cells (one interleaved pair) for the bit encoding, 32 for the byte
// encoding -- and K-row y-aprons: every block must be at least that wide (a
// neighbour, or the shard itself when x wraps inside it, fills the apron
// columns) and, on a partitioned y axis, at least K rows tall.
static int64_t temporal_xapron(int kernel) { return kernel == LIFE_KERNEL_BIT ? 64 : 32; }
static bool temporal_ok(int64_t nx, int64_t ny, int dims0, int dims1, int K, int64_t xa) {
    for (int k = 0; k < dims0; k++) {
        int64_t s, e;
        life_decomposition(nx, dims0, k, &s, &e);
        if (e - s < xa) return false;
    }
    if (dims1 > 1)
        for (int k = 0; k < dims1; k++) {
            int64_t s, e;
            life_decomposition(ny, dims1, k, &s, &e);
            if (e - s < K) return false;
        }
    return true;
}

int life_layout_query(int64_t nx, int64_t ny, int dims0, int dims1, int rank, int kernel,
                      life_layout *out) {
    if (!out || nx <= 0 || ny <= 0 || dims0 <= 0 || dims1 <= 0 || rank < 0 ||
        rank >= dims0 * dims1 || (kernel != LIFE_KERNEL_BYTE && kernel != LIFE_KERNEL_BIT))
        return LIFE_EINVAL;
    if (nx < dims0 || ny < dims1) return LIFE_EINVAL;  // no empty blocks
    memset(out, 0, sizeof *out);
    const int c0 = rank / dims1, c1 = rank % dims1;  // MPI_Cart_coords, row-major
    int64_t xs, xe, ys, ye;
    life_decomposition(nx, dims0, c0, &xs, &xe);
    life_decomposition(ny, dims1, c1, &ys, &ye);
    out->w = xe - xs;
    out->h = ye - ys;
    out->x0 = xs;
    out->y0 = ys;
    out->kernel = kernel;
    out->coords[0] = c0;
    out->coords[1] = c1;
    const int K = temporal_depth(kernel);
    const int64_t xa = temporal_xapron(kernel);
    const bool temporal = K > 1 && temporal_ok(nx, ny, dims0, dims1, K, xa);
    out->xapron = temporal ? xa : 1;
    out->yapron = temporal ? K : 1;
    out->generations_per_exchange = temporal ? K : 1;
    const int64_t cells_per_unit = kernel == LIFE_KERNEL_BIT ? 128 : 16;
    out->units = (out->w + cells_per_unit - 1) / cells_per_unit;
    out->xoff = kXoff;
    // room for the last unit, the right apron (a cell, one 64-cell pair, or 32
    // byte cells) and the right extra dword; the temporal byte stencil reads
    // whole 32-byte words up to the one holding cell w+31
    out->pitch = round_up(kXoff + 16 * out->units + (temporal && kernel == LIFE_KERNEL_BYTE ? 64 : 16), 256);
    out->rows = out->h + 2 * out->yapron;
    return LIFE_OK;
}

}  // extern "C"

int64_t life::flow_chunk_passes(int64_t tiles, int64_t grid, int64_t cap) {
    if (tiles < 1 || grid < 0 || cap < 0) return 0;
    // items = passes * tiles; pulls = items + grid (each workgroup's last pull
    // finds the queue empty) must stay <= kFlowMaxHead
    int64_t n = (kFlowMaxHead - grid) / tiles;
    if (n < 0) n = 0;
    return cap > 0 && cap < n ? cap : n;
}

life::PassPlan life::next_pass(int K, int bmax, bool deep, int since, int64_t remaining) {
    int64_t seg = remaining;
    if (deep && since < K) seg = std::min(seg, (int64_t)(K - since));
    const int64_t n = (seg + bmax - 1) / bmax;
    PassPlan p;
    p.m = (int)((seg + n - 1) / n);
    p.refill_first = since + p.m > K;
    if (p.refill_first) since = 0;
    const bool last = remaining == p.m;
    p.extend = deep && since + p.m < K && !(last && since + p.m + bmax > K);
    p.ext = K - since - p.m;
    return p;
}

life::PipePlan life::pipe_plan(int64_t nty, int64_t B, int R, int S) {
    PipePlan p;
    if (R < 3 || R > kPipeMaxRegions || S < 1 || S > kPipeMaxStreams || nty < 2 * (int64_t)R) return p;
    p.R = R;
    p.S = S;
    // regions: whole bands when each region can hold one, else whole tile rows;
    // the rows the unit does not divide go to the last region
    p.aligned = B > 1 && nty / B >= R;
    const int64_t unit = p.aligned ? B : 1, units = nty / unit;
    p.ty[0] = 0;
    for (int r = 0; r < R; r++) p.ty[r + 1] = p.ty[r] + unit * (units / R + (r < units % R ? 1 : 0));
    p.ty[R] = nty;
    // waits: passes 0 and 1 with a vector clock per launch -- know[i][s] = the
    // latest launch of stream s known to have finished when launch i starts
    int know[2 * kPipeMaxRegions][kPipeMaxStreams];
    for (int i = 0; i < 2 * R; i++) {
        int *k = know[i];
        for (int s = 0; s < S; s++) k[s] = i >= S ? know[i - S][s] : -1;
        if (i >= S) k[i % S] = i - S;  // stream order
        if (i < R) continue;           // pass 0: the fence before it only
        const int j = i - R;
        int need[3];
        for (int dr = -1; dr <= 1; dr++) need[dr + 1] = ((j + dr + 1) % R + R) % R;  // launch index in pass 0
        std::sort(need, need + 3, [](int a, int b) { return a > b; });                // the latest first
        for (int q : need) {
            if (k[q % S] >= q) continue;
            p.wait[j][p.nwait[j]++] = i - q;
            for (int s = 0; s < S; s++) k[s] = std::max(k[s], know[q][s]);
            k[q % S] = std::max(k[q % S], q);
        }
    }
    for (int j = 0; j < R; j++)
        for (int w = 0; w < p.nwait[j]; w++) p.record[((j - p.wait[j][w]) % R + R) % R] = true;
    return p;
}

int life::halo_op_slot(const life_halo_op *ops, int i) {
    int n = 0;
    for (int k = 0; k < i; k++) n += ops[k].phase == ops[i].phase && ops[k].kind == ops[i].kind && ops[k].what == ops[i].what;
    return n;
}

int life::halo_match_send(const life_halo_op *mine, int recv, int rank, const life_halo_op *peer_ops, int npeer) {
    const life_halo_op &o = mine[recv];
    int kth = 0;  // this is the kth recv from o.peer in its phase
    for (int k = 0; k < recv; k++)
        kth += mine[k].phase == o.phase && mine[k].kind == LIFE_HALO_RECV && mine[k].peer == o.peer;
    for (int k = 0; k < npeer; k++) {
        const life_halo_op &q = peer_ops[k];
        if (q.phase == o.phase && q.kind == LIFE_HALO_SEND && q.peer == rank && kth-- == 0) return k;
    }
    return -1;
}

int life::halo_wait_peers(const life_halo_op *ops, int n, int rank, int phase, int kind, int *peers) {
    int ns = 0;
    for (int i = 0; i < n; i++) {
        if (ops[i].phase != phase || ops[i].kind != kind || ops[i].peer == rank) continue;
        if (std::find(peers, peers + ns, ops[i].peer) == peers + ns) peers[ns++] = ops[i].peer;
    }
    return ns;
}

int64_t life::gather_frame_row_bytes(int64_t nx, int fmt) {
    return fmt == kGatherBits ? (nx + 7) / 8 : nx * (fmt == kGatherVtk ? 2 : 1);
}

int life::gather_plan(int64_t nx, int64_t ny, int dims0, int dims1, int kernel, int fmt, GatherPiece *pieces,
                      int max, int64_t *slot_bytes) {
    if (dims0 < 1 || dims1 < 1 || fmt < kGatherDense || fmt > kGatherBits || !pieces || !slot_bytes) return LIFE_EINVAL;
    const int world = dims0 * dims1;
    if (max < world) return LIFE_EINVAL;
    const int root = world - 1;  // life_collect: cart rank of (dims0-1, dims1-1)
    const int64_t frb = gather_frame_row_bytes(nx, fmt);
    int64_t big = 0;
    for (int k = 0; k < world; k++) {
        const int r = k == 0 ? root : k - 1;  // the root's own block, then the fan-in order
        life_layout L;
        if (life_layout_query(nx, ny, dims0, dims1, r, kernel, &L) != LIFE_OK) return LIFE_EINVAL;
        GatherPiece &p = pieces[k];
        p.rank = r;
        p.slot = k == 0 ? -1 : (k - 1) % 2;
        p.row_bytes = fmt == kGatherBits ? ((L.x0 & 7) + L.w + 7) / 8 : L.w * (fmt == kGatherVtk ? 2 : 1);
        p.rows = L.h;
        p.bytes = p.row_bytes * p.rows;
        p.dst = L.y0 * frb + (fmt == kGatherBits ? (L.x0 >> 3) : L.x0 * (fmt == kGatherVtk ? 2 : 1));
        p.shared_first = fmt == kGatherBits && (L.x0 & 7) != 0;
        p.shared_last = fmt == kGatherBits && ((L.x0 + L.w) & 7) != 0 && L.x0 + L.w < nx;
        if (p.bytes > big) big = p.bytes;
    }
    *slot_bytes = big;
    return world;
}

// The halo plan; `loop` (bit 0: x, bit 1: y) treats that axis, which the
// shard spans whole (dims == 1), as partitioned too, with the shard as its own
// left and right neighbour (LIFE_OPT_LOOPBACK: the transport's send/recv path
// exercised by one rank).
int life::halo_plan(int64_t nx, int64_t ny, int dims0, int dims1, int rank, int kernel, int loop,
                    life_halo_op *ops, int max_ops) {
    life_layout L;
    const int rc = life_layout_query(nx, ny, dims0, dims1, rank, kernel, &L);
    if (rc != LIFE_OK) return rc;
    const int c0 = L.coords[0], c1 = L.coords[1];
    const int64_t w = L.w, h = L.h, xa = L.xapron, ya = L.yapron;
    life_halo_op tmp[16];
    int n = 0;
    auto add = [&](int phase, int kind, int peer, int what, int64_t index, int64_t width, int64_t first,
                   int64_t count) {
        life_halo_op &o = tmp[n++];
        o.phase = phase;
        o.kind = kind;
        o.peer = peer;
        o.what = what;
        o.index = index;
        o.width = width;
        o.first = first;
        o.count = count;
    };
    const bool px = dims0 > 1 || (loop & 1), py = dims1 > 1 || (loop & 2);
    // Both axes exchanged by messages with K-deep temporal aprons: ONE phase
    // (one RCCL group per exchange instead of two back to back, round 5):
    // columns, whole padded rows (their x-apron bytes are stale and are
    // overwritten), and the four K x xapron corners explicitly, as
    // life_cart.c:257-273 exchanges them (there one cell each).  Sends go in
    // direction order E, W, S, N, SE, SW, NE, NW; each receive is listed in
    // the order of the direction its sender sends in, so the k-th message
    // between two ranks pairs up however many directions they share (dims 2,
    // the loopback's self).  Corners are received into staging and unpacked
    // after the group, over the stale row bytes.  Not for the loopback (the
    // shard its own peer in all eight directions): RCCL ran the sixteen
    // self-messages of one group in 39 us, longer than the two groups of the
    // column and row phases (19 + 14 us; 16384 x 32768, profiles/r05/g),
    // while distinct peers over xGMI are served by separate channels.
    const bool fused = px && py && L.generations_per_exchange > 1 && loop == 0;
    const int ph_rows = fused ? 0 : 1;
    // Phase 0: columns (dim 0 splits x), owned rows only.  MPI_Cart_shift(dim 0).
    if (!px) {
        add(0, LIFE_HALO_FILL, -1, LIFE_HALO_COLUMN, -xa, xa, ya, h);
    } else {
        const int right = cart_rank((c0 + 1) % dims0, c1, dims1);
        const int left = cart_rank((c0 - 1 + dims0) % dims0, c1, dims1);
        // life_cart.c:251-254 order: Send right, Recv left, Send left, Recv right.
        add(0, LIFE_HALO_SEND, right, LIFE_HALO_COLUMN, w - xa, xa, ya, h);
        add(0, LIFE_HALO_SEND, left, LIFE_HALO_COLUMN, 0, xa, ya, h);
        add(0, LIFE_HALO_RECV, left, LIFE_HALO_COLUMN, -xa, xa, ya, h);
        add(0, LIFE_HALO_RECV, right, LIFE_HALO_COLUMN, w, xa, ya, h);
    }
    // Phase 1 (phase 0 when fused): whole rows including the x-apron just
    // received (the corners), or with a stale x-apron the corners overwrite.
    if (!py) {
        add(1, LIFE_HALO_FILL, -1, LIFE_HALO_ROW, 0, ya, -xa, w + 2 * xa);
    } else {
        const int right = cart_rank(c0, (c1 + 1) % dims1, dims1);
        const int left = cart_rank(c0, (c1 - 1 + dims1) % dims1, dims1);
        // life_cart.c:235-238 order.  Padded row of owned row y is y + ya.
        add(ph_rows, LIFE_HALO_SEND, right, LIFE_HALO_ROW, h, ya, -xa, w + 2 * xa);
        add(ph_rows, LIFE_HALO_SEND, left, LIFE_HALO_ROW, ya, ya, -xa, w + 2 * xa);
        add(ph_rows, LIFE_HALO_RECV, left, LIFE_HALO_ROW, 0, ya, -xa, w + 2 * xa);
        add(ph_rows, LIFE_HALO_RECV, right, LIFE_HALO_ROW, h + ya, ya, -xa, w + 2 * xa);
    }
    if (fused) {
        // direction d = (dx, dy) in the order SE, SW, NE, NW; the shard at
        // (c0 + dx, c1 + dy) gets my corner next to it: x side by dx (my right
        // column w - xa, or cells [0, xa)), rows by dy (my bottom K rows,
        // padded h, or my top K, padded ya)
        static const int kDir[4][2] = {{1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
        auto at = [&](int dx, int dy) {
            return cart_rank((c0 + dx + dims0) % dims0, (c1 + dy + dims1) % dims1, dims1);
        };
        for (const auto &d : kDir)
            add(0, LIFE_HALO_SEND, at(d[0], d[1]), LIFE_HALO_CORNER, d[0] > 0 ? w - xa : 0, xa, d[1] > 0 ? h : ya,
                ya);
        // the sender of direction d sits at -d: its corner lands in my apron
        // on the side facing it (left apron -xa when it is left of me)
        for (const auto &d : kDir)
            add(0, LIFE_HALO_RECV, at(-d[0], -d[1]), LIFE_HALO_CORNER, d[0] > 0 ? -xa : w, xa,
                d[1] > 0 ? 0 : h + ya, ya);
    }
    if (ops) {
        if (max_ops < n) return LIFE_EINVAL;
        memcpy(ops, tmp, sizeof(life_halo_op) * n);
    }
    return n;
}

extern "C" {

int life_halo_plan(int64_t nx, int64_t ny, int dims0, int dims1, int rank, int kernel,
                   life_halo_op *ops, int max_ops) {
    return life::halo_plan(nx, ny, dims0, dims1, rank, kernel, 0, ops, max_ops);
}

const char *life_strerror(int err) {
    switch (err) {
    case LIFE_OK: return "success";
    case LIFE_EINVAL: return "invalid argument";
    case LIFE_EHIP: return "HIP runtime error";
    case LIFE_ERCCL: return "RCCL error";
    case LIFE_ENOMEM: return "out of memory";
    case LIFE_ESTATE: return "invalid state";
    case LIFE_EIO: return "I/O or parse error";
    default: return "unknown error";
    }
}

// SURVEY 8(b)'s proposed name for the same function
const char *life_dev_strerror(int err) { return life_strerror(err); }

}  // extern "C"

// ---- Life-like rules (life_host.h)
life::RuleWords life::rule_words(uint32_t birth, uint32_t survive) {
    RuleWords w;
    for (int alive = 0; alive < 2; alive++)
        for (int s = 0; s < 5; s++) {
            const RuleLeaf leaf = rule_leaf(birth, survive, alive, s);
            w.a[alive][s] = leaf.a;
            w.b[alive][s] = leaf.b;
        }
    return w;
}

uint32_t life::conway7_host(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0, uint32_t c1,
                            uint32_t alive) {
    const uint32_t p = bitop3_host(kR7Par, a0, b0, c0), n = bitop3_host(kR7Nae, a0, b0, c0);
    const uint32_t x = bitop3_host(kR7Par, a1, b1, c1), y = bitop3_host(kR7Nae, a1, b1, c1);
    const uint32_t g1 = bitop3_host(kR7G1, p, n, y);
    const uint32_t g2 = bitop3_host(kR7G2, n, x, g1);
    return bitop3_host(kR7Out, p, alive, g2);
}

namespace {
// digits 0-8 up to `end` (a '/' or the NUL) into a mask
bool rule_digits(const char *&p, char end, uint32_t *mask) {
    *mask = 0;
    for (; *p != end; ++p) {
        if (*p < '0' || *p > '8') return false;
        *mask |= 1u << (*p - '0');
    }
    return true;
}
}  // namespace

bool life::rule_parse(const char *text, uint32_t *birth, uint32_t *survive) {
    if (!text || !*text) return false;
    const char *p = text;
    uint32_t b = 0, s = 0;
    if (*p == 'B' || *p == 'b') {  // B.../S...
        ++p;
        if (!rule_digits(p, '/', &b)) return false;
        ++p;
        if (*p != 'S' && *p != 's') return false;
        ++p;
        if (!rule_digits(p, '\0', &s)) return false;
    } else {  // S/B
        if (!rule_digits(p, '/', &s)) return false;
        ++p;
        if (!rule_digits(p, '\0', &b)) return false;
    }
    *birth = b;
    *survive = s;
    return true;
}

void life::rule_format(uint32_t birth, uint32_t survive, char out[24]) {
    char *p = out;
    *p++ = 'B';
    for (int k = 0; k <= 8; k++)
        if ((birth >> k) & 1u) *p++ = (char)('0' + k);
    *p++ = '/';
    *p++ = 'S';
    for (int k = 0; k <= 8; k++)
        if ((survive >> k) & 1u) *p++ = (char)('0' + k);
    *p = '\0';
}

bool life::rule_parse_gen(const char *text, uint32_t *birth, uint32_t *survive, uint32_t *states) {
    if (!text) return false;
    const char *s1 = strchr(text, '/');
    const char *s2 = s1 ? strchr(s1 + 1, '/') : nullptr;
    if (!s2) {  // no third part: a Life-like rule
        *states = 2;
        return rule_parse(text, birth, survive);
    }
    // the first two parts are rule_parse's, the third the state count: one or two digits, no leading zero
    const std::string head(text, (size_t)(s2 - text));
    const char *p = s2 + 1;
    if (*p == 'C' || *p == 'c' || *p == 'G' || *p == 'g') ++p;
    if (*p < '1' || *p > '9') return false;
    uint32_t c = (uint32_t)(*p++ - '0');
    if (*p >= '0' && *p <= '9') c = 10 * c + (uint32_t)(*p++ - '0');
    if (*p != '\0' || c < 2 || c > kGenMaxStates) return false;
    if (!rule_parse(head.c_str(), birth, survive)) return false;
    *states = c;
    return true;
}

void life::rule_format_gen(uint32_t birth, uint32_t survive, uint32_t states, char out[32]) {
    rule_format(birth, survive, out);
    if (states > 2) snprintf(out + strlen(out), 8, "/C%u", states);
}

// life_last_error's setter lives with the device runtime (life_dev.hip); a
// program that links this unit alone (the CPU harnesses) has none
namespace life {
namespace rt {
__attribute__((weak, visibility("hidden"))) void set_err(const char *fmt, ...);
}
}  // namespace life

extern "C" {

int life_rule_parse(const char *text, uint32_t *birth, uint32_t *survive) {
    if (birth && survive && life::rule_parse(text, birth, survive)) return LIFE_OK;
    if (life::rt::set_err)
        life::rt::set_err("rule \"%.64s\": expected B<digits>/S<digits> or <digits>/<digits> (S/B), digits 0-8",
                          text ? text : "(null)");
    return LIFE_EINVAL;
}

int life_rule_format(uint32_t birth, uint32_t survive, char out[24]) {
    if (!out || ((birth | survive) & ~life::kRuleMask)) {
        if (life::rt::set_err) life::rt::set_err("rule masks 0x%x / 0x%x: bits above 8", birth, survive);
        return LIFE_EINVAL;
    }
    life::rule_format(birth, survive, out);
    return LIFE_OK;
}

int life_rule_parse_gen(const char *text, uint32_t *birth, uint32_t *survive, uint32_t *states) {
    if (birth && survive && states && life::rule_parse_gen(text, birth, survive, states)) return LIFE_OK;
    if (life::rt::set_err)
        life::rt::set_err("rule \"%.64s\": expected B<digits>/S<digits> or <digits>/<digits> (S/B), digits 0-8, with "
                          "an optional third part /C<states> (G for C; S/B/<states>), states 2-%u",
                          text ? text : "(null)", life::kGenMaxStates);
    return LIFE_EINVAL;
}

int life_rule_format_gen(uint32_t birth, uint32_t survive, uint32_t states, char out[32]) {
    if (!out || ((birth | survive) & ~life::kRuleMask) || states < 2 || states > life::kGenMaxStates) {
        if (life::rt::set_err)
            life::rt::set_err("rule masks 0x%x / 0x%x, %u states: bits above 8 or states outside 2-%u", birth, survive,
                              states, life::kGenMaxStates);
        return LIFE_EINVAL;
    }
    life::rule_format_gen(birth, survive, states, out);
    return LIFE_OK;
}

int life_batch_query(int64_t nx, int64_t ny, int *tier, int64_t *bytes_per_universe) {
    const life::BatchPlan p = life::batch_plan(nx, ny);
    if (p.tier == 0) {
        if (life::rt::set_err) life::rt::set_err("%s", p.why);
        return LIFE_EINVAL;
    }
    if (tier) *tier = p.tier;
    if (bytes_per_universe) *bytes_per_universe = p.bytes;
    return LIFE_OK;
}

int life_batch_query_plan(int64_t nx, int64_t ny, int *tier, int *words, int *lanes_per_strip, int *rows, int *strips,
                          int *threads) {
    const life::BatchPlan p = life::batch_plan(nx, ny);
    if (p.tier == 0) {
        if (life::rt::set_err) life::rt::set_err("%s", p.why);
        return LIFE_EINVAL;
    }
    const bool group = p.tier == LIFE_BATCH_TIER_GROUP;
    if (tier) *tier = p.tier;
    if (words) *words = p.words;
    if (lanes_per_strip) *lanes_per_strip = group ? 1 << p.lg_wp : 0;
    if (rows) *rows = group ? p.rows : 0;
    if (strips) *strips = group ? p.strips : 0;
    if (threads) *threads = 64 * p.waves_per_group;
    return LIFE_OK;
}

int life_tile_decode_query(const life_tile_launch *launch, const int64_t *wg, int64_t n, life_tile_item *out) {
    life::TileDec d;
    const char *why = "null argument";
    if (!launch || n < 0 || (n > 0 && (!wg || !out)) || !life::tile_decode_fill(*launch, &d, &why)) {
        if (life::rt::set_err) life::rt::set_err("tile launch description: %s", why);
        return LIFE_EINVAL;
    }
    for (int64_t i = 0; i < n; i++) {
        if (wg[i] < 0 || wg[i] > 0x7FFFFFFFll) {  // a launch holds fewer than 2^31 workgroups
            if (life::rt::set_err) life::rt::set_err("workgroup id %lld outside [0, 2^31)", (long long)wg[i]);
            return LIFE_EINVAL;
        }
        const life::TileItem t = life::tile_decode(d, (uint32_t)wg[i]);
        out[i] = life_tile_item{t.kind, t.region, t.tx, t.ty, t.ty0, t.rows, (int64_t)t.bi};
    }
    return LIFE_OK;
}

}  // extern "C"

// ---- batches (life_host.h)
life::BatchPlan life::batch_plan(int64_t nx, int64_t ny) {
    BatchPlan p;
    auto fail = [&](const char *what) {
        snprintf(p.why, sizeof p.why,
                 "batch of %lld x %lld universes: %s (wave tier: nx <= %lld and ny <= %lld; group tier: nx <= %lld and "
                 "ny = strips x R rows, R in 1 2 3 4 5 6 8 10 12 16 20 25 32, strips x lanes per strip <= %d)",
                 (long long)nx, (long long)ny, what, (long long)kBatchWaveMaxX, (long long)kBatchWaveMaxY,
                 (long long)kBatchGroupMaxX, kBatchGroupThreads);
        return p;
    };
    if (nx < 1 || ny < 1) return fail("empty shape");
    if (nx > kBatchGroupMaxX) return fail("too wide");
    p.words = (int)((nx + 31) / 32);
    if (nx <= kBatchWaveMaxX && ny <= kBatchWaveMaxY) {
        p.tier = LIFE_BATCH_TIER_WAVE;
        p.bytes = 4 * (int64_t)p.words * ny;
        p.waves_per_group = kBatchWaves;
        p.universes_per_group = kBatchWaves;
        return p;
    }
    while ((1 << p.lg_wp) < p.words) ++p.lg_wp;
    const int64_t strips = kBatchGroupThreads >> p.lg_wp;
    static const int kRows[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 25, 32};  // life_kernels.hip kRegRows
    for (int R : kRows)
        if (ny % R == 0 && ny / R <= strips) {
            p.tier = LIFE_BATCH_TIER_GROUP;
            p.bytes = 4 * (int64_t)p.words * ny;  // of an accepted shape only: ny is any int64 before this
            p.rows = R;
            p.strips = (int)(ny / R);
            p.waves_per_group = (int)((((int64_t)p.strips << p.lg_wp) + 63) / 64);
            p.universes_per_group = 1;
            return p;
        }
    p.words = 0;
    return fail("no strip height fits one workgroup");
}

namespace {
// Slots grouped by the time they fall free (a list schedule of a few item
// kinds keeps a handful of distinct free times).
struct SlotGroups {
    static constexpr int kMax = 32;
    double t[kMax];
    int64_t c[kMax];
    int n = 0;
    void add(double tt, int64_t cc) {
        for (int i = 0; i < n; i++)
            if (t[i] > tt - 1e-9 && t[i] < tt + 1e-9) {
                c[i] += cc;
                return;
            }
        if (n < kMax) {
            t[n] = tt;
            c[n++] = cc;
            return;
        }
        // (never reached at the shapes planned: merge into the latest group, which
        // only makes the estimate pessimistic)
        int j = 0;
        for (int i = 1; i < n; i++)
            if (t[i] > t[j]) j = i;
        if (tt > t[j]) t[j] = tt;
        c[j] += cc;
    }
    // deals `items` items of duration d, returns the latest end
    double deal(double d, int64_t items, double end) {
        while (items > 0 && n > 0) {
            int i = 0;
            for (int k = 1; k < n; k++)
                if (t[k] < t[i]) i = k;
            const int64_t k = c[i] < items ? c[i] : items;
            items -= k;
            const double nt = t[i] + d;
            if (k == c[i]) {
                t[i] = t[--n];
                c[i] = c[n];
            } else {
                c[i] -= k;
            }
            add(nt, k);
            if (nt > end) end = nt;
        }
        return end;
    }
};

struct TailKey {
    int64_t nfull, B0, B1, ty0, ty1, yend, T, T2, slots, pre;
    int nb, mode;
    double c;
    bool operator==(const TailKey &o) const {
        return nfull == o.nfull && nb == o.nb && B0 == o.B0 && B1 == o.B1 && ty0 == o.ty0 && ty1 == o.ty1 &&
               yend == o.yend && T == o.T && T2 == o.T2 && slots == o.slots && pre == o.pre && mode == o.mode &&
               c == o.c;
    }
};
// the one-band forms' column count and band as a band list
int64_t one_band_full(int64_t ntx, int64_t B) { return B > 1 ? ntx - 1 : ntx; }
life::BandRows one_band(int64_t B) {
    life::BandRows b;
    if (B > 1) {
        b.n = 1;
        b.B[0] = B;
    }
    return b;
}
}  // namespace

life::BandSplit life::band_split(int64_t o, int max_parts) {
    BandSplit s;
    if (o < 1 || o > 62) return s;
    // lanes of the smallest group holding x owned pairs (x <= 30)
    auto gsh_of = [](int64_t x) {
        int g = 2;
        while ((1 << g) < x + 2) ++g;
        return g;
    };
    int best = 64;  // a whole tile
    if (o <= 30) {
        s.n = 1;
        s.b[0] = BandCol{0, (int)o, gsh_of(o)};
        best = 1 << s.b[0].gsh;
    }
    // two parts {a, o - a}: strictly fewer lanes only, the widest first part first
    for (int64_t a = std::min<int64_t>(o - 1, 30); max_parts > 1 && a >= 1 && o - a <= 30; --a) {
        const int g0 = gsh_of(a), g1 = gsh_of(o - a), lanes = (1 << g0) + (1 << g1);
        if (lanes >= best) continue;
        best = lanes;
        s.n = 2;
        s.b[0] = BandCol{0, (int)a, g0};
        s.b[1] = BandCol{(int)a, (int)(o - a), g1};
    }
    return s;
}

double life::tail_makespan2(int64_t ntx, int64_t B, int64_t F_rows, int64_t n2, int64_t slots, double c,
                            int64_t pre) {
    return tail_makespan2(one_band_full(ntx, B), one_band(B), F_rows, n2, slots, c, pre);
}

life::TailPlan life::tail_plan(int64_t ntx, int64_t B, int64_t ty0, int64_t ty1, int64_t yend, int64_t T,
                               int64_t T2, int64_t slots, int mode, double c, int64_t pre) {
    if (ntx < 1) {
        TailPlan none;
        none.F = ty1;
        return none;
    }
    return tail_plan(one_band_full(ntx, B), one_band(B), ty0, ty1, yend, T, T2, slots, mode, c, pre);
}

double life::tail_makespan2(int64_t nfull, const BandRows &bands, int64_t F_rows, int64_t n2, int64_t slots,
                            double c, int64_t pre) {
    if (slots < 1) return 0.0;
    const int64_t nf = (pre > 0 ? pre : 0) + tail_row_items(nfull, bands, F_rows);
    const int64_t r = nf / slots, rem = nf % slots;
    SlotGroups g;
    g.add((double)r, slots - rem);
    if (rem) g.add((double)(r + 1), rem);
    const double end = nf ? (double)(r + (rem ? 1 : 0)) : 0.0;
    return g.deal(c + (1.0 - c) * 0.5, tail_row_items(nfull, bands, n2), end);
}

life::TailPlan life::tail_plan(int64_t nfull, const BandRows &bands, int64_t ty0, int64_t ty1, int64_t yend,
                               int64_t T, int64_t T2, int64_t slots, int mode, double c, int64_t pre) {
    TailPlan none;
    none.F = ty1;
    if (nfull < 0 || nfull + bands.n < 1 || bands.n < 0 || bands.n > kMaxBands || ty1 <= ty0 || T < 1 || T2 < 1 || slots < 1 || mode < 1 || mode > 2 || pre < 0) return none;
    // the launch shares the slots with `pre` items dispatched before it
    const int64_t nall = pre + tail_row_items(nfull, bands, ty1 - ty0);
    none.makespan = tail_makespan2(nfull, bands, ty1 - ty0, 0, slots, c, pre);
    // Whole rounds: nothing to fill.  One round or less: the model's slots are
    // not independent there (a CU's three slots share its SIMDs, and a lone
    // tile runs faster), so it is not trusted to re-tile an underfilled launch.
    if (nall <= slots || nall % slots == 0) return none;
    static std::mutex mu;
    static std::vector<std::pair<TailKey, TailPlan>> cache;
    const TailKey key{nfull, bands.n > 0 ? bands.B[0] : 1, bands.n > 1 ? bands.B[1] : 1, ty0, ty1, yend, T, T2, slots, pre,
                      bands.n, mode, c};
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const auto &e : cache)
            if (e.first == key) return e.second;
    }
    TailPlan best = none;
    auto halves = [&](int64_t F) -> int64_t {
        const int64_t left = yend - F * T;
        return left > 0 ? (left + T2 - 1) / T2 : 0;
    };
    if (mode == 1) {
        // round 4's rule: the fewest bottom rows whose half tiles fill one
        // round, when the last round is under half full
        if (nall % slots <= slots / 2) {
            int64_t q = 1;
            while (q < ty1 - ty0 && tail_row_items(nfull, bands, (q * T + T2 - 1) / T2) < slots) ++q;
            if (q < ty1 - ty0) {
                best.F = ty1 - q;
                best.n2 = halves(best.F);
                best.makespan = tail_makespan2(nfull, bands, best.F - ty0, best.n2, slots, c, pre);
            }
        }
    } else {
        // every split point (ties keep more full tiles)
        for (int64_t F = ty1 - 1; F >= ty0; --F) {
            const int64_t n2 = halves(F);
            const double t = tail_makespan2(nfull, bands, F - ty0, n2, slots, c, pre);
            if (t < best.makespan - 1e-9) {
                best.F = F;
                best.n2 = n2;
                best.makespan = t;
            }
        }
    }
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() >= 512) cache.erase(cache.begin());
    cache.emplace_back(key, best);
    return best;
}
