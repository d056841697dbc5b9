// life_frames.hip -- moving cells in and out of the device runtime: upload
// and random fill, life_collect in its three frame formats (dense / VTK /
// LIFEBITS gather), the census, the sparse I/O (clear, cell lists, packed-frame
// upload, window readout and paste, density maps) and the copy benchmark.
#include "life_dev_internal.h"

using namespace life::rt;

extern "C" {

int life_dev_upload(life_dev *d, const uint8_t *grid) {
    if (!d || !grid) return LIFE_EINVAL;
    d->act_valid = false;  // every writer of the state drops the activity maps (LIFE_OPT_SKIP_DEAD)
    for (Shard &s : d->shards) {
        const life_layout &L = s.lay;
        HIPCHK(hipSetDevice(s.device));
        uint8_t *stage = nullptr;
        HIPCHK(hipMalloc(&stage, (size_t)(L.w * L.h)));
        // `grid` is the caller's pageable memory: the copy is ordered on the
        // shard's stream (not the null stream, which does not order against
        // the non-blocking shard streams) and waited for before this call
        // returns, so the caller may reuse `grid` at once.
        HIPCHK(hipMemcpy2DAsync(stage, (size_t)L.w, grid + L.y0 * d->nx + L.x0, (size_t)d->nx, (size_t)L.w,
                                (size_t)L.h, hipMemcpyHostToDevice, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        HIPCHK(life::launch_import_block(L, stage, s.buf[s.cur], s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        HIPCHK(hipFree(stage));
    }
    CHK(exchange(d, 0, false));
    return life_dev_sync(d);
}

int life_dev_fill_random(life_dev *d, uint64_t seed, uint32_t thr32) {
    if (!d) return LIFE_EINVAL;
    d->act_valid = false;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull;  // key = splitmix64(seed)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    const uint64_t key = z ^ (z >> 31);
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(life::launch_fill_random(s.lay, d->nx, key, thr32, s.buf[s.cur], s.stream));
    }
    CHK(exchange(d, 0, false));
    return LIFE_OK;
}

}  // extern "C"

namespace {
// Device staging of one shard's export, kept between calls (a 65536^2 grid's
// frame is 4 GiB dense / 8 GiB as VTK text: no allocation per frame).
int stage_buffer(Shard &s, size_t bytes, uint8_t **out) {
    if (s.stage_bytes < bytes) {
        if (s.stage) HIPCHK(hipFree(s.stage));
        s.stage = nullptr;
        s.stage_bytes = 0;
        HIPCHK(hipMalloc(&s.stage, bytes));
        s.stage_bytes = bytes;
    }
    *out = s.stage;
    return LIFE_OK;
}

// life_collect in one of three frame formats: DENSE 0/1 cells (export
// kernel, 1 B per cell), VTK "%d\n" cell text (vtk kernel, 2 B per cell) or
// BITS packed rows (bits kernel, LIFEBITS: bit x & 7 of byte x >> 3).  Every
// shard exports its block on the device; in-process shards copy straight into
// place, rank mode sends the blocks to the root (world-1) over RCCL in the
// order of life::gather_plan.
enum class Frame { DENSE = life::kGatherDense, VTK = life::kGatherVtk, BITS = life::kGatherBits };

int gather_impl(life_dev *d, uint8_t *out, Frame fmt) {
    const int root = d->world - 1;  // life_collect: cart rank of (dims0-1, dims1-1)
    const bool have_root = find_local(d, root) != nullptr;
    if (have_root && !out) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    std::vector<life::GatherPiece> plan((size_t)d->world);
    int64_t slot = 0;
    if (life::gather_plan(d->nx, d->ny, d->dims[0], d->dims[1], d->kernel, (int)fmt, plan.data(), d->world,
                          &slot) != d->world) {
        set_err("gather plan failed");
        return LIFE_EINVAL;
    }
    auto piece_of = [&](int rank) -> const life::GatherPiece & {
        for (const life::GatherPiece &p : plan)
            if (p.rank == rank) return p;
        return plan[0];  // unreachable: every rank has a piece
    };
    const int64_t frb = life::gather_frame_row_bytes(d->nx, (int)fmt);
    auto export_block = [&](Shard &s, uint8_t **stage) -> int {
        const life_layout &L = s.lay;
        CHK(stage_buffer(s, (size_t)piece_of(s.rank).bytes, stage));
        if (fmt == Frame::DENSE)
            HIPCHK(life::launch_export_block(L, s.buf[s.cur], *stage, s.stream));
        else if (fmt == Frame::VTK)
            HIPCHK(life::launch_vtk_block(L, s.buf[s.cur], *stage, s.stream));
        else
            HIPCHK(life::launch_bits_block(L, s.buf[s.cur], *stage, s.stream));
        return LIFE_OK;
    };
    // BITS: a byte holding cells of two blocks (a block edge at x % 8 != 0)
    // is OR-ed together from both exports; those frame bytes start at 0
    std::vector<uint8_t> tmp;
    // `out` is the caller's pageable memory: each copy is ordered on the
    // stream that produced `src` (never the null stream) and waited for.
    auto place = [&](const life::GatherPiece &p, const uint8_t *src, hipStream_t st) -> int {
        const int64_t rb = p.row_bytes;
        uint8_t *dst = out + p.dst;
        if (!p.shared_first && !p.shared_last) {
            HIPCHK(hipMemcpy2DAsync(dst, (size_t)frb, src, (size_t)rb, (size_t)rb, (size_t)p.rows,
                                    hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            return LIFE_OK;
        }
        tmp.resize((size_t)p.bytes);
        HIPCHK(hipMemcpyAsync(tmp.data(), src, tmp.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const bool f = p.shared_first, l = p.shared_last;
        for (int64_t y = 0; y < p.rows; y++) {
            uint8_t *o = dst + y * frb;
            const uint8_t *t = tmp.data() + y * rb;
            const int64_t a = f ? 1 : 0, b = l ? rb - 1 : rb;
            if (b > a) memcpy(o + a, t + a, (size_t)(b - a));
            if (f) o[0] |= t[0];
            if (l && (rb > 1 || !f)) o[rb - 1] |= t[rb - 1];
        }
        return LIFE_OK;
    };
    if (fmt == Frame::BITS && have_root) {
        // zero the shared bytes of every block boundary (all ranks' blocks)
        for (const life::GatherPiece &p : plan)
            if (p.shared_first)
                for (int64_t y = 0; y < p.rows; y++) out[p.dst + y * frb] = 0;
    }
    if (!d->rank_mode) {
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            uint8_t *stage;
            CHK(export_block(s, &stage));
        }
        for (Shard &s : d->shards) {  // every export is queued before the first copy waits
            HIPCHK(hipSetDevice(s.device));
            HIPCHK(hipStreamSynchronize(s.stream));
            CHK(place(piece_of(s.rank), s.stage, s.stream));
        }
        return LIFE_OK;
    }
    Shard &s = d->shards[0];
    HIPCHK(hipSetDevice(s.device));
    uint8_t *stage;
    CHK(export_block(s, &stage));
    if (s.rank != root) {
        if (!s.comm) {
            set_err("gather: rank %d has no communicator", s.rank);
            return LIFE_ESTATE;
        }
        NCCLCHK(ncclSend(stage, (size_t)piece_of(s.rank).bytes, ncclUint8, root, s.comm, s.stream));
        return bounded_sync(s, "gather: send to the root", root);
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    // The root's own block sits in the front of the staging buffer; two
    // receive slots follow.  Block k+1 arrives over RCCL (non-blocking
    // stream) while the host copies block k out of the other slot (on the
    // idle second compute stream, into the caller's pageable memory), so the
    // fan-in of world-1 blocks is not serialised behind the D2H copies.
    CHK(place(plan[0], stage, s.stream));  // copied out first: the buffer may grow below
    CHK(stage_buffer(s, 2 * (size_t)slot, &stage));
    if (d->world > 1 && !s.comm) {
        set_err("gather: the root has no communicator");
        return LIFE_ESTATE;
    }
    for (size_t k = 1; k < plan.size(); k++) {
        const life::GatherPiece &p = plan[k];
        if (k == 1) NCCLCHK(ncclRecv(stage, (size_t)p.bytes, ncclUint8, p.rank, s.comm, s.stream));
        CHK(bounded_sync(s, "gather: receive at the root", p.rank));  // block k is in slot p.slot
        if (k + 1 < plan.size()) {
            const life::GatherPiece &q = plan[k + 1];
            NCCLCHK(ncclRecv(stage + (size_t)q.slot * (size_t)slot, (size_t)q.bytes, ncclUint8, q.rank, s.comm,
                             s.stream));
        }
        CHK(place(p, stage + (size_t)p.slot * (size_t)slot, s.stream2));
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    return LIFE_OK;
}
}  // namespace

extern "C" {

int life_dev_gather(life_dev *d, uint8_t *grid) {
    if (!d) return LIFE_EINVAL;
    return gather_impl(d, grid, Frame::DENSE);
}

int life_dev_gather_vtk(life_dev *d, char *body) {
    if (!d) return LIFE_EINVAL;
    return gather_impl(d, reinterpret_cast<uint8_t *>(body), Frame::VTK);
}

int life_dev_gather_bits(life_dev *d, uint8_t *packed) {
    if (!d) return LIFE_EINVAL;
    return gather_impl(d, packed, Frame::BITS);
}

static int census(life_dev *d, unsigned long long out[2]) {
    out[0] = out[1] = 0;
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipMemsetAsync(s.d_count, 0, 2 * sizeof(unsigned long long), s.stream));
        HIPCHK(life::launch_census(s.lay, d->nx, s.buf[s.cur], s.d_count, s.stream));
        if (d->rank_mode && s.comm)
            NCCLCHK(ncclAllReduce(s.d_count, s.d_count, 2, ncclUint64, ncclSum, s.comm, s.stream));
        HIPCHK(hipMemcpyAsync(s.h_count, s.d_count, 2 * sizeof *s.h_count, hipMemcpyDeviceToHost, s.stream));
        CHK(bounded_sync(s, "census all-reduce", -1));  // pinned destination
        out[0] += s.h_count[0];
        out[1] += s.h_count[1];
    }
    return LIFE_OK;
}

int64_t life_dev_live_count(life_dev *d) {
    if (!d) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    unsigned long long c[2];
    CHK(census(d, c));
    return (int64_t)c[0];
}

int life_dev_checksum(life_dev *d, uint64_t *sum) {
    if (!d || !sum) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    unsigned long long c[2];
    CHK(census(d, c));
    *sum = (uint64_t)c[1];
    return LIFE_OK;
}

// ---- sparse I/O: nothing of size nx*ny on the host or over PCIe ----

int life_dev_clear(life_dev *d) {
    if (!d) return LIFE_EINVAL;
    CHK(life_dev_sync(d));  // behind the work on all three streams
    d->act_valid = false;
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipMemsetAsync(s.buf[s.cur], 0, (size_t)(s.lay.pitch * s.lay.rows), s.stream));
    }
    CHK(exchange(d, 0, false));  // as life_dev_upload: the deep-halo count restarts
    return life_dev_sync(d);
}

int life_dev_set_cells(life_dev *d, const int64_t *xy, int64_t n, int alive) {
    if (!d || n < 0 || (n > 0 && !xy)) return LIFE_EINVAL;
    if (n == 0) return LIFE_OK;
    d->act_valid = false;
    CHK(life_dev_sync(d));  // the edit orders behind the work on all three streams
    constexpr int64_t kChunk = 1 << 20;  // pairs staged at a time (16 MiB)
    for (int64_t i = 0; i < n; i += kChunk) {
        const int64_t m = std::min(kChunk, n - i);
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            uint8_t *stage;
            CHK(stage_buffer(s, (size_t)m * 2 * sizeof(int64_t), &stage));
            // `xy` is the caller's pageable memory: ordered on the shard's
            // stream and waited for (see life_dev_upload)
            HIPCHK(hipMemcpyAsync(stage, xy + 2 * i, (size_t)m * 2 * sizeof(int64_t), hipMemcpyHostToDevice, s.stream));
            HIPCHK(life::launch_set_cells(s.lay, d->nx, d->ny, reinterpret_cast<const int64_t *>(stage), m, alive,
                                          s.buf[s.cur], s.stream));
        }
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            HIPCHK(hipStreamSynchronize(s.stream));
        }
    }
    // Every apron is refilled K deep from the edited blocks, FILL ops and the
    // self-wrapped x-apron included; a part-used deep halo (d->since > 0) held
    // cells advanced from the state before the edit: exchange() restarts it.
    CHK(exchange(d, 0, false));
    return life_dev_sync(d);
}

int life_dev_upload_bits(life_dev *d, const uint8_t *packed) {
    if (!d || !packed) return LIFE_EINVAL;
    d->act_valid = false;
    CHK(life_dev_sync(d));  // as life_dev_set_cells
    const int64_t frb = (d->nx + 7) / 8;  // the frame's row bytes (64-bit offsets: 4 GiB at 2^35 cells)
    for (Shard &s : d->shards) {
        const life_layout &L = s.lay;
        HIPCHK(hipSetDevice(s.device));
        // the byte columns [x0 >> 3, (x0 + w + 7) >> 3) of the shard's rows: a
        // byte two blocks share (an edge at x % 8 != 0) goes to both, and the
        // kernel keeps each one's cells
        const int64_t rb = life::bits_row_bytes(L), sp = life::unbits_pitch(L);
        uint8_t *stage;
        CHK(stage_buffer(s, (size_t)(sp * L.h), &stage));
        // `packed` is the caller's pageable memory: ordered on the shard's
        // stream and waited for (see life_dev_upload)
        HIPCHK(hipMemcpy2DAsync(stage, (size_t)sp, packed + L.y0 * frb + (L.x0 >> 3), (size_t)frb, (size_t)rb,
                                (size_t)L.h, hipMemcpyHostToDevice, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        // timing on: the unpack launch takes an event pair of its own and is
        // counted by life_dev_kernel_stats (no bytes are booked for it)
        Bracket b;
        CHK(bracket_begin(d, s, true, 1, kExtNever, true, s.stream, &b));
        HIPCHK(life::launch_unbits_block(L, stage, s.buf[s.cur], s.stream));
        CHK(bracket_end(b, s.stream));
    }
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    CHK(exchange(d, 0, false));  // every apron K deep, the deep-halo count restarts (see life_dev_set_cells)
    return life_dev_sync(d);
}

namespace {
// The pieces of the periodic interval [a, a + len) (a in [0, n), len <= n)
// inside the block [b0, b0 + bl): at most two, the block seen at b0 and at
// b0 + n.  out: window offset, block offset, length.
struct Span {
    int64_t win, blk, len;
};
int wrapped_spans(int64_t a, int64_t len, int64_t n, int64_t b0, int64_t bl, Span out[2]) {
    int k = 0;
    for (int64_t shift = 0; shift <= n; shift += n) {
        const int64_t lo = std::max(a, b0 + shift), hi = std::min(a + len, b0 + shift + bl);
        if (hi > lo) out[k++] = Span{lo - a, lo - b0 - shift, hi - lo};
    }
    return k;
}
int64_t floor_mod(int64_t v, int64_t n) {
    const int64_t r = v % n;
    return r < 0 ? r + n : r;
}
// A shard whose readout is combined with the other ranks' over RCCL.
bool reduces(const life_dev *d, const Shard &s) { return d->rank_mode && s.comm; }
}  // namespace

int life_dev_gather_rect(life_dev *d, int64_t x0, int64_t y0, int64_t w, int64_t h, uint8_t *cells) {
    if (!d || !cells || w < 1 || h < 1 || w > d->nx || h > d->ny) return LIFE_EINVAL;
    CHK(life_dev_sync(d));
    const int64_t ax = floor_mod(x0, d->nx), ay = floor_mod(y0, d->ny);
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        const life_layout &L = s.lay;
        Span sx[2], sy[2];
        const int kx = wrapped_spans(ax, w, d->nx, L.x0, L.w, sx), ky = wrapped_spans(ay, h, d->ny, L.y0, L.h, sy);
        // the window in device memory, row pitch w: this shard's pieces in place
        uint8_t *win;
        CHK(stage_buffer(s, (size_t)(w * h), &win));
        const bool red = reduces(d, s);
        if (red) HIPCHK(hipMemsetAsync(win, 0, (size_t)(w * h), s.stream));
        for (int j = 0; j < ky; j++)
            for (int i = 0; i < kx; i++)
                HIPCHK(life::launch_rect_piece(L, s.buf[s.cur], sx[i].blk, sy[j].blk, sx[i].len, sy[j].len,
                                               win + sy[j].win * w + sx[i].win, w, s.stream));
        if (red) {
            // rank mode: every rank's pieces summed into every rank's window (as census())
            NCCLCHK(ncclAllReduce(win, win, (size_t)(w * h), ncclUint8, ncclSum, s.comm, s.stream));
            HIPCHK(hipMemcpyAsync(cells, win, (size_t)(w * h), hipMemcpyDeviceToHost, s.stream));
            CHK(bounded_sync(s, "gather_rect all-reduce", -1));
            continue;
        }
        // `cells` is the caller's pageable memory: each copy ordered on the
        // stream that produced the piece, and waited for
        for (int j = 0; j < ky; j++)
            for (int i = 0; i < kx; i++) {
                const size_t off = (size_t)(sy[j].win * w + sx[i].win);
                HIPCHK(hipMemcpy2DAsync(cells + off, (size_t)w, win + off, (size_t)w, (size_t)sx[i].len,
                                        (size_t)sy[j].len, hipMemcpyDeviceToHost, s.stream));
            }
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    return LIFE_OK;
}

int life_dev_set_rect(life_dev *d, int64_t x0, int64_t y0, int64_t w, int64_t h, const uint8_t *cells) {
    if (!d || !cells || w < 1 || h < 1 || w > d->nx || h > d->ny) return LIFE_EINVAL;
    d->act_valid = false;
    CHK(life_dev_sync(d));  // the edit orders behind the work on all three streams
    const int64_t ax = floor_mod(x0, d->nx), ay = floor_mod(y0, d->ny);
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        const life_layout &L = s.lay;
        Span sx[2], sy[2];
        const int kx = wrapped_spans(ax, w, d->nx, L.x0, L.w, sx), ky = wrapped_spans(ay, h, d->ny, L.y0, L.h, sy);
        if (kx == 0 || ky == 0) continue;  // the window misses this block
        // the window in device memory, row pitch w; `cells` is the caller's
        // pageable memory: ordered on the shard's stream and waited for below
        uint8_t *win;
        CHK(stage_buffer(s, (size_t)(w * h), &win));
        HIPCHK(hipMemcpyAsync(win, cells, (size_t)(w * h), hipMemcpyHostToDevice, s.stream));
        // in order on the one stream: with w == nx and x0 % 64 != 0 the two
        // pieces of a row share a 64-cell pair
        for (int j = 0; j < ky; j++)
            for (int i = 0; i < kx; i++)
                HIPCHK(life::launch_paste_piece(L, s.buf[s.cur], sx[i].blk, sy[j].blk, sx[i].len, sy[j].len,
                                                win + sy[j].win * w + sx[i].win, w, s.stream));
    }
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    CHK(exchange(d, 0, false));  // as life_dev_set_cells: every apron refilled, a part-used deep halo restarted
    return life_dev_sync(d);
}

int life_dev_gather_density(life_dev *d, int64_t fx, int64_t fy, uint32_t *counts) {
    if (!d || !counts || fx < 1 || fy < 1) return LIFE_EINVAL;
    if ((unsigned __int128)fx * (unsigned __int128)fy >= ((unsigned __int128)1 << 32)) return LIFE_EINVAL;
    if (fx > d->nx) fx = d->nx;  // factors beyond the grid: one bin
    if (fy > d->ny) fy = d->ny;
    CHK(life_dev_sync(d));
    const int64_t bw = (d->nx + fx - 1) / fx, bh = (d->ny + fy - 1) / fy;
    const size_t nbins = (size_t)(bw * bh);
    std::vector<uint32_t> part_map;  // in-process shards after the first: added on the host
    bool first = true;
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        uint8_t *stage;
        CHK(stage_buffer(s, nbins * sizeof(uint32_t), &stage));
        uint32_t *map = reinterpret_cast<uint32_t *>(stage);
        HIPCHK(hipMemsetAsync(map, 0, nbins * sizeof(uint32_t), s.stream));
        HIPCHK(life::launch_density(s.lay, s.buf[s.cur], fx, fy, bw, map, s.stream));
        if (reduces(d, s))
            NCCLCHK(ncclAllReduce(map, map, nbins, ncclUint32, ncclSum, s.comm, s.stream));
        uint32_t *dst = counts;
        if (!first) {
            part_map.resize(nbins);
            dst = part_map.data();
        }
        HIPCHK(hipMemcpyAsync(dst, map, nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
        CHK(bounded_sync(s, "gather_density all-reduce", -1));
        if (!first)
            for (size_t k = 0; k < nbins; k++) counts[k] += part_map[k];
        first = false;
    }
    return LIFE_OK;
}

int life_measure_copy(int device, int64_t bytes, int reps, double *gbps) {
    if (!gbps || bytes < 16 || bytes % 16 || reps < 1) return LIFE_EINVAL;
    HIPCHK(hipSetDevice(device));
    void *a = nullptr, *b = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = LIFE_OK;
    float best = 0.f;
    auto run = [&]() -> int {
        HIPCHK(hipMalloc(&a, (size_t)bytes));
        HIPCHK(hipMalloc(&b, (size_t)bytes));
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipMemsetAsync(a, 1, (size_t)bytes, st));
        HIPCHK(life::launch_copy(a, b, bytes, st));  // warm-up (page mapping, clocks)
        for (int r = 0; r < reps; r++) {
            HIPCHK(hipEventRecord(e0, st));
            HIPCHK(life::launch_copy(a, b, bytes, st));
            HIPCHK(hipEventRecord(e1, st));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            if (best == 0.f || ms < best) best = ms;
        }
        return LIFE_OK;
    };
    rc = run();
    if (st) (void)hipStreamSynchronize(st);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (rc == LIFE_OK) *gbps = 2.0 * (double)bytes / (best * 1e-3) / 1e9;
    return rc;
}

}  // extern "C"
