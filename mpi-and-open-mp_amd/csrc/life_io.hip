// life_io.hip -- the data-movement kernels around the stencil: halo column
// staging, dense import / export, the VTK and LIFEBITS formatters, the random
// fill, the census, the sparse-I/O kernels and the copy-ceiling probe.  None
// of them is near the roofline; they live apart from life_kernels.hip so that
// a new output format does not touch the stencil's code object.
#include "life_io.h"
#include "life_act.h"
#include "life_bitops.h"

#include <stdint.h>

namespace life {
namespace {

// The block's view of its padded buffer, by value in every kernel here
// (buffer pointers stay separate parameters: their const-ness shows).  Owned
// cell (x, y) lives in row buf + (y + ya) * pitch, from byte xoff on; w x h
// owned cells, `units` 16-byte units per owned row, (gx0, gy0) the block's
// first cell in the global grid.  A kernel unpacks it in its first line:
//   const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
struct BlockView {
    int64_t pitch, ya, xoff, w, h, units, gx0, gy0;
};
inline BlockView view(const life_layout &L) {
    return BlockView{L.pitch, L.yapron, L.xoff, L.w, L.h, L.units, L.x0, L.y0};
}

// ------------------------------------------------------------------ cell access
// Byte: cell x of a padded row at row[xoff + x].  Bit: the pair layout
// (life_bitops.h): bit pair_bit(x) of dword pair_dword(x) counted from
// row + xoff (x may be negative: the left apron).
__device__ __forceinline__ uint32_t get_cell(const uint8_t *row, int64_t xoff, int64_t x, bool bit) {
    if (!bit) return row[xoff + x];
    const uint32_t *w = reinterpret_cast<const uint32_t *>(row + xoff);
    return (w[pair_dword(x)] >> pair_bit(x)) & 1u;
}
__device__ __forceinline__ void set_cell(uint8_t *row, int64_t xoff, int64_t x, uint32_t v, bool bit) {
    if (!bit) {
        row[xoff + x] = (uint8_t)v;
        return;
    }
    uint32_t *w = reinterpret_cast<uint32_t *>(row + xoff) + pair_dword(x);
    const uint32_t m = 1u << pair_bit(x);
    *w = (*w & ~m) | (v ? m : 0u);
}

// Column halo staging.  Cell columns (xapron == 1): one byte 0/1 per row.
// Temporal layouts: the bit encoding's x-apron is one pair (64 cells, 8 B
// per row and side, sent in pair form), the byte encoding's 32 byte cells.
// The left column (cells [0, 64)) is pair 0; the right one (cells [w-64,
// w)) and the right apron (cells [w, w+64)) straddle two pairs when w % 64 !=
// 0: they go through the natural 64-bit order (nat64 / pair_of), a funnel
// shift on the way out, a merge that keeps the owned cells on the way in.
__device__ __forceinline__ uint64_t pair_nat(const uint32_t *wd, int64_t p) { return nat64(wd[2 * p], wd[2 * p + 1]); }
__device__ __forceinline__ void put_pair(uint32_t *wd, int64_t p, uint64_t v) {
    const uint2 q = pair_of(v);
    wd[2 * p] = q.x;
    wd[2 * p + 1] = q.y;
}
__device__ __forceinline__ uint64_t right_column_bits(const uint32_t *wd, int64_t w) {  // cells [w-64, w), w >= 64
    const int64_t x = w - 64, p = x >> 6;
    const uint32_t s = (uint32_t)(x & 63);
    if (s == 0) return pair_nat(wd, p);
    return (pair_nat(wd, p) >> s) | (pair_nat(wd, p + 1) << (64 - s));
}
__device__ __forceinline__ void put_right_apron_bits(uint32_t *wd, int64_t w, uint64_t v) {  // cells [w, w+64)
    const int64_t p = w >> 6;
    const uint32_t s = (uint32_t)(w & 63);
    if (s == 0) {
        put_pair(wd, p, v);
        return;
    }
    const uint64_t keep = (1ull << s) - 1ull;  // the owned cells of the partial pair
    put_pair(wd, p, (pair_nat(wd, p) & keep) | (v << s));
    put_pair(wd, p + 1, v >> (64 - s));  // cells beyond w+63: never read as owned
}
__device__ __forceinline__ void copy32(uint8_t *dst, const uint8_t *src) {
    // byte-cell columns need not be 4-byte aligned (w % 4 != 0)
    for (int k = 0; k < 32; ++k) dst[k] = src[k];
}

// Threads [h, h + 4K) of a corner exchange (temporal layouts, K = ya): the
// owned row a send-slot corner c comes from -- c = 0, 1 (SE, SW): the bottom
// K rows; c = 2, 3 (NE, NW): the top K -- and whether it is the right
// column (c even) or pair 0 / the first 32 cells (c odd).  The receive slot
// c lands in apron row -K + r (c = 0, 1) or h + r (c = 2, 3), x-apron left
// (c even) or right (c odd).
__global__ void pack_columns_kernel(const uint8_t *buf, const BlockView blk, int64_t xa, uint8_t *stage, bool bit,
                                    int64_t nc) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= h + nc) return;
    bool right = true, left = true;  // columns: both (slot y and slot h + y)
    int64_t out = y, lo = h + y;     // the stage entries of the right column and of pair 0 / cells [0, 32)
    if (y >= h) {                    // corner c, row r: one entry
        const int64_t c = (y - h) / ya, r = (y - h) % ya;
        out = lo = y + h;  // entries 2h + cK + r
        right = (c & 1) == 0;
        left = !right;
        y = c < 2 ? h - ya + r : r;
    }
    const uint8_t *row = buf + (y + ya) * pitch;
    if (xa == 64 && bit) {
        const uint32_t *wd = reinterpret_cast<const uint32_t *>(row + xoff);
        uint64_t *st = reinterpret_cast<uint64_t *>(stage);
        if (right) {
            const uint2 r = pair_of(right_column_bits(wd, w));
            st[out] = (uint64_t)r.x | ((uint64_t)r.y << 32);
        }
        if (left) st[lo] = *reinterpret_cast<const uint64_t *>(wd);  // pair 0
        return;
    }
    if (xa == 32) {  // 32 byte cells per row and side
        if (right) copy32(stage + 32 * out, row + xoff + w - 32);
        if (left) {
            const uint4 *l = reinterpret_cast<const uint4 *>(row + xoff);
            uint4 *st = reinterpret_cast<uint4 *>(stage + 32 * lo);
            st[0] = l[0];
            st[1] = l[1];
        }
        return;
    }
    stage[y] = (uint8_t)get_cell(row, xoff, w - 1, bit);
    stage[h + y] = (uint8_t)get_cell(row, xoff, 0, bit);
}

__global__ void unpack_columns_kernel(uint8_t *buf, const BlockView blk, int64_t xa, const uint8_t *stage, bool bit,
                                      int64_t nc) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= h + nc) return;
    bool left = true, right = true;  // columns: slot y -> left apron, slot h + y -> right apron
    int64_t in = y, ri = h + y;
    if (y >= h) {  // corner c, row r: apron rows -K + r (c < 2) or h + r, left apron for even c
        const int64_t c = (y - h) / ya, r = (y - h) % ya;
        in = ri = y + h;
        left = (c & 1) == 0;
        right = !left;
        y = c < 2 ? r - ya : h + r;
    }
    uint8_t *row = buf + (y + ya) * pitch;
    if (xa == 64 && bit) {
        uint32_t *wd = reinterpret_cast<uint32_t *>(row + xoff);
        const uint64_t *st = reinterpret_cast<const uint64_t *>(stage);
        if (left) reinterpret_cast<uint64_t *>(wd)[-1] = st[in];  // pair -1 = cells [-64, 0)
        if (right) {
            const uint64_t r = st[ri];
            put_right_apron_bits(wd, w, nat64((uint32_t)r, (uint32_t)(r >> 32)));
        }
        return;
    }
    if (xa == 32) {
        if (left) {
            uint4 *l = reinterpret_cast<uint4 *>(row + xoff - 32);
            const uint4 *st = reinterpret_cast<const uint4 *>(stage + 32 * in);
            l[0] = st[0];
            l[1] = st[1];
        }
        if (right) copy32(row + xoff + w, stage + 32 * ri);
        return;
    }
    set_cell(row, xoff, -1, stage[y] ? 1u : 0u, bit);
    set_cell(row, xoff, w, stage[h + y] ? 1u : 0u, bit);
}

// Periodic x inside one shard of a temporal layout whose width is not a
// multiple of the lane column (64 bit cells / 32 byte cells; the tiles' WRAPX
// reads whole lane columns): the shard is its own left and right neighbour,
// so the aprons are filled from its own columns.
__global__ void wrap_columns_kernel(uint8_t *buf, const BlockView blk, bool bit) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= h) return;
    uint8_t *row = buf + (y + ya) * pitch;
    if (bit) {
        uint32_t *wd = reinterpret_cast<uint32_t *>(row + xoff);
        const uint64_t l = pair_nat(wd, 0), r = right_column_bits(wd, w);
        put_pair(wd, -1, r);
        put_right_apron_bits(wd, w, l);
        return;
    }
    copy32(row + xoff - 32, row + xoff + w - 32);
    copy32(row + xoff + w, row + xoff);
}

// One thread per 16-byte unit of an owned row: dense (row pitch w) -> padded.
template <int CPU>  // cells per unit: 16 (byte) or 128 (bit)
__global__ void import_kernel(const uint8_t *dense, uint8_t *buf, const BlockView blk) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= units * h) return;
    const int64_t u = i % units, y = i / units;
    const uint8_t *in = dense + y * w;
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    const int64_t x0 = u * CPU;
    for (int k = 0; k < CPU; ++k) {
        const int64_t x = x0 + k;
        if (x >= w) break;
        const uint32_t v = in[x] != 0;
        if (CPU == 16)
            word[k >> 2] |= v << (8 * (k & 3));
        else
            word[pair_dword(k)] |= v << pair_bit(k);  // a unit = two interleaved pairs
    }
    *reinterpret_cast<uint4 *>(buf + (y + ya) * pitch + xoff + 16 * u) =
        make_uint4(word[0], word[1], word[2], word[3]);
}

template <int CPU>
__global__ void export_kernel(const uint8_t *buf, uint8_t *dense, const BlockView blk) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= units * h) return;
    const int64_t u = i % units, y = i / units;
    const uint4 q = *reinterpret_cast<const uint4 *>(buf + (y + ya) * pitch + xoff + 16 * u);
    const uint32_t word[4] = {q.x, q.y, q.z, q.w};
    uint8_t *o = dense + y * w;
    const int64_t x0 = u * CPU;
    for (int k = 0; k < CPU; ++k) {
        const int64_t x = x0 + k;
        if (x >= w) break;
        o[x] = CPU == 16 ? (uint8_t)((word[k >> 2] >> (8 * (k & 3))) & 0xFFu)
                         : (uint8_t)((word[pair_dword(k)] >> pair_bit(k)) & 1u);
    }
}

// VTK CELL_DATA body of a block (life_save_vtk, life_cart.c:181-185: "%d\n"
// per cell, x fastest): 2 bytes per cell, '0'/'1' then '\n', row pitch 2w.
// One thread per 8 cells of a row (16 output bytes); 2-D grid, y strides rows.
__device__ __forceinline__ uint64_t vtk4(uint32_t cells4) {  // 4 cells, bit k -> ASCII pair k
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v |= (uint64_t)(0x0A30u | ((cells4 >> k) & 1u)) << (16 * k);
    return v;
}
template <bool BIT>
__global__ void vtk_kernel(const uint8_t *buf, const BlockView blk, uint8_t *out) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t x0 = 8 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (x0 >= w) return;
    const int n = w - x0 < 8 ? (int)(w - x0) : 8;
    const bool vec = (w & 7) == 0;  // 16-B aligned output rows
    for (int64_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t *row = buf + (y + ya) * pitch + xoff;
        uint32_t c;  // cell k at bit k
        if (BIT) {
            // x0 is a multiple of 8: four even cells from E, four odd from O
            const uint32_t *wd = reinterpret_cast<const uint32_t *>(row) + 2 * (x0 >> 6);
            const uint32_t sh = (uint32_t)((x0 & 63) >> 1);
            c = nat32((wd[0] >> sh) & 15u, (wd[1] >> sh) & 15u);
        } else {
            c = 0;
            for (int k = 0; k < n; ++k) c |= (uint32_t)(row[x0 + k] & 1u) << k;
        }
        uint8_t *o = out + y * 2 * w + 2 * x0;
        if (vec && n == 8) {
            *reinterpret_cast<uint4 *>(o) = make_uint4((uint32_t)vtk4(c), (uint32_t)(vtk4(c) >> 32),
                                                       (uint32_t)vtk4(c >> 4), (uint32_t)(vtk4(c >> 4) >> 32));
        } else {
            for (int k = 0; k < n; ++k) {
                o[2 * k] = (uint8_t)('0' + ((c >> k) & 1u));
                o[2 * k + 1] = '\n';
            }
        }
    }
}

// Packed frame rows of a block (the driver's LIFEBITS checkpoint format:
// cell x of a row at bit (x & 7) of byte (x >> 3)).  The block starts at
// global column x0; with s = x0 & 7 its cells land at bits s.. of its first
// output byte, so output byte j holds block cells 8j - s .. 8j - s + 7 (those
// outside [0, w) are 0: the host ORs the bytes two blocks share).  One thread
// per output byte; 2-D grid, y strides rows.  Bit encoding: the pair(s)
// holding the byte's cells in natural order (nat64), then a funnel shift.
template <bool BIT>
__global__ void bits_kernel(const uint8_t *buf, const BlockView blk, int s, uint8_t *out, int64_t rb) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rb) return;
    const int64_t c0 = 8 * j - s;  // block cell of bit 0 of this byte (>= -7)
    const uint32_t lo = c0 < 0 ? (uint32_t)(-c0) : 0u;                     // bits below: none
    const uint32_t hi = w - c0 >= 8 ? 8u : (uint32_t)(w - c0);            // bits at and above: none
    const uint32_t keep = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    for (int64_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t *row = buf + (y + ya) * pitch + xoff;
        uint32_t v;
        if (BIT) {
            const uint32_t *wd = reinterpret_cast<const uint32_t *>(row);
            if (c0 < 0) {
                v = (uint32_t)pair_nat(wd, 0) << lo;
            } else {
                // the next pair is owned or x-apron / pitch padding: in-row
                const int64_t pp = c0 >> 6;
                const uint32_t sh = (uint32_t)(c0 & 63);
                uint64_t n = pair_nat(wd, pp) >> sh;
                if (sh > 56) n |= pair_nat(wd, pp + 1) << (64 - sh);
                v = (uint32_t)n;
            }
        } else {
            v = 0;
            for (uint32_t b = lo; b < hi; ++b) v |= (uint32_t)(row[c0 + b] & 1u) << b;
        }
        out[y * rb + j] = (uint8_t)(v & keep);
    }
}

// The inverse (life_dev_upload_bits): `in` holds, per owned row and at row
// pitch `ipitch` (a multiple of 16), the rb = bits_row_bytes packed bytes that
// cover the block, so block cell c sits at bit s + c of its row, s = x0 & 7.
// One thread per 16-byte unit of an owned row; 2-D grid, y strides rows.  Bit
// encoding: the unit's 128 cells are bits [s + 128u, s + 128u + 128) -- one
// aligned 16-B load plus the byte the shift pulls in (read only when it is
// one of the rb, i.e. when it can hold a cell below w), a funnel shift, then
// pair_of per 64 cells.  Byte encoding: 16 cells from 2-3 bytes, a nibble per
// dword.  Whole units are stored as in import_kernel: the cells at and beyond
// w become 0 and the caller's exchange fills the aprons.
__device__ __forceinline__ uint64_t low_mask64(int64_t n) {  // the n lowest bits, n clamped to 0..64
    return n <= 0 ? 0ull : n >= 64 ? ~0ull : (~0ull >> (64 - n));
}
template <bool BIT>
__global__ void unbits_kernel(const uint8_t *in, int64_t ipitch, int64_t rb, int s, uint8_t *buf,
                              const BlockView blk) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= units) return;
    const int64_t valid = w - u * (BIT ? 128 : 16);  // cells of this unit inside the block (>= 1)
    const int64_t xb = BIT ? 16 * u + 16 : 2 * u + 2;  // the byte after the unit's aligned ones
    const bool extra = s != 0 && xb < rb;
    for (int64_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t *row = in + y * ipitch;
        const uint32_t e = extra ? row[xb] : 0u;
        uint4 q;
        if (BIT) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + 16 * u);
            uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32), hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
            if (s) {
                lo = (lo >> s) | (hi << (64 - s));
                hi = (hi >> s) | ((uint64_t)e << (64 - s));
            }
            const uint2 p0 = pair_of(lo & low_mask64(valid)), p1 = pair_of(hi & low_mask64(valid - 64));
            q = make_uint4(p0.x, p0.y, p1.x, p1.y);
        } else {
            const uint32_t v = *reinterpret_cast<const uint16_t *>(row + 2 * u) | (e << 16);
            q = unpack_half((v >> s) & (uint32_t)low_mask64(valid < 16 ? valid : 16), 0);
        }
        *reinterpret_cast<uint4 *>(buf + (y + ya) * pitch + xoff + 16 * u) = q;
    }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <int CPU>
__global__ void fill_random_kernel(uint8_t *buf, const BlockView blk, int64_t nx, uint64_t key, uint32_t thr) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= units * h) return;
    const int64_t u = i % units, y = i / units;
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    const int64_t x0 = u * CPU;
    const uint64_t base = (uint64_t)((gy0 + y) * nx + gx0);
    for (int k = 0; k < CPU; ++k) {
        const int64_t x = x0 + k;
        if (x >= w) break;
        const uint32_t v = (uint32_t)(splitmix64(key ^ (base + (uint64_t)x)) >> 32) < thr;
        if (CPU == 16)
            word[k >> 2] |= v << (8 * (k & 3));
        else
            word[pair_dword(k)] |= v << pair_bit(k);
    }
    *reinterpret_cast<uint4 *>(buf + (y + ya) * pitch + xoff + 16 * u) =
        make_uint4(word[0], word[1], word[2], word[3]);
}

// Census of the owned cells: live count and the position-weighted checksum
// sum over live (x, y) of mix64(y*nx + x + 1), both mod 2^64 -- independent
// of the cell encoding and of the partition, so the 1-GPU and N-shard runs of
// one grid, and the byte and bit kernels, can be compared at sizes no host
// copy or CPU oracle reaches.  2-D grid: x over 16-B units, y strides rows.
__device__ __forceinline__ uint64_t cell_mix(uint64_t v) {
    v *= 0x9E3779B97F4A7C15ull;
    return v ^ (v >> 29);
}

template <int CPU>
__global__ void census_kernel(const uint8_t *buf, const BlockView blk, int64_t nx, unsigned long long *out) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long c = 0, sum = 0;
    constexpr int kPerWord = CPU / 4;  // cells per dword
    if (u < units) {
        const int64_t valid = w - u * CPU;  // cells of this unit inside the block
        uint32_t m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (CPU == 16) {
                const int64_t left = valid - k * kPerWord;
                m[k] = left <= 0 ? 0u : left >= kPerWord ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (32 - 8 * left));
            } else {  // dword k: cells 64 (k >> 1) + 2i + (k & 1), i < 32
                const int64_t n = (valid - 64 * (k >> 1) - (k & 1) + 1) >> 1;  // valid bits (floor; may be < 0)
                m[k] = n <= 0 ? 0u : n >= 32 ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (32 - n));
            }
        }
        for (int64_t y = blockIdx.y; y < h; y += gridDim.y) {
            const uint4 q = *reinterpret_cast<const uint4 *>(buf + (y + ya) * pitch + xoff + 16 * u);
            const uint32_t word[4] = {q.x, q.y, q.z, q.w};
            const uint64_t base = (uint64_t)((gy0 + y) * nx + gx0 + u * CPU) + 1u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t bits = word[k] & m[k];  // byte cells are 0/1: bit 8j = cell j of the dword
                c += __popc(bits);
                while (bits) {
                    const int b = __ffs(bits) - 1;
                    bits &= bits - 1u;
                    sum += cell_mix(base + (uint64_t)(CPU == 16 ? k * kPerWord + (b >> 3)
                                                                : 64 * (k >> 1) + 2 * b + (k & 1)));
                }
            }
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        c += __shfl_xor(c, s);
        sum += __shfl_xor(sum, s);
    }
    if ((threadIdx.x & 63) == 0) {
        if (c) atomicAdd(out, c);
        if (sum) atomicAdd(out + 1, sum);
    }
}

// Sparse edits (life_dev_set_cells): one thread per (x, y) pair of the staged
// list; coordinates wrap with a true modulo and only the cells of this block
// are written -- an atomic OR / AND on the owning dword of the pair layout
// (two listed cells may share a dword), a byte store for byte cells.  Aprons
// and the pad bits past w are not touched: the caller refills the halo.
__device__ __forceinline__ int64_t wrap_mod(int64_t v, int64_t n) {
    const int64_t r = v % n;
    return r < 0 ? r + n : r;
}
template <bool BIT>
__global__ void set_cells_kernel(uint8_t *buf, const BlockView blk, int64_t nx, int64_t ny, const int64_t *xy,
                                 int64_t n, int alive) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t x = wrap_mod(xy[2 * i], nx) - gx0, y = wrap_mod(xy[2 * i + 1], ny) - gy0;
    if (x < 0 || x >= w || y < 0 || y >= h) return;
    uint8_t *row = buf + (y + ya) * pitch + xoff;
    if (BIT) {
        uint32_t *wd = reinterpret_cast<uint32_t *>(row) + pair_dword(x);
        const uint32_t m = 1u << pair_bit(x);
        if (alive)
            atomicOr(wd, m);
        else
            atomicAnd(wd, ~m);
    } else {
        row[x] = alive ? 1 : 0;
    }
}

// A window piece (life_dev_gather_rect): block cells [lx0, lx0 + pw) x
// [ly0, ly0 + ph) as 0/1 bytes at out[j * opitch + i], read straight from the
// padded layout.  One thread per 8 output cells of a row; 2-D grid, y strides
// rows.  Bit encoding: the pair holding the first cell in natural order
// (nat64), funnel-shifted with the next pair when the 8 cells straddle it
// (that pair is read only then, and is owned: the cells are).
template <bool BIT>
__global__ void rect_kernel(const uint8_t *buf, const BlockView blk, int64_t lx0, int64_t ly0, int64_t pw,
                            int64_t ph, uint8_t *out, int64_t opitch) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t i0 = 8 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i0 >= pw) return;
    const int n = pw - i0 < 8 ? (int)(pw - i0) : 8;
    const int64_t x = lx0 + i0;
    for (int64_t j = blockIdx.y; j < ph; j += gridDim.y) {
        const uint8_t *row = buf + (ly0 + j + ya) * pitch + xoff;
        uint32_t c;  // cell k at bit k
        if (BIT) {
            const uint32_t *wd = reinterpret_cast<const uint32_t *>(row);
            const int64_t pp = x >> 6;
            const uint32_t sh = (uint32_t)(x & 63);
            uint64_t v = pair_nat(wd, pp) >> sh;
            if (sh + (uint32_t)n > 64u) v |= pair_nat(wd, pp + 1) << (64 - sh);
            c = (uint32_t)v;
        } else {
            c = 0;
            for (int k = 0; k < n; ++k) c |= (uint32_t)(row[x + k] & 1u) << k;
        }
        uint8_t *o = out + j * opitch + i0;
        for (int k = 0; k < n; ++k) o[k] = (uint8_t)((c >> k) & 1u);
    }
}

// The inverse (life_dev_set_rect): block cells [lx0, lx0 + pw) x [ly0, ly0 +
// ph) become in[j * ipitch + i] != 0; the aprons and every cell outside the
// piece stay as they are.  2-D grid, y strides rows.  Bit encoding: one thread
// per 64-cell pair the piece touches -- its bytes of that pair gathered into
// natural order, then a read-modify-write of the pair under the mask of the
// covered cells: one thread of a launch owns a dword, so no atomics; two
// pieces of one row that share a pair (w == nx, x0 % 64 != 0) are two launches
// in order on one stream.  Byte encoding: one thread per cell, a plain store.
template <bool BIT>
__global__ void paste_kernel(uint8_t *buf, const BlockView blk, int64_t lx0, int64_t ly0, int64_t pw, int64_t ph,
                             const uint8_t *in, int64_t ipitch) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!BIT) {
        if (t >= pw) return;
        for (int64_t j = blockIdx.y; j < ph; j += gridDim.y)
            buf[(ly0 + j + ya) * pitch + xoff + lx0 + t] = in[j * ipitch + t] != 0;
        return;
    }
    const int64_t p = (lx0 >> 6) + t;  // this thread's pair: cells [64p, 64p + 64)
    const int64_t a = p * 64 > lx0 ? p * 64 : lx0, b = p * 64 + 64 < lx0 + pw ? p * 64 + 64 : lx0 + pw;
    if (a >= b) return;  // past the piece's last pair
    const uint32_t sh = (uint32_t)(a - p * 64);
    const int n = (int)(b - a);
    const uint64_t mask = low_mask64(n) << sh;
    for (int64_t j = blockIdx.y; j < ph; j += gridDim.y) {
        const uint8_t *src = in + j * ipitch + (a - lx0);
        uint64_t v = 0;
        for (int k = 0; k < n; ++k) v |= (uint64_t)(src[k] != 0) << k;
        uint32_t *wd = reinterpret_cast<uint32_t *>(buf + (ly0 + j + ya) * pitch + xoff);
        put_pair(wd, p, (pair_nat(wd, p) & ~mask) | (v << sh));
    }
}

// Density map (life_dev_gather_density): map[by * bw + bx] += live owned cells
// with global x / fx == bx and y / fy == by.  Shaped like the census -- a lane
// per 16-byte unit column, one uint4 load per lane and row -- but block y
// walks `rpb` CONSECUTIVE rows, so a lane counts down the rows of one bin row
// in registers.  The lane splits its unit over the bins it touches with
// masks built once: bin cells [c0, c1) of the unit keep, in dword k, the bits
// below_k(c1) & ~below_k(c0), below_k(c) = the dword's cells under c -- for
// the interleaved pairs (c + 1) >> 1 bits of an even dword and c >> 1 of an
// odd one (c counted from the pair's first cell), for byte cells 8 bits per
// cell; cells past w fall outside every [c0, c1).  Bins are taken two at a
// time (a unit of fx >= CPU cells touches at most two: one pass over the
// rows; smaller factors re-read the rows once per further bin pair, from
// cache), and each (unit, bin, bin row) ends in ONE atomicAdd.  A wave whose
// lanes all lie in one bin adds up across the wave first and lane 0 issues
// the atomic.  Lanes past the last unit of a partly filled wave shadow lane
// 0's column with empty masks, so the wave stays convergent.
__device__ __forceinline__ uint32_t low_mask(int64_t n) {  // the n lowest bits, n clamped to 0..32
    return n <= 0 ? 0u : n >= 32 ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (32 - n));
}
template <int CPU>
__device__ __forceinline__ uint32_t cells_below(int k, int64_t c) {  // dword k's bits of unit cells [0, c)
    if (CPU == 16) return low_mask(8 * (c - 4 * k)) & 0x01010101u;
    return low_mask((c - 64 * (k >> 1) - (k & 1) + 1) >> 1);
}
template <int CPU>
__global__ __launch_bounds__(256) void density_kernel(const uint8_t *buf, const BlockView blk, int64_t fx, int64_t fy,
                                                      int64_t bw, int64_t rpb, uint32_t *map) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t u0 = u - (threadIdx.x & 63);  // the wave's first unit
    if (u0 >= units) return;                    // a whole wave past the row
    const bool live = u < units;
    const int64_t uu = live ? u : u0;
    const int64_t left = w - uu * CPU;
    const int64_t valid = !live ? 0 : left < CPU ? left : CPU;  // cells of this unit inside the block
    const int64_t gxu = gx0 + uu * CPU;
    const int64_t bfirst = gxu / fx, blast = live ? (gxu + valid - 1) / fx : bfirst;
    const bool one = __all(blast == bfirst && bfirst == __shfl(bfirst, 0)) != 0;  // the wave shares one bin
    const int64_t r0 = (int64_t)blockIdx.y * rpb, r1 = r0 + rpb < h ? r0 + rpb : h;
    const uint8_t *col = buf + ya * pitch + xoff + 16 * uu;
    for (int64_t b = bfirst; b <= blast; b += 2) {
        uint32_t ma[4], mb[4];
        {
            const int64_t e0 = b * fx - gxu, e1 = e0 + fx, e2 = e1 + fx;  // bin edges, in unit cells
            const int64_t c0 = e0 < 0 ? 0 : e0 > valid ? valid : e0, c1 = e1 < 0 ? 0 : e1 > valid ? valid : e1;
            const int64_t c2 = e2 < 0 ? 0 : e2 > valid ? valid : e2;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t l0 = cells_below<CPU>(k, c0), l1 = cells_below<CPU>(k, c1);
                ma[k] = l1 & ~l0;
                mb[k] = cells_below<CPU>(k, c2) & ~l1;
            }
        }
        for (int64_t y = r0; y < r1;) {
            const int64_t by = (gy0 + y) / fy;
            const int64_t lim = (by + 1) * fy - gy0, ye = lim < r1 ? lim : r1;  // rows [y, ye) share bin row by
            uint32_t ca = 0, cb = 0;
#pragma unroll 4
            for (; y < ye; ++y) {
                const uint4 q = *reinterpret_cast<const uint4 *>(col + y * pitch);
                ca += __popc(q.x & ma[0]) + __popc(q.y & ma[1]) + __popc(q.z & ma[2]) + __popc(q.w & ma[3]);
                cb += __popc(q.x & mb[0]) + __popc(q.y & mb[1]) + __popc(q.z & mb[2]) + __popc(q.w & mb[3]);
            }
            uint32_t *o = map + by * bw + b;
            if (one) {  // cb == 0: the unit ends inside bin b
                for (int s = 32; s > 0; s >>= 1) ca += __shfl_xor(ca, s);
                if ((threadIdx.x & 63) == 0 && ca) atomicAdd(o, ca);
            } else {
                if (ca) atomicAdd(o, ca);
                if (cb) atomicAdd(o + 1, cb);
            }
        }
    }
}

// Activity map of a bit buffer (LIFE_OPT_SKIP_DEAD, life_act.h): bit y % 32 of
// the masks of map cell (y / 32, c) is set when owned row y holds a live cell
// in pairs [62 c, 62 c + 62) / in the first / in the last of them; the map
// arrives zeroed.  Shaped like the census: one streaming pass over the owned
// cells only (w a multiple of 64: whole pairs), a lane per pair and an 8-B
// load per row.  A workgroup per map cell, its four waves 8 rows each, one
// ballot per row; a wave ORs in the masks of its rows.
__global__ __launch_bounds__(256) void act_scan_kernel(const uint8_t *buf, const BlockView blk, uint32_t *map,
                                                       int64_t ncol) {
    const auto [pitch, ya, xoff, w, h, units, gx0, gy0] = blk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = blockIdx.x, c = blockIdx.y, W = w / 64;
    const int64_t j = c * kActPairs + lane;
    const bool on = lane < kActPairs && j < W;
    const int llast = (int)(W - c * kActPairs < kActPairs ? W - c * kActPairs : kActPairs) - 1;
    uint32_t m[kActWords] = {};
    for (int k = 0; k < 8; ++k) {
        const int64_t y = r * kActRows + 8 * wave + k;
        if (y >= h) break;  // uniform
        const uint64_t v = on ? *reinterpret_cast<const uint64_t *>(buf + (y + ya) * pitch + xoff + 8 * j) : 0ull;
        const unsigned long long nz = __ballot(v != 0ull);
        const uint32_t bit = 1u << (8 * wave + k);
        if (nz) m[kActAny] |= bit;
        if (nz & 1ull) m[kActFirst] |= bit;
        if ((nz >> llast) & 1ull) m[kActLast] |= bit;
    }
    if (lane == 0)
        for (int k = 0; k < kActWords; ++k)
            if (m[k]) atomicOr(map + act_word(r, c, ncol, k), m[k]);
}

// Copy ceiling: one 16-B load + store per lane, one wave-instruction each,
// a workgroup per 4 KiB.  Measured against grid-stride, unrolled and
// nontemporal variants (scripts/ubench_copy.hip, profiles/r01/ubench_copy.txt):
// this shape is the fastest, 6.30 TB/s on 2 GiB.
__global__ __launch_bounds__(256) void copy_kernel(const uint4 *__restrict__ in, uint4 *__restrict__ out,
                                                   int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i];
}

inline bool is_bit(const life_layout &L) { return L.kernel == LIFE_KERNEL_BIT; }
inline unsigned blocks_for(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// One launch (256 lanes per workgroup) of the block's encoding: `bit` for the
// bit layout, else `byte`, two instances of one kernel template with the same
// parameter list P, so a launcher writes its arguments once.
template <class... P, class... A>
hipError_t launch_enc(const life_layout &L, void (*bit)(P...), void (*byte)(P...), dim3 grid, hipStream_t s, A... a) {
    (is_bit(L) ? bit : byte)<<<grid, 256, 0, s>>>(a...);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pack_columns(const life_layout &L, const uint8_t *buf, uint8_t *stage, hipStream_t s,
                               bool corners) {
    if (corners && L.xapron < 32) return hipErrorInvalidValue;
    const int64_t nc = corners ? 4 * L.yapron : 0;
    pack_columns_kernel<<<blocks_for(L.h + nc, 256), 256, 0, s>>>(buf, view(L), L.xapron, stage, is_bit(L), nc);
    return hipGetLastError();
}

hipError_t launch_wrap_columns(const life_layout &L, uint8_t *buf, hipStream_t s) {
    if (L.xapron < 32 || L.w < L.xapron) return hipErrorInvalidValue;
    wrap_columns_kernel<<<blocks_for(L.h, 256), 256, 0, s>>>(buf, view(L), is_bit(L));
    return hipGetLastError();
}

hipError_t launch_unpack_columns(const life_layout &L, uint8_t *buf, const uint8_t *stage, hipStream_t s,
                                 bool corners) {
    if (corners && L.xapron < 32) return hipErrorInvalidValue;
    const int64_t nc = corners ? 4 * L.yapron : 0;
    unpack_columns_kernel<<<blocks_for(L.h + nc, 256), 256, 0, s>>>(buf, view(L), L.xapron, stage, is_bit(L), nc);
    return hipGetLastError();
}

hipError_t launch_import_block(const life_layout &L, const uint8_t *dense, uint8_t *buf, hipStream_t s) {
    return launch_enc(L, import_kernel<128>, import_kernel<16>, blocks_for(L.units * L.h, 256), s, dense, buf,
                      view(L));
}

hipError_t launch_export_block(const life_layout &L, const uint8_t *buf, uint8_t *dense, hipStream_t s) {
    return launch_enc(L, export_kernel<128>, export_kernel<16>, blocks_for(L.units * L.h, 256), s, buf, dense,
                      view(L));
}

hipError_t launch_fill_random(const life_layout &L, int64_t nx, uint64_t key, uint32_t thr32, uint8_t *buf,
                              hipStream_t s) {
    return launch_enc(L, fill_random_kernel<128>, fill_random_kernel<16>, blocks_for(L.units * L.h, 256), s, buf,
                      view(L), nx, key, thr32);
}

hipError_t launch_vtk_block(const life_layout &L, const uint8_t *buf, uint8_t *out, hipStream_t s) {
    const dim3 grid(blocks_for((L.w + 7) / 8, 256), (unsigned)(L.h < 8192 ? L.h : 8192));
    return launch_enc(L, vtk_kernel<true>, vtk_kernel<false>, grid, s, buf, view(L), out);
}

hipError_t launch_bits_block(const life_layout &L, const uint8_t *buf, uint8_t *out, hipStream_t s) {
    const int sh = (int)(L.x0 & 7);
    const int64_t rb = bits_row_bytes(L);
    const dim3 grid(blocks_for(rb, 256), (unsigned)(L.h < 8192 ? L.h : 8192));
    return launch_enc(L, bits_kernel<true>, bits_kernel<false>, grid, s, buf, view(L), sh, out, rb);
}

hipError_t launch_unbits_block(const life_layout &L, const uint8_t *in, uint8_t *buf, hipStream_t s) {
    const int sh = (int)(L.x0 & 7);
    const dim3 grid(blocks_for(L.units, 256), (unsigned)(L.h < 8192 ? L.h : 8192));
    return launch_enc(L, unbits_kernel<true>, unbits_kernel<false>, grid, s, in, unbits_pitch(L), bits_row_bytes(L), sh,
                      buf, view(L));
}

hipError_t launch_copy(const void *in, void *out, int64_t bytes, hipStream_t s) {
    const int64_t n = bytes / 16;
    copy_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(reinterpret_cast<const uint4 *>(in),
                                                            reinterpret_cast<uint4 *>(out), n);
    return hipGetLastError();
}

hipError_t launch_census(const life_layout &L, int64_t nx, const uint8_t *buf, unsigned long long *out,
                         hipStream_t s) {
    const dim3 grid(blocks_for(L.units, 256), (unsigned)(L.h < 4096 ? L.h : 4096));
    return launch_enc(L, census_kernel<128>, census_kernel<16>, grid, s, buf, view(L), nx, out);
}

hipError_t launch_set_cells(const life_layout &L, int64_t nx, int64_t ny, const int64_t *xy, int64_t n, int alive,
                            uint8_t *buf, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    return launch_enc(L, set_cells_kernel<true>, set_cells_kernel<false>, blocks_for(n, 256), s, buf, view(L), nx, ny,
                      xy, n, alive);
}

hipError_t launch_rect_piece(const life_layout &L, const uint8_t *buf, int64_t lx0, int64_t ly0, int64_t pw,
                             int64_t ph, uint8_t *out, int64_t opitch, hipStream_t s) {
    if (lx0 < 0 || ly0 < 0 || pw < 1 || ph < 1 || lx0 + pw > L.w || ly0 + ph > L.h) return hipErrorInvalidValue;
    const dim3 grid(blocks_for((pw + 7) / 8, 256), (unsigned)(ph < 8192 ? ph : 8192));
    return launch_enc(L, rect_kernel<true>, rect_kernel<false>, grid, s, buf, view(L), lx0, ly0, pw, ph, out, opitch);
}

hipError_t launch_paste_piece(const life_layout &L, uint8_t *buf, int64_t lx0, int64_t ly0, int64_t pw, int64_t ph,
                              const uint8_t *in, int64_t ipitch, hipStream_t s) {
    if (lx0 < 0 || ly0 < 0 || pw < 1 || ph < 1 || lx0 + pw > L.w || ly0 + ph > L.h) return hipErrorInvalidValue;
    const int64_t lanes = is_bit(L) ? ((lx0 + pw - 1) >> 6) - (lx0 >> 6) + 1 : pw;  // pairs touched / cells
    const dim3 grid(blocks_for(lanes, 256), (unsigned)(ph < 8192 ? ph : 8192));
    return launch_enc(L, paste_kernel<true>, paste_kernel<false>, grid, s, buf, view(L), lx0, ly0, pw, ph, in, ipitch);
}

hipError_t launch_act_scan(const life_layout &L, const uint8_t *buf, uint32_t *map, hipStream_t s) {
    if (!is_bit(L) || L.w % 64 != 0) return hipErrorInvalidValue;
    const int64_t ncol = act_cols(L.w / 64), nrow = act_rows(L.h);
    if (ncol > 65535 || nrow > 0x7fffffff) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(map, 0, (size_t)(ncol * nrow * kActWords) * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    act_scan_kernel<<<dim3((unsigned)nrow, (unsigned)ncol), 256, 0, s>>>(buf, view(L), map, ncol);
    return hipGetLastError();
}

hipError_t launch_density(const life_layout &L, const uint8_t *buf, int64_t fx, int64_t fy, int64_t bw,
                          uint32_t *map, hipStream_t s) {
    if (fx < 1 || fy < 1 || bw < 1) return hipErrorInvalidValue;
    // rows per block: about two lanes per hardware thread slot of the chip
    // (256 CUs x 2048), at most 65535 blocks in y
    const int64_t bx = blocks_for(L.units, 256);
    int64_t chunks = (int64_t)(2 * 256 * 2048) / (bx * 256);
    chunks = chunks < 1 ? 1 : chunks > L.h ? L.h : chunks;
    if (chunks > 65535) chunks = 65535;
    const int64_t rpb = (L.h + chunks - 1) / chunks;
    const dim3 grid((unsigned)bx, (unsigned)((L.h + rpb - 1) / rpb));
    return launch_enc(L, density_kernel<128>, density_kernel<16>, grid, s, buf, view(L), fx, fy, bw, rpb, map);
}

}  // namespace life
