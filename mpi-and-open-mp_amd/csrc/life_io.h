// life_io.h -- host-side launchers of the data-movement kernels (life_io.hip):
// halo column staging, dense import / export, the VTK and LIFEBITS formatters,
// the random fill, the census, the sparse-I/O kernels and the copy probe.
//
// All launchers are asynchronous on `s` and return the hipError_t of the
// launch.  Buffers are the padded shard layout of life_layout (see
// include/life_mi355x.h and DESIGN.md "Data layout in HBM").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "life_mi355x.h"

namespace life {

// Column halo staging: pack writes the last xapron columns to slot 0 and the
// first xapron columns to slot 1 (h rows each: 1 byte 0/1 per row for a cell
// column, one 8-B pair per row for a bit-encoded 64-cell column, 32 bytes per
// row for a byte-encoded 32-cell column); unpack writes slot 0 into x in
// [-xapron, 0) and slot 1 into [w, w + xapron).
inline int64_t column_bytes_per_row(const life_layout &L) {
    if (L.xapron == 1) return 1;
    return L.kernel == LIFE_KERNEL_BIT ? 8 : 32;
}
// corners (the fused one-phase plan, life_halo_plan): also the four K x
// xapron corner blocks behind the two columns, K = yapron rows each.  Send
// slots 2h + cK + r, c in the plan's direction order SE, SW, NE, NW: my
// bottom-right, bottom-left, top-right, top-left K rows; receive slots in the
// same order: my top-left, top-right, bottom-left, bottom-right apron corner.
hipError_t launch_pack_columns(const life_layout &L, const uint8_t *buf, uint8_t *stage,
                               hipStream_t s, bool corners = false);
hipError_t launch_unpack_columns(const life_layout &L, uint8_t *buf, const uint8_t *stage,
                                 hipStream_t s, bool corners = false);
// staging bytes of one direction (send or receive) of a shard's exchange
inline int64_t column_stage_bytes(const life_layout &L) {
    return (2 * L.h + (L.xapron > 1 ? 4 * L.yapron : 0)) * column_bytes_per_row(L);
}
// Temporal layouts: a periodic x axis inside one shard is wrapped by the
// stencil (whole lane columns) when w is a multiple of the x-apron (64 bit
// cells, 32 byte cells); otherwise the shard fills its own aprons from its own
// columns (launch_wrap_columns, needs w >= xapron).
inline bool self_wrap_x(const life_layout &L, int dims0) {
    return L.xapron > 1 && dims0 == 1 && L.w % L.xapron != 0;
}
hipError_t launch_wrap_columns(const life_layout &L, uint8_t *buf, hipStream_t s);

// Dense w*h byte block (row pitch w) <-> padded encoded buffer.
hipError_t launch_import_block(const life_layout &L, const uint8_t *dense, uint8_t *buf,
                               hipStream_t s);
hipError_t launch_export_block(const life_layout &L, const uint8_t *buf, uint8_t *dense,
                               hipStream_t s);

// The block's VTK cell data: '0'/'1' + '\n' per owned cell, rows of 2w bytes.
hipError_t launch_vtk_block(const life_layout &L, const uint8_t *buf, uint8_t *out, hipStream_t s);
// Packed rows (LIFEBITS: bit x & 7 of byte x >> 3) of a block starting at
// global column x0: bits_row_bytes(L) bytes per row, the block's cells from
// bit x0 & 7 of its first byte on.
inline int64_t bits_row_bytes(const life_layout &L) { return ((L.x0 & 7) + L.w + 7) / 8; }
hipError_t launch_bits_block(const life_layout &L, const uint8_t *buf, uint8_t *out, hipStream_t s);
// The way back: `in` holds the same bits_row_bytes(L) bytes per owned row at
// row pitch unbits_pitch(L) (16-B aligned loads; the bytes between the two
// need not be set).  Writes every 16-B unit of the owned rows, cells at and
// beyond w as 0; the aprons are the caller's to refill.
inline int64_t unbits_pitch(const life_layout &L) { return (bits_row_bytes(L) + 15) / 16 * 16; }
hipError_t launch_unbits_block(const life_layout &L, const uint8_t *in, uint8_t *buf, hipStream_t s);

// Counter-based synthetic init of the owned cells (global indices).
hipError_t launch_fill_random(const life_layout &L, int64_t nx, uint64_t key, uint32_t thr32,
                              uint8_t *buf, hipStream_t s);

// Adds the live owned cells' count to out[0] and their checksum
// (sum of mix64(global y*nx + x + 1), mod 2^64) to out[1].
hipError_t launch_census(const life_layout &L, int64_t nx, const uint8_t *buf, unsigned long long *out,
                         hipStream_t s);

// Sparse edits: the n (x, y) pairs of `xy` (device memory, global
// coordinates, wrapped with a true modulo) that fall in the block become
// alive or dead; other cells, the aprons and the pad bits stay as they are.
hipError_t launch_set_cells(const life_layout &L, int64_t nx, int64_t ny, const int64_t *xy, int64_t n, int alive,
                            uint8_t *buf, hipStream_t s);
// Block cells [lx0, lx0 + pw) x [ly0, ly0 + ph) (owned) as 0/1 bytes at
// out[j * opitch + i].
hipError_t launch_rect_piece(const life_layout &L, const uint8_t *buf, int64_t lx0, int64_t ly0, int64_t pw,
                             int64_t ph, uint8_t *out, int64_t opitch, hipStream_t s);
// The way back: block cells [lx0, lx0 + pw) x [ly0, ly0 + ph) (owned) become
// in[j * ipitch + i] != 0; nothing else is written.  Pieces that share a
// 64-cell pair of a row must be launched in order on one stream.
hipError_t launch_paste_piece(const life_layout &L, uint8_t *buf, int64_t lx0, int64_t ly0, int64_t pw, int64_t ph,
                              const uint8_t *in, int64_t ipitch, hipStream_t s);
// Adds the block's live cells to the density map: map[(y / fy) * bw + x / fx]
// over global (x, y); bw = bins per map row.
hipError_t launch_density(const life_layout &L, const uint8_t *buf, int64_t fx, int64_t fy, int64_t bw,
                          uint32_t *map, hipStream_t s);

// The activity map of a bit block whose width is a multiple of 64 (life_act.h;
// LIFE_OPT_SKIP_DEAD): zeroes `map` (act_cols x act_rows cells of kActWords
// row masks) and sets the bits of every owned row that holds a live cell.
hipError_t launch_act_scan(const life_layout &L, const uint8_t *buf, uint32_t *map, hipStream_t s);

// Copy-ceiling probe: out[0, bytes) = in[0, bytes), bytes a multiple of 16.
hipError_t launch_copy(const void *in, void *out, int64_t bytes, hipStream_t s);

}  // namespace life
