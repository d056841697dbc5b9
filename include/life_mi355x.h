/*
 * life_mi355x.h -- C ABI of the MI355X-native Game-of-Life hot path.
 *
 * Drop-in boundary for the reference kekoveca/MPI-and-Open-MP.  The reference
 * has no library or FFI: its "operator interface" is the set of free functions
 * on `life_t` in 6-cartesian/life_cart.c:39-49, called only from main()
 * (life_cart.c:51-85).  Each entry point below names the reference function
 * it replaces.  Plain pointers and sizes only; no torch or HIP types.
 *
 * Grid convention (same as the reference's ind(), life_cart.c:11): cells are
 * 0/1, row-major, x fastest: cell (x, y) at grid[y*nx + x].  Indices are
 * 64-bit (the reference overflows int beyond ~46340^2, life_cart.c:101).
 *
 * Errors: every int-returning call returns LIFE_OK (0) or a negative
 * LIFE_E* code (the reference asserts or aborts via MPI_ERRORS_ARE_FATAL);
 * life_strerror() names it.  Not thread-safe: one host thread owns a handle.
 */
#ifndef LIFE_MI355X_H
#define LIFE_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIFE_OK 0
#define LIFE_EINVAL (-1)   /* bad argument (sizes, dims, empty block, ...) */
#define LIFE_EHIP (-2)     /* HIP runtime error (message: life_last_error()) */
#define LIFE_ERCCL (-3)    /* RCCL error */
#define LIFE_ENOMEM (-4)   /* host or device allocation failed */
#define LIFE_ESTATE (-5)   /* call not valid in this state */
#define LIFE_EIO (-6)      /* file I/O or parse error (driver helpers) */

/* Cell encoding / kernel family. */
#define LIFE_KERNEL_BYTE 0 /* 1 byte per cell, SWAR byte stencil */
#define LIFE_KERNEL_BIT 1  /* 1 bit per cell (32 cells/word), bit-sliced adder */

/* Halo transport between shards. */
#define LIFE_XPORT_AUTO 0  /* RCCL across processes/devices, LOCAL otherwise */
#define LIFE_XPORT_RCCL 1  /* ncclSend/ncclRecv (xGMI) */
#define LIFE_XPORT_LOCAL 2 /* device-to-device copies inside one process */

typedef struct life_dev life_dev; /* opaque: device memory, streams, RCCL comms */

/* ---------------------------------------------------------------- host only */

/* decomposition(): block k of n cells over p parts, the last block takes the
 * remainder.  Replaces life_cart.c:217-223 (and 5-gather/life_mpi.c:170-175). */
void life_decomposition(int64_t n, int p, int k, int64_t *start, int64_t *stop);

/* MPI_Dims_create(n, 2, {0,0}) as called in life_init (life_cart.c:117-118):
 * dims[0] >= dims[1], as balanced as possible. 2->{2,1}, 4->{2,2}, 8->{4,2}. */
void life_dims_create(int n, int dims[2]);

/* Partition shape for n shards of an nx x ny grid (the 1-D
 * row strips of 3-life/4-life/5-gather vs the 2-D blocks of 6-cartesian).
 * CART: life_dims_create (life_cart.c:117-118).  ROWS: {1, n}, horizontal
 * strips (5-gather/life_mpi.c:96-99 cuts y the same way): every halo message is
 * a run of whole padded rows, sent straight from the buffer with no pack
 * kernel.  COLS: {n, 1}.  AUTO: ROWS when every strip is at least
 * LIFE_AUTO_MIN_STRIP_ROWS tall, else CART -- measured
 * on MI355X with the LOCAL transport at 65536^2 per shard (DESIGN.md §6,
 * profiles/r01/partition_sweep.jsonl), row strips cost the owning GPU 0-6 %
 * less per generation than 2-D blocks with either encoding.  Returns
 * LIFE_EINVAL for n < 1, an unknown policy or a shape with empty blocks. */
#define LIFE_PARTITION_CART 0
#define LIFE_PARTITION_ROWS 1
#define LIFE_PARTITION_COLS 2
#define LIFE_PARTITION_AUTO 3
#define LIFE_AUTO_MIN_STRIP_ROWS 1024
int life_dims_choose(int64_t nx, int64_t ny, int n, int policy, int dims[2]);

/* One halo-exchange operation of a shard (replaces exchange_columns /
 * exchange_rows / exchange_corners, life_cart.c:225-279, and the 1-D ring
 * exchange of 5-gather/life_mpi.c:181-191).  Coordinates are the shard's
 * LOCAL frame: owned cells x in [0,w), y in [0,h); padded row of owned row y
 * is y + yapron; the apron is x in [-xapron, 0) u [w, w+xapron) and rows
 * y in [-yapron, 0) u [h, h+yapron) (see life_layout). */
#define LIFE_HALO_SEND 0
#define LIFE_HALO_RECV 1
#define LIFE_HALO_FILL 2   /* axis not partitioned (dims[d] == 1): wrapped inside the shard */
#define LIFE_HALO_COLUMN 0 /* cells x in [index, index+width) of padded rows [first, first+count) */
#define LIFE_HALO_ROW 1    /* padded rows [index, index+width), cells x in [first, first+count) */
#define LIFE_HALO_CORNER 2 /* as a column op: cells x in [index, index+width) of padded rows [first, first+count) */
typedef struct {
    int32_t phase; /* 0: x (columns) first, then 1: y (rows incl. corners); both axes
                      exchanged with temporal aprons: all in phase 0, corners explicit */
    int32_t kind;  /* LIFE_HALO_SEND / RECV / FILL */
    int32_t peer;  /* global shard rank, -1 for FILL */
    int32_t what;  /* LIFE_HALO_COLUMN / LIFE_HALO_ROW / LIFE_HALO_CORNER */
    int64_t index; /* first column x, or first padded row */
    int64_t first; /* first padded row (column op) or first cell x (row op) */
    int64_t count; /* rows (column op) or cells (row op) */
    int64_t width; /* columns (column op) or rows (row op) */
} life_halo_op;

/* Builds the per-exchange halo plan of shard `rank` of a dims[0] x dims[1]
 * periodic Cartesian partition (rank = c0*dims[1] + c1, dim 0 splits x, as
 * MPI_Cart_create(reorder=0) at life_cart.c:119-121) for cell encoding
 * `kernel` (apron widths from life_layout_query).  Writes up to max_ops ops
 * in execution order and returns their number (or LIFE_EINVAL).  Sends to
 * and receives from one peer are matched in issue order. */
int life_halo_plan(int64_t nx, int64_t ny, int dims0, int dims1, int rank, int kernel,
                   life_halo_op *ops, int max_ops);

/* Padded layout of a shard as allocated on the device: rows = h + 2*yapron
 * padded rows of `pitch` bytes; owned cell (x, y) lives in padded row
 * y + yapron at cell offset x from byte `xoff`.  Byte encoding: byte x.  Bit
 * encoding: 64-cell pairs of little-endian dwords, bit-interleaved -- cell x
 * is bit ((x & 63) >> 1) of dword 2*(x >> 6) + (x & 1) (floor division,
 * counted from xoff): the even cells of a pair in its first dword, the odd
 * cells in its second (the stencil's horizontal neighbours then need one
 * funnel shift per dword).  `generations_per_exchange` is how
 * many generations one halo exchange feeds: 1 for the one-cell apron; for
 * the temporally blocked stencil (x-apron of one lane column: 64 cells for
 * bits, 32 for bytes; K-row y-apron; blocks at least that wide) K =
 * LIFE_TEMPORAL_DEPTH (bit) or LIFE_TEMPORAL_DEPTH_BYTE (byte), or
 * 8/12/16/24/32 from the environment variables of the same names. */
#define LIFE_TEMPORAL_DEPTH 32
#define LIFE_TEMPORAL_DEPTH_BYTE 32
typedef struct {
    int64_t w, h;      /* owned block */
    int64_t x0, y0;    /* global origin of the block */
    int64_t pitch;     /* bytes per padded row */
    int64_t xoff;      /* byte offset of owned cell x = 0 in a padded row */
    int64_t rows;      /* h + 2*yapron */
    int64_t units;     /* 16-byte lanes per row the one-generation stencil walks */
    int64_t xapron;    /* apron width in cells (x) */
    int64_t yapron;    /* apron depth in rows (y) */
    int32_t kernel;    /* LIFE_KERNEL_* */
    int32_t coords[2]; /* Cartesian coordinates of the shard */
    int32_t generations_per_exchange;
    int32_t reserved;
} life_layout;

int life_layout_query(int64_t nx, int64_t ny, int dims0, int dims1, int rank, int kernel,
                      life_layout *out);

/* Life-like (outer-totalistic) rules.  A rule is two 9-bit masks: `birth`
 * bit k set = a dead cell with k live neighbours (of 8) is born, `survive`
 * bit k set = a live cell with k live neighbours stays alive; every other cell
 * is dead in the next generation.  Conway's B3/S23 (life_cart.c:202-208) is
 * birth = 1 << 3, survive = (1 << 2) | (1 << 3).  life_rule_parse accepts
 * "B36/S23" in either letter case and Golly's "23/3" (S/B): digits 0-8 in any
 * order, repeats harmless, empty lists allowed ("B2/S"); anything else is
 * LIFE_EINVAL with a life_last_error() message that quotes the text.
 * life_rule_format writes the canonical "B.../S..." with ascending digits
 * (LIFE_EINVAL for bits above 8).  Neither needs a GPU. */
#define LIFE_RULE_CONWAY_BIRTH 0x008u
#define LIFE_RULE_CONWAY_SURVIVE 0x00Cu
int life_rule_parse(const char *text, uint32_t *birth, uint32_t *survive);
int life_rule_format(uint32_t birth, uint32_t survive, char out[24]);

/* Generations rules (the batch's wave tier runs them:
 * life_batch_set_rule_gen).  A cell state is s in [0, states), 2 <= states <=
 * LIFE_GEN_MAX_STATES: 0 dead, 1 alive, 2 .. states - 1 dying.  With n the
 * number of the 8 neighbours whose state is exactly 1: s = 0 becomes 1 if
 * `birth` bit n is set, else stays 0; s = 1 stays 1 if `survive` bit n is set,
 * else becomes 2 mod states; s >= 2 becomes (s + 1) mod states.  states = 2 is
 * the Life-like rule of the two masks.  life_rule_parse_gen accepts everything
 * life_rule_parse accepts (states = 2), "B2/S345/C4" with G accepted for C in
 * either letter case, and Golly's "345/2/4" (S/B/C); the state count is one or
 * two decimal digits without a leading zero.  States outside 2 .. 16, an empty
 * third part, a fourth part or trailing junk are LIFE_EINVAL with a
 * life_last_error() message that quotes the text.  life_rule_format_gen writes
 * the canonical "B.../S.../Cn", and for states = 2 exactly what
 * life_rule_format writes (LIFE_EINVAL for bits above 8 or states outside 2 ..
 * 16).  Neither needs a GPU. */
#define LIFE_GEN_MAX_STATES 16
int life_rule_parse_gen(const char *text, uint32_t *birth, uint32_t *survive, uint32_t *states);
int life_rule_format_gen(uint32_t birth, uint32_t survive, uint32_t states, char out[32]);

const char *life_strerror(int err);
const char *life_dev_strerror(int err); /* the same (SURVEY 8(b)'s name for it) */
const char *life_last_error(void); /* detail of the last LIFE_EHIP/ERCCL on this thread */

/* ---------------------------------------------------------------- device */

/* life_init (life_cart.c:92-144) minus the file parsing: sizes the global
 * nx x ny periodic grid, splits it over `nshards` shards driven by THIS
 * process (dims = life_dims_create(nshards)), one per visible device
 * (shard i on device i % device_count), and allocates double-buffered padded
 * blocks.  Transport AUTO: RCCL when every shard has its own device, LOCAL
 * device copies otherwise (e.g. several logical shards on one GPU). */
int life_dev_create(int64_t nx, int64_t ny, int nshards, int kernel, life_dev **out);

/* Same with every knob: dims (0,0 = dims_create), transport.  LIFE_XPORT_RCCL
 * needs one device per shard and builds one communicator rank per shard with
 * ncclCommInitAll -- a single shard included (a one-device communicator, so
 * LIFE_OPT_LOOPBACK exercises this single-process RCCL path on one GPU). */
int life_dev_create_ex(int64_t nx, int64_t ny, int nshards, int dims0, int dims1, int kernel,
                       int transport, life_dev **out);

/* One-process-per-GPU mode (torchrun / mpirun style): this process owns the
 * single shard `rank` of `world` on `device`; `unique_id` (128 bytes) comes
 * from life_get_unique_id() on rank 0, broadcast by the caller (required when
 * world > 1; with world == 1 it is optional and, if given, still builds a
 * one-rank RCCL communicator, used by the census all-reduce). */
int life_get_unique_id(uint8_t unique_id[128]);
int life_dev_create_rank(int64_t nx, int64_t ny, int kernel, int rank, int world, int dims0,
                         int dims1, const uint8_t unique_id[128], int device, life_dev **out);

/* The loaded cells of life_init (life_cart.c:104-109): `grid` is the full
 * nx*ny host grid (nonzero = alive); each local shard takes its block.  Then
 * fills the halos.  In rank mode every rank passes the full grid. */
int life_dev_upload(life_dev *d, const uint8_t *grid);

/* Device-side synthetic init (no host grid): cell(x,y) =
 * (splitmix64(splitmix64(seed) ^ (y*nx+x)) >> 32) < thr32,
 * splitmix64 the standard finaliser.  thr32 = density * 2^32. */
int life_dev_fill_random(life_dev *d, uint64_t seed, uint32_t thr32);

/* `generations` x (life_exchange + life_step): life_cart.c:73-74
 * (replaces life_exchange :275-279 and life_step :189-215). Asynchronous.
 * With a temporally blocked layout, up to generations_per_exchange
 * generations run per launch and the halo is exchanged once per launch. */
int life_dev_step(life_dev *d, int64_t generations);

/* life_collect (life_cart.c:281-305; MPI_Gather in 5-gather/life_mpi.c:177-179):
 * device-side gather of every block to the root shard (global rank
 * world-1, as the reference) and one copy into `grid` (nx*ny bytes, 0/1).
 * In rank mode only the root writes `grid` (others may pass NULL). Blocking. */
int life_dev_gather(life_dev *d, uint8_t *grid);

/* The same collect, formatted on the device as the cell-data body of
 * life_save_vtk (life_cart.c:181-185): "%d\n" per cell, y outer, x inner --
 * 2*nx*ny bytes of '0'/'1' and '\n' written to `body` (root only in rank
 * mode).  The caller writes the 10 header lines in front (driver/life.c). */
int life_dev_gather_vtk(life_dev *d, char *body);

/* The same collect as packed rows: ny rows of ceil(nx/8) bytes, cell x at
 * bit (x & 7) of byte (x >> 3) -- the body of the driver's LIFEBITS
 * checkpoint frame (driver/life.c save_bits), 1/16 of the VTK text and 1/8
 * of the dense grid over PCIe (root only in rank mode).  Blocking. */
int life_dev_gather_bits(life_dev *d, uint8_t *packed);

/* Live cells over the whole grid (all ranks). Blocking. */
int64_t life_dev_live_count(life_dev *d);

/* Position-weighted checksum of the whole grid (all ranks), independent of
 * the encoding and the partition: sum over live cells (x, y) of
 * mix64(y*nx + x + 1) mod 2^64, mix64(v) = t ^ (t >> 29), t = v *
 * 0x9E3779B97F4A7C15 mod 2^64.  Lets N-shard and 1-shard runs of one grid be
 * compared at sizes no host gather reaches.  Blocking. */
int life_dev_checksum(life_dev *d, uint64_t *sum);

/* ---- Sparse I/O for grids no host buffer holds (no reference counterpart:
 * life_init fills a full host grid, life_cart.c:104-109, and life_collect
 * gathers one, :281-305).  Each shard works on its own block on the device;
 * nothing of size nx*ny is allocated on the host or crosses PCIe.  All four
 * calls are blocking and valid at any step boundary.  In rank mode they are
 * COLLECTIVE: every rank passes the same arguments, and the two readers give
 * every rank the whole result -- each rank adds its pieces to a zeroed device
 * buffer and the buffers are summed with ncclAllReduce, as the census is.
 * With world > 1 that combine has never executed (one-GPU box), as the
 * gather fan-in above has not; world 1 with a unique id runs it on a
 * one-rank communicator. */

/* Every cell dead: the state after life_dev_upload of an all-zero grid. */
int life_dev_clear(life_dev *d);

/* The n cells (xy[2k], xy[2k+1]) = (x, y), x on the contiguous axis, become
 * alive (alive != 0) or dead (0); every other cell is untouched.  Coordinates
 * wrap with a true modulo (any int64; as the driver's .cfg loader);
 * duplicates are allowed.  The list is staged on each shard's device, a
 * kernel keeps the cells of the shard's block, and the halos are then
 * refilled as after an upload (a part-used deep halo included).  n == 0 is a
 * no-op; n < 0, or xy == NULL with n > 0, is LIFE_EINVAL. */
int life_dev_set_cells(life_dev *d, const int64_t *xy, int64_t n, int alive);

/* The inverse of life_dev_gather_bits: `packed` is ny rows of ceil(nx/8)
 * bytes, cell x at bit (x & 7) of byte (x >> 3); bits at and beyond nx in a
 * row's last byte are ignored.  Replaces the whole state, as life_dev_upload,
 * at 1/8 of its host buffer, PCIe bytes and device staging: each shard copies
 * the byte columns covering its block into its kept staging buffer and a
 * kernel unpacks them into the padded layout (a byte two blocks share goes to
 * both; each keeps its own cells); the halos are then refilled as after an
 * upload.  Blocking; valid at any step boundary.  Rank mode: collective, the
 * same `packed` on every rank, each keeps its block (world > 1 has never
 * executed).  With life_dev_set_timing on, the unpack launch is one more
 * timed launch of life_dev_kernel_stats (no bytes booked). */
int life_dev_upload_bits(life_dev *d, const uint8_t *packed);

/* The periodic window of w x h cells at (x0, y0): cells[j*w + i] (0/1) is
 * cell ((x0 + i) mod nx, (y0 + j) mod ny); x0, y0 any int64, 1 <= w <= nx,
 * 1 <= h <= ny (else LIFE_EINVAL).  Read straight from the padded blocks (up
 * to four wrapped pieces per shard); device staging is w*h bytes. */
int life_dev_gather_rect(life_dev *d, int64_t x0, int64_t y0, int64_t w, int64_t h, uint8_t *cells);

/* The inverse of life_dev_gather_rect: cell ((x0 + i) mod nx, (y0 + j) mod ny)
 * becomes cells[j*w + i] != 0; every other cell is untouched.  x0, y0 any
 * int64; 1 <= w <= nx, 1 <= h <= ny, else LIFE_EINVAL.  The window is staged
 * (w*h bytes) on every shard it touches and pasted into the padded block in up
 * to four wrapped pieces; the halos are then refilled as after
 * life_dev_set_cells (a part-used deep halo included).  Blocking; valid at
 * any step boundary.  Rank mode: collective with identical arguments on every
 * rank (world > 1 has never executed). */
int life_dev_set_rect(life_dev *d, int64_t x0, int64_t y0, int64_t w, int64_t h, const uint8_t *cells);

/* Block-summed density map: ceil(ny/fy) rows of ceil(nx/fx) counts,
 * counts[by*bw + bx] = live cells with x / fx == bx and y / fy == by (the last
 * bin row / column may be partial).  fx, fy >= 1 and fx*fy < 2^32, else
 * LIFE_EINVAL; a factor larger than the grid gives one bin on that axis.
 * One streaming pass over the owned words (popcounts under per-bin masks). */
int life_dev_gather_density(life_dev *d, int64_t fx, int64_t fy, uint32_t *counts);

int life_dev_sync(life_dev *d);
/* life_dev_sync, then (rank mode) an all-reduce every rank joins: the
 * synchronisation the reference gets from its blocking MPI calls; the driver
 * brackets its timer with it.  Blocking. */
int life_dev_barrier(life_dev *d);
/* Visible HIP devices (hipGetDeviceCount), or a negative LIFE_E* code. */
int life_device_count(void);
int life_dev_layout(life_dev *d, int local_shard, life_layout *out);
int life_dev_world(life_dev *d, int *world, int *dims0, int *dims1, int *nlocal, int *transport);
/* Where local shard `local_shard` runs (measurement support, so a multi-GPU
 * result can prove what it ran on): its HIP device ordinal, that device's PCI
 * bus id (hipDeviceGetPCIBusId; distinct per physical GPU, up to 63 chars +
 * NUL), and the rank count of its RCCL communicator (ncclCommCount; 0 when
 * the shard has none, e.g. LOCAL transport).  Any out pointer may be NULL. */
int life_dev_shard_info(life_dev *d, int local_shard, int *device, char pci_bus_id[64], int *rccl_nranks);

/* Kernel timing for roofline reporting: when on, every stencil launch is
 * bracketed by HIP events on the stream it runs on.  stats returns the mean
 * device time of one stencil launch (ms), the number of launches, and the
 * algorithmic HBM bytes one launch moves (1 B read + 1 B written per cell for
 * BYTE, 2 bits for BIT, over the cells that launch updates).  on = 1 also
 * records the overlapped schedule's phase events (life_dev_phase_stats: ring,
 * interior, halo, block); on = 2 times the launches only (their events are
 * stamped by the dispatches themselves), leaving no event packets between the
 * ring, halo and interior work of a partitioned step; on = 3 records only
 * the call's span (life_dev_call_stats) on a multi-stream call -- per-launch
 * events there put ~10 us between back-to-back launches (profiles/r05/c, d) --
 * while a single-stream call keeps its one event pair around all launches. */
int life_dev_set_timing(life_dev *d, int on);

/* Execution-path switches (defaults 1): LIFE_OPT_SMALL_GRID lets a
 * single-shard grid that fits one CU run all generations of a step call in
 * one resident-workgroup launch (1: the grid in VGPRs when its shape allows,
 * else in LDS; 2: LDS only; 0: off); LIFE_OPT_OVERLAP overlaps the halo
 * exchange with the interior kernel on partitioned grids.  Results are
 * identical either way (tests switch them to reach every kernel). */
#define LIFE_OPT_SMALL_GRID 1
#define LIFE_OPT_OVERLAP 2
/* (option 3, the sweep stencil, was removed: slower than the tiles in every
 * measured case, profiles/r02/sweep_ab.txt) */
/* LIFE_OPT_BLOCK_GENS: the tiled stencil's generations per launch at most
 * (1..32, capped by generations_per_exchange; 0: the default, 12 for bits
 * and 32 for bytes, or LIFE_BLOCK_GENS from the environment).  A step call of
 * g generations runs ceil(g / max) launches of nearly equal size; a bit
 * launch of m generations holds m ghost rows above and below each tile
 * (tile height 8R - 2m), a byte launch K. */
#define LIFE_OPT_BLOCK_GENS 5
/* LIFE_OPT_SMALL_GRID value 3: the register-resident small-grid kernel
 * WINDOWED over several CUs whenever the shape allows
 * (life_kernels.hip rsmall_kernel<.., WIN>): ceil(h / own) workgroups, each
 * holding its own rows plus K halo rows above and below for K generations
 * per launch; value 1 (default) windows only grids whose one-workgroup strips
 * would be 4 or more rows tall (p46gun_big).  LIFE_OPT_SMALL_WINDOW sets the
 * strip height R and K as value = R * 256 + K (R in 1..6 or 8, K <= 255;
 * default and value 0: automatic, R = 1, K = min(30, (strips - 4) / 2)).  Shapes it does
 * not fit run as value 1 without the window.  Value 4: as 1, never
 * windowed (the one-workgroup kernel; tests). */
#define LIFE_OPT_SMALL_WINDOW 4
/* LIFE_OPT_LOOPBACK (default 0; single-shard devices only): 1 runs the one
 * shard as a periodic Cartesian partition of itself -- both axes' halos are
 * exchanged through the transport with the shard as its own left and right
 * neighbour (two sends and two receives to one peer per phase, as at
 * dims = 2), the boundary ring and interior overlapped on their streams,
 * instead of the stencil wrapping the axes.  With a rank-mode device
 * (life_dev_create_rank, world 1, a unique id) the messages are RCCL
 * ncclSend/ncclRecv: how one GPU executes the multi-GPU data path.  Results
 * are identical either way.  The grid must be at least one halo deep
 * (generations_per_exchange rows).  Value 2 loops the x axis only, 3 the y
 * axis only (the other axis wraps in the stencil): the axes a real partition
 * cuts -- N = 2's {2, 1} blocks exchange columns only. */
#define LIFE_OPT_LOOPBACK 6
/* LIFE_OPT_FLOW (default 3, automatic, or LIFE_FLOW from the environment): a step call
 * on a single shard whose axes both wrap inside it (bit encoding, width a
 * multiple of 64) runs its whole passes of m generations (m = the block
 * size, LIFE_OPT_BLOCK_GENS; at least 4 passes) as ONE persistent launch: workgroups pull
 * (pass, tile) items in order and a tile starts when the tiles its window
 * reads have finished the previous pass, so no pass boundary drains the chip;
 * the remainder runs as an ordinary launch.  1: write-through hand-off
 * stores; 2: plain stores + a release fence per tile; 0: off; 3: form 1
 * when a pass is under 5 rounds of resident workgroups (its launch tail
 * would idle the chip: 32768^2), else off (65536^2, where the per-launch
 * tiles measured 3 % faster).  The byte encoding always runs
 * per-launch tiles.  Same results.  Neither this option nor
 * LIFE_OPT_SMALL_GRID applies while a rule other than B3/S23 is set
 * (life_dev_set_rule): the dataflow and small-grid kernels exist for B3/S23
 * only, and those calls run the per-launch tiles or the one-generation
 * kernel. */
#define LIFE_OPT_FLOW 7
/* LIFE_OPT_FLOW_CHUNK (default 0 = automatic): the dataflow launch's queue
 * head is a 32-bit counter, so a step call's passes are split over several
 * persistent launches, each with passes x tiles + resident workgroups below
 * 2^31 pulls; a positive value caps the passes per launch further (tests). */
#define LIFE_OPT_FLOW_CHUNK 8
/* LIFE_OPT_DEEP_HALO (default 1; LIFE_DEEP_HALO=0 at load time turns it
 * off): partitioned bit shards with K-deep aprons exchange their halo only
 * when the next pass would outrun it -- the passes in between also advance
 * the apron cells they will read (rows [-e, 0) and [h, h + e), the apron
 * pairs), so one exchange feeds up to K generations instead of one pass of
 * at most LIFE_OPT_BLOCK_GENS.  0: one exchange per pass.  Same results.
 * The value decides which passes exchange, so every rank must hold the same
 * one: in rank mode (world > 1) this option is COLLECTIVE -- every rank calls
 * it with the same value at the same step boundary; it checks agreement
 * with an RCCL all-reduce and fails with LIFE_EINVAL (all ranks keep the old
 * value) when ranks differ, or with LIFE_ERCCL after LIFE_COMM_TIMEOUT_S when
 * a rank never calls it.  Part-used aprons are refilled by the next step's
 * first pass that needs them.  Every life_dev_configure call waits for the
 * device (life_dev_sync). */
#define LIFE_OPT_DEEP_HALO 9
/* Option 10 (LIFE_OPT_SKEW, time-skewed ghost-free tiles) was retired in
 * round 5: 8 % slower per launch on MI355X; it now fails
 * with LIFE_EINVAL like any unknown option. */
/* LIFE_OPT_PIPELINE (default LIFE_PIPELINE from the environment, else 1):
 * a step call of at least 2 per-launch tile passes on a single shard whose
 * axes both wrap inside it cuts every pass into R row regions, one launch
 * each, dealt alternately over the shard's two compute streams and ordered
 * by events: a region of pass p + 1 waits only for the regions r - 1, r, r + 1
 * of pass p, and the order rotates by one region per pass, so the first
 * region of the next pass starts in the launch tail of this one instead of
 * behind a drained chip.  0: off (one launch per pass); 1: automatic (R =
 * 4, when a pass holds at least 4 rounds of resident workgroups and the call
 * at least 4 passes: where measured to win); 3..16: that many
 * regions whenever the tile grid allows (at least 2 tile rows per region).
 * Either encoding; LIFE_OPT_FLOW decides first.  Passes timed one by one
 * (life_dev_set_timing with LIFE_TIMING_MODE 1 / 2) run as one launch each.
 * Same results; the statistics count one launch per pass either way. */
#define LIFE_OPT_PIPELINE 11
/* LIFE_OPT_SKIP_DEAD (default 0; 1 on; any other value LIFE_EINVAL): step a
 * sparse universe in the time of its live area.  While on, a step call runs
 * every pass as a skip-dead pass on a device that qualifies: a single shard in
 * a single process, both axes wrapped by the stencil (no partitioned axis, no
 * LIFE_OPT_LOOPBACK, a width that is a multiple of 64), the bit encoding, a
 * temporal layout, and a grid that does not take the small-grid path.  Such a
 * pass runs only the tiles whose input window -- the owned rows plus m ghost
 * rows at each end, the owned pair columns plus one edge lane column at each
 * side, wrapped periodically -- may hold a live cell; every other tile's
 * owned block ends up all dead in the destination buffer without the tile
 * body running ("nothing is born from nothing": B0 rules are refused by
 * life_dev_set_rule).  Results are bit-identical to the ordinary tiles, under
 * B3/S23 and under every rule life_dev_set_rule accepts.  The option decides
 * after LIFE_OPT_SMALL_GRID and before LIFE_OPT_FLOW / LIFE_OPT_PIPELINE: such
 * a call runs neither the dataflow form nor pipelined regions, and
 * life_dev_last_path returns LIFE_PATH_SKIP.  On every other device (byte
 * encoding, more than one shard, rank mode with world > 1, a width that is
 * no multiple of 64, a small grid) the option is accepted and has no effect,
 * as LIFE_OPT_FLOW.  The call stays asynchronous: nothing per pass is read
 * back, nothing is waited for.
 * What a tile may skip is kept in one activity map per grid buffer (per tile
 * column x 32 rows, row masks "this row of the block may hold a live cell":
 * in any pair, in its first pair, in its last pair), which the skip-dead
 * passes maintain themselves.  Every other writer of the state
 * invalidates the maps: life_dev_upload, life_dev_upload_bits,
 * life_dev_fill_random, life_dev_clear, life_dev_set_cells, life_dev_set_rect,
 * a step pass of any other form (the option toggled, a small-grid call), and
 * turning the option on; life_dev_set_rule leaves them valid.  The next step
 * call then rebuilds them first with one streaming scan of the grid (about
 * the cost of life_dev_live_count).
 * Timing (life_dev_set_timing): a skip-dead pass is ONE timed launch (its
 * plan kernel, map clear and tile launch under one bracket);
 * life_dev_kernel_work books the whole grid's cell-updates for it, while
 * bytes_per_launch and the VALU count are booked as 0 -- the host does not
 * know how many tiles ran without a readback; life_dev_activity does. */
#define LIFE_OPT_SKIP_DEAD 12
/* LIFE_OPT_POPULATION (default 0; 1 on; any other value LIFE_EINVAL): while
 * on, every life_dev_step(d, n) call records the live-cell count of the whole
 * grid after each of its n generations, for life_dev_population to read.  The
 * call stays asynchronous and nothing is read back during it; the state it
 * computes is bit-identical with the option on or off.  A call may record at
 * most 1048576 generations (LIFE_EINVAL with a message above that; split the
 * call).  Device memory: 8 B per generation of the longest recorded call and
 * shard, plus 16 KiB of counters per shard.
 * Fast path -- the bit encoding, a temporal layout, every shard a multiple of
 * 64 cells wide: the passes run census instances of the bit tiles (B3/S23 and
 * table rule; whole-block, ring / interior, deep-halo, banded, half-height
 * tail and skip-dead launches alike), which popcount the cells each tile owns
 * after every generation of the pass inside its registers: no extra pass over
 * HBM, still up to LIFE_OPT_BLOCK_GENS generations per launch.
 * life_dev_last_path reports _TILES or _SKIP as without the option, a pass
 * stays one timed launch, and life_dev_kernel_work counts the census's 2
 * operations per pair row and generation.
 * Every other device (the byte encoding, one-cell aprons, a shard width that
 * is no multiple of 64) gets the same trace the plain way: one generation per
 * launch, each followed by the census kernel of life_dev_live_count on the
 * stream -- about the cost of a host loop of life_dev_step(d, 1) +
 * life_dev_live_count(d) minus its readbacks and syncs.
 * Precedence, as under a rule other than B3/S23: LIFE_OPT_FLOW,
 * LIFE_OPT_SMALL_GRID and LIFE_OPT_PIPELINE are ignored while the option is on
 * (those shapes run the per-launch tiles or the one-generation kernel, one
 * launch per pass; the dataflow and small-grid kernels record nothing and
 * pipelined passes overlap in time); LIFE_OPT_SKIP_DEAD keeps acting, and a
 * pass of a recording call leaves the activity maps valid. */
#define LIFE_OPT_POPULATION 13
/* LIFE_OPT_RULE7 (default LIFE_RULE7 from the environment, else 3; 0..3, any
 * other value LIFE_EINVAL): which forms of the B3/S23 bit tiles compute the
 * rule in 7 bit operations per dword instead of 8 (20 instead of 22 VALU
 * instructions per pair row and generation: the column sums kept as parity
 * and not-all-equal) -- LIFE_RULE7_TILES: the per-launch tiles
 * in every launch form (whole block, ring / interior, deep-halo passes,
 * banded columns, half-height tail, pipelined regions), LIFE_RULE7_FLOW: the
 * dataflow tiles (LIFE_OPT_FLOW).  Both arms are separate kernels of the same
 * tile code and give bit-identical results; 0 runs the 8-gate kernels
 * everywhere (the A/B arm).  Accepted on every device; without effect on the
 * byte encoding, under a rule other than B3/S23, and on the census
 * (LIFE_OPT_POPULATION), skip-dead, one-generation and small-grid kernels,
 * which have one arm.  life_dev_kernel_work keeps counting 22 operations per
 * pair row for both arms ("22-op equivalents"), so rates of the two compare.
 * life_dev_last_rule_arm: the forms (the same bits) of which at least one launch
 * of the LAST life_dev_step call ran the 7-gate arm; 0 when none did. */
#define LIFE_OPT_RULE7 14
#define LIFE_RULE7_TILES 1
#define LIFE_RULE7_FLOW 2
int life_dev_last_rule_arm(life_dev *d);
int life_dev_configure(life_dev *d, int option, int value);
/* The population trace of the LAST life_dev_step call.  Blocking: waits for
 * the device.  *generations (may be NULL) = the generations that call
 * recorded: its n with LIFE_OPT_POPULATION on, 0 with the option off, for a
 * call of 0 generations and before any call.  counts[g], g < min(max,
 * *generations), = the live cells of the whole grid after generation g + 1 of
 * that call, summed over all local shards; counts == NULL with max == 0 only
 * queries the length.  In rank mode the sum across ranks is an all-reduce on
 * the shard's communicator, as life_dev_live_count's, so the call is
 * COLLECTIVE there (never executed with world > 1: one-GPU boxes). */
int life_dev_population(life_dev *d, int64_t *counts, int64_t max, int64_t *generations);
/* The skip-dead passes of the LAST life_dev_step call, summed: their number,
 * the tiles whose body ran, the tiles that only stored zeros over a block the
 * destination buffer held as possibly live, and the tiles of their tile
 * grids (run + cleared + skipped).  Blocking: waits for the device and reads
 * the counters.  Zeros when the last call ran no such pass.  Any out pointer
 * may be NULL. */
int life_dev_activity(life_dev *d, int64_t *passes, int64_t *tiles_run, int64_t *tiles_cleared, int64_t *tiles_total);
/* The rule the device evolves under (masks as life_rule_parse gives them); a
 * new device runs B3/S23.  life_dev_set_rule waits for queued work, as
 * life_dev_configure does, and may be called between any two step calls; the
 * state is untouched.  LIFE_EINVAL, with a message, for: bits above 8;
 * birth & 1 (B0 rules: the tiles' zero slots above and below the window, the
 * allocation slack rows and the row padding all rely on "nothing is born from
 * nothing" -- lifting that is out of scope); any rule other than B3/S23 on a
 * LIFE_KERNEL_BYTE device (the byte encoding is the reference-layout
 * comparison, its kernels SWAR arithmetic on byte sums: rules are a feature of
 * the bit encoding).  In rank mode (world > 1) the call is COLLECTIVE and
 * checks with the all-reduce of LIFE_OPT_DEEP_HALO that every rank passes the
 * same rule (never executed with world > 1: one-GPU boxes).
 * Paths under a rule other than B3/S23: the per-launch bit tiles in every
 * launch form (whole block, ring / interior, deep-halo passes, banded
 * columns, half-height tail, pipelined regions) and the one-generation bit
 * kernel run the rule as a compile-time variant of the same code (the table
 * tail: 25 instead of 12 bit operations per dword, 2 tiles per CU instead of
 * 3); LIFE_OPT_FLOW and LIFE_OPT_SMALL_GRID are ignored while such a rule is
 * set -- those shapes run the tiles or the one-generation kernel, and
 * life_dev_last_path reports what ran.  Setting B3/S23 again returns the
 * device to the B3/S23 kernels and paths exactly. */
int life_dev_set_rule(life_dev *d, uint32_t birth, uint32_t survive);
int life_dev_get_rule(life_dev *d, uint32_t *birth, uint32_t *survive);
/* The kernel family that ran the bulk of the last life_dev_step call:
 * LIFE_PATH_ONEGEN (one generation per launch), _TILES (temporally blocked
 * tiles, one launch per pass), _FLOW (the dataflow tiles, LIFE_OPT_FLOW),
 * _SMALL (a small-grid resident kernel), _SKIP (skip-dead passes,
 * LIFE_OPT_SKIP_DEAD); _NONE before the first step. */
#define LIFE_PATH_NONE 0
#define LIFE_PATH_ONEGEN 1
#define LIFE_PATH_TILES 2
#define LIFE_PATH_FLOW 3
#define LIFE_PATH_SMALL 5
#define LIFE_PATH_SKIP 6
int life_dev_last_path(life_dev *d);
int life_dev_kernel_stats(life_dev *d, double *avg_ms, int64_t *launches, double *bytes_per_launch);
/* The same timed launches: mean cell-updates per launch (cells x generations
 * it advanced) and mean VALU lane-operations per launch (op-count model of
 * the temporal bit stencil; 0 for the HBM-bound one-generation kernels).
 * bytes_per_launch above is the COMPULSORY HBM traffic: one read + one write
 * of every updated cell's encoding per launch, so a temporally blocked launch
 * advancing K generations books its cells once, not K times. */
int life_dev_kernel_work(life_dev *d, double *cell_updates_per_launch, double *valu_ops_per_launch);
/* Partitioned shards, timing on: mean device time per overlapped block
 * (one exchange period: 1 generation, or up to K with temporal layouts) of
 * its phases, each shard's blocks averaged -- the boundary-ring kernels
 * (compute stream), the interior kernel (second compute stream, concurrent),
 * the halo exchange of the ring's new state (comm stream: pack, ncclSend /
 * ncclRecv or local copies, unpack; from the moment the ring is done), and
 * the whole block from the ring's start to the join of the three streams.
 * block - interior is what the halo and ring add to the critical path (0 when
 * fully hidden).  Zeros when no block was timed (unpartitioned grids). */
int life_dev_phase_stats(life_dev *d, double *ring_ms, double *interior_ms, double *halo_ms, double *block_ms,
                         int64_t *blocks);
/* Timing on: where the wall time of the LAST life_dev_step call went
 * (measurement support; no reference counterpart -- life_cart.c times whole
 * runs with MPI_Wtime).  host_enqueue_ms: CPU time spent inside the call
 * (every launch, event, RCCL group and copy it enqueues; the call returns
 * before the device finishes); pass_enqueue_max_ms: the longest single pass
 * (one generation_block / one generation) of it; passes: its passes;
 * device_span_ms: from the first piece of work of the call starting on the
 * device to the last one ending, max over the local shards (HIP events at
 * the call's two ends on the compute stream, where the call's streams are
 * joined).  A caller that brackets the call plus a sync with its own clock
 * sees elapsed - device_span = launch latency + host-side gaps + the sync's
 * wake-up.  Zeros before the first timed call. */
int life_dev_call_stats(life_dev *d, double *host_enqueue_ms, double *pass_enqueue_max_ms, int64_t *passes,
                        double *device_span_ms);

/* Stencil tuning for the whole process, per kernel family (-1: both): rows
 * each lane walks (16/32/64) and rows of loads kept in flight (2/4/8, or 18
 * = a 16-row strip's every row loaded before the first is computed; other
 * row counts then use 4); 0 keeps the current value.  Defaults come from measurement;
 * LIFE_STEP_ROWS / LIFE_STEP_DEPTH override them at load time. */
int life_tune(int kernel, int rows, int depth);

/* Temporal (generations_per_exchange = K > 1) tile height of encoding
 * `kernel` (-1: both, each taking the value if valid for it): register rows
 * per wave -- bit: 16/24 rows of 64-cell pairs (default 24), byte: 32/48
 * rows of 32-cell words (default 48); a tile is one workgroup of 8
 * vertically stacked waves, waves*rows - 2*ghost owned rows;
 * 0 keeps the current values; LIFE_TEMPORAL_ROWS / LIFE_TEMPORAL_ROWS_BYTE
 * override at load time. */
int life_tune_temporal(int kernel, int rows);

/* Measured HBM copy ceiling of `device` ("also report a
 * measured stream-copy ceiling"): a 16-B-per-lane grid-stride copy kernel over
 * two fresh `bytes`-sized buffers, best of `reps` runs timed with HIP events;
 * *gbps = 2 * bytes (read + write) / time.  Allocates and frees its buffers. */
int life_measure_copy(int device, int64_t bytes, int reps, double *gbps);

/* life_free (life_cart.c:146-157). */
void life_dev_destroy(life_dev *d);

/* ---- Batches: many independent small universes stepped in one launch
 * (DESIGN.md 5.11).  A life_batch holds `count` periodic nx x ny universes of
 * one shape on one GPU, in its own storage (natural 32-cell words, bit k of
 * word j = cell 32j + k, ceil(nx/32) words per row, no aprons), and one
 * stream: every call below is ordered on it, so step -> census / gather needs
 * no sync by the caller.  No reference counterpart (the reference steps one
 * grid).  Two tiers, by shape alone:
 *  LIFE_BATCH_TIER_WAVE   1 <= nx <= 128, 1 <= ny <= 64: one universe per
 *                         wave, the whole state in its registers, no barrier
 *                         and no LDS exchange per generation; any rule
 *                         life_dev_set_rule accepts, one for all universes or
 *                         one each (life_batch_set_rules); LIFE_BATCH_OPT_
 *                         SETTLE, LIFE_BATCH_OPT_CYCLE, LIFE_BATCH_OPT_ONSET.
 *  LIFE_BATCH_TIER_GROUP  every other shape the one-workgroup register kernel
 *                         of the small-grid path takes (at most 2048 cells
 *                         wide, strips of R rows dividing ny, R one of 1 2 3 4
 *                         5 6 8 10 12 16 20 25 32, at most 1024 / Wp strips,
 *                         Wp = the words per row rounded up to a power of
 *                         two): one universe per workgroup, B3/S23 only.
 * Any other shape is LIFE_EINVAL, with a message naming both limits.  Both
 * tiers take LIFE_BATCH_OPT_POPULATION. */
typedef struct life_batch life_batch; /* opaque: device memory and one stream */
#define LIFE_BATCH_TIER_WAVE 1
#define LIFE_BATCH_TIER_GROUP 2
/* Host only (no GPU needed): the tier of a shape and the bytes one universe
 * takes on the device, 4 * ceil(nx/32) * ny.  Either out pointer may be NULL.
 * LIFE_EINVAL with a message for a shape in neither tier. */
int life_batch_query(int64_t nx, int64_t ny, int *tier, int64_t *bytes_per_universe);
/* Host only: the rest of the plan of a shape, that is which kernel instance
 * and launch life_batch_step takes.  words: 32-cell words per row, ceil(nx/32);
 * threads: threads of a workgroup, 64 * its waves.  Group tier:
 * lanes_per_strip = Wp, `words` rounded up to a power of two; rows = the strip
 * height R; strips = ny / R (strips * lanes_per_strip of the threads own
 * words).  Wave tier: lanes_per_strip, rows and strips are 0.  Any out pointer
 * may be NULL.  Refuses what life_batch_query refuses, with the same message. */
int life_batch_query_plan(int64_t nx, int64_t ny, int *tier, int *words, int *lanes_per_strip, int *rows, int *strips,
                          int *threads);
/* count >= 1 universes, all dead, on HIP device `device`, rule B3/S23,
 * generation 0.  Blocking.  LIFE_EINVAL: the shape (as life_batch_query), count
 * < 1, out NULL; LIFE_EHIP: no such device; LIFE_ENOMEM. */
int life_batch_create(int64_t nx, int64_t ny, int64_t count, int device, life_batch **out);
void life_batch_destroy(life_batch *b);
/* Universes [first, first + n) from / to n dense grids of ny * nx bytes each,
 * row-major, one after the other (upload: nonzero = alive; gather: 0 / 1).
 * Both block until `grids` may be reused / is filled.  upload resets the
 * settled flag of the universes it writes and of no other; one that covers all
 * universes restarts the generation counter at 0.  LIFE_EINVAL: first < 0, n <
 * 0, first + n > count, grids NULL with n > 0. */
int life_batch_upload(life_batch *b, int64_t first, int64_t n, const uint8_t *grids);
int life_batch_gather(life_batch *b, int64_t first, int64_t n, uint8_t *grids);
/* Every universe filled at random: universe u is bit for bit what
 * life_dev_fill_random(seed + u mod 2^64, thr32) gives an nx x ny grid.
 * Asynchronous.  Resets every settled flag and the generation counter. */
int life_batch_fill_random(life_batch *b, uint64_t seed, uint32_t thr32);
/* The rule of the following steps (masks as life_rule_parse gives them); the
 * states are untouched, every settled flag is cleared (a state settled under
 * one rule is not settled under another).  LIFE_EINVAL, with a message: bits
 * above 8, B0 rules, any rule other than B3/S23 on a group-tier batch. */
int life_batch_set_rule(life_batch *b, uint32_t birth, uint32_t survive);
int life_batch_get_rule(life_batch *b, uint32_t *birth, uint32_t *survive);
/* A rule per universe (wave tier): universes [first, first +
 * n) take the masks birth[k] / survive[k], the others keep theirs.  The states
 * and the generation counter are untouched; the settled and cycle flags of the
 * universes written, and of no others, are cleared.  Ordered on the batch's
 * stream; the host arrays may be reused on return.  n == 0 is a no-op.
 * LIFE_EINVAL, with a message naming the first offending index and its rule,
 * and nothing changed: a bad range (as life_batch_upload), an entry with bits
 * above 8 or B0, an entry other than B3/S23 on a group-tier batch (which stays
 * uniform: there the call only clears the flags).
 * From a call with n > 0 until the next life_batch_set_rule a wave-tier batch
 * is "mixed", whatever the values: it holds a table of 8 B per universe on the
 * device (allocated by the first such call, released by life_batch_set_rule),
 * every universe steps through the table tail of its own masks (B3/S23
 * included), and life_batch_get_rule returns LIFE_ESTATE (ask life_batch_
 * get_rules).  life_batch_get_rules always works: on a uniform batch it repeats
 * the one rule.  Either out pointer may be NULL.  Blocking. */
int life_batch_set_rules(life_batch *b, int64_t first, int64_t n, const uint32_t *birth, const uint32_t *survive);
int life_batch_get_rules(life_batch *b, int64_t first, int64_t n, uint32_t *birth, uint32_t *survive);
/* Generations rules on the wave tier (semantics: life_rule_
 * parse_gen above).  life_batch_set_rule_gen is life_batch_set_rule with a
 * state count: it refuses what that refuses, states outside 2 .. LIFE_GEN_MAX_
 * STATES, and states > 2 on a group-tier batch (LIFE_EINVAL with a message,
 * nothing changed); with states = 2 it is life_batch_set_rule.  life_batch_
 * set_rules_gen is life_batch_set_rules with a state count per universe, under
 * the same conventions (the first offending entry is named, nothing changed;
 * the batch is "mixed" afterwards); the table entry stays 8 B, the state count
 * in the high half of the birth word.  life_batch_set_rules writes states = 2.
 * The get calls mirror life_batch_get_rule (LIFE_ESTATE on a mixed batch) and
 * life_batch_get_rules; any out pointer may be NULL.  While the uniform rule
 * has states > 2, life_batch_get_rule returns LIFE_ESTATE (ask life_batch_
 * get_rule_gen).
 * EVERY set-rule call, old or new, resets the dying cells of the universes it
 * covers to dead (life_batch_set_rule and _set_rule_gen: all of them; the
 * _set_rules forms: their range) and leaves the alive cells untouched, beside
 * clearing the settled and cycle flags as documented above: no universe ever
 * holds a state at or above its state count.
 * Storage: the alive plane is the batch's storage as before (life_batch_query's
 * bytes_per_universe stays the alive plane's).  The dying cells live in 1
 * (states <= 3), 2 (<= 5) or 4 (<= 16) extra bit planes of the same word
 * layout, plane-major, each bytes_per_universe x count bytes, as many as the
 * largest state count the batch has seen since it last was two-state needs:
 * allocated, zeroed, when a rule with states > 2 first arrives, grown when a
 * larger one does, released when life_batch_set_rule (or _set_rule_gen with
 * states = 2) returns the batch to two states.  A batch that never saw such a
 * rule allocates nothing and runs the kernels it ran before.
 * The older calls keep their meaning, applied to the alive plane: life_batch_
 * upload (nonzero = alive) clears the dying cells of the universes it writes,
 * life_batch_gather returns 0 / 1 of "alive", life_batch_census counts the
 * alive cells and sums over them, life_batch_fill_random gives a random alive
 * plane with nothing dying.  LIFE_BATCH_OPT_SETTLE and LIFE_BATCH_OPT_CYCLE
 * compare the whole state, every plane.
 * life_batch_upload_states / life_batch_gather_states are upload / gather with
 * the state s itself in every byte.  The upload checks on the host, before
 * anything is written, that every byte is below the state count of its
 * universe: LIFE_EINVAL naming the universe and the value otherwise.
 * life_batch_census_gen: per universe, `count` entries each, any may be NULL:
 * the cells with s = 1, the cells with s >= 2, and the sum over all cells of s
 * x mix64(y * nx + x + 1) mod 2^64 (life_batch_census's checksum where nothing
 * is dying).  Blocking.
 * Out of scope: Generations on the group tier, on life_dev and in the driver;
 * B0; more than 16 states; random fills of dying cells. */
int life_batch_set_rule_gen(life_batch *b, uint32_t birth, uint32_t survive, uint32_t states);
int life_batch_get_rule_gen(life_batch *b, uint32_t *birth, uint32_t *survive, uint32_t *states);
int life_batch_set_rules_gen(life_batch *b, int64_t first, int64_t n, const uint32_t *birth, const uint32_t *survive,
                             const uint32_t *states);
int life_batch_get_rules_gen(life_batch *b, int64_t first, int64_t n, uint32_t *birth, uint32_t *survive,
                             uint32_t *states);
int life_batch_upload_states(life_batch *b, int64_t first, int64_t n, const uint8_t *grids);
int life_batch_gather_states(life_batch *b, int64_t first, int64_t n, uint8_t *grids);
int life_batch_census_gen(life_batch *b, int64_t *live, int64_t *dying, uint64_t *checksum);
/* LIFE_BATCH_OPT_SETTLE (wave tier, value 0 / 1, default 0): while on, a wave
 * compares its universe after each generation of a step call, from the call's
 * second on, with the state two generations earlier.  At the first generation
 * g with S_g == S_(g-2) (still lifes and period-2 oscillators) it records the
 * absolute generation (life_batch_settled), runs (n - g) mod 2 more generations
 * and exits: the state it leaves is exactly the state after all n.  A
 * universe already flagged runs n mod 2 generations in later calls.  States
 * are bit-identical with the option on and off.  LIFE_EINVAL: a group-tier
 * batch, any other option or value, turning it on while LIFE_BATCH_OPT_CYCLE
 * is on (two detectors for one wave: pick one).
 * LIFE_BATCH_OPT_CYCLE (wave tier, value 0 / 1, default 0): cycle detection of
 * any period by Brent's algorithm, restarted at every step call.  In a call of
 * n generations from state S_0 at absolute generation G_0: T = S_0, power = 1,
 * lam = 0; for g = 1 .. n: compute S_g, increment lam; if S_g == T the
 * universe is cyclic with the exact minimal period lam, recorded with the
 * absolute generation G_0 + g (life_batch_cycles), and detection stops; else
 * if lam == power: T = S_g, power *= 2, lam = 0.  The checkpoints fall at g =
 * 2^k - 1, and a cycle of period p entered after m generations is found at g
 * = c + p for the first checkpoint c >= m with c + 1 >= p.  After detection
 * at g the wave runs (n - g) mod p more generations and exits; a universe
 * already flagged runs n mod p generations in later calls.  States are bit-
 * identical with the option on and off.  Detection restarts per call: a call
 * of n generations finds what Brent finds within n, so a long run belongs in
 * few long calls (a glider on a 32 x 32 torus, period 128, is found by one
 * step(255) and not by step(100) + step(155)).  life_batch_settled is not
 * touched by this option.  LIFE_EINVAL: a group-tier batch, a value other
 * than 0 / 1, turning it on while LIFE_BATCH_OPT_SETTLE is on.
 * LIFE_BATCH_OPT_POPULATION (both tiers, value 0 / 1, default 0): while on,
 * every life_batch_step(b, n) records, for every universe, the live cells
 * after each of the call's n generations (life_batch_population), in the
 * kernels that hold the universes: the call stays one asynchronous launch and
 * nothing is read back during it.  The states, census, settled flags and
 * cycle pairs it leaves are bit-identical with the option on and off; with a
 * detector on, a wave computes all n generations instead of leaving early, so
 * the trace is complete for every universe.  A recording call holds count x n
 * entries of 4 bytes on the device, in a buffer allocated on first need, grown
 * to the largest call and released by life_batch_destroy and by turning the
 * option off.  A call of more than 2^30 entries (4 GiB) is refused with
 * LIFE_EINVAL before anything is allocated or launched, with the states and
 * the generation counter unchanged: split the call.  Two-state universes
 * only: LIFE_EINVAL when turned on while a universe's rule has more than two
 * states, and from life_batch_set_rule_gen / _set_rules_gen with more than
 * two states while it is on (their two-state calls keep working).
 * LIFE_BATCH_OPT_ONSET (wave tier, value 0 / 1, default 0): the exact onset of
 * the cycle beside its period.  It acts together with LIFE_BATCH_OPT_CYCLE.
 * While both are on, the wave that finds universe u's period lam at
 * generation g of a call from state S_0 at absolute generation G_0 also runs
 * Brent's second phase: it advances a copy of S_0 by lam generations and
 * steps S_0 and S_lam together until they are equal, which gives
 *   mu = min { m >= 0 : S_m == S_(m+lam) }     (Generations: in every plane)
 * and records onset[u] = G_0 + mu (life_batch_onsets).  Always mu <= g - lam:
 * the checkpoint S_(g-lam) == S_g lies on the cycle; the search is a counted
 * loop of at most g - lam steps after the lam of the copy, in registers, in
 * the same launch.  The value is max(true onset, G_0): the exact generation at
 * which the orbit entered its cycle when that happened at or after G_0 -- in
 * particular in the first step call after an upload or fill -- and G_0 for a
 * universe that was already cycling at G_0 without being flagged.  A universe
 * flagged before the option was turned on keeps -1 until its flags are reset.
 * States, census, cycle pairs, the generation counter and population traces
 * are bit-identical with the option on and off: the search's generations are
 * recorded in no trace.  LIFE_EINVAL, with nothing changed: a group-tier
 * batch, a value other than 0 / 1, turning it on while LIFE_BATCH_OPT_CYCLE is
 * off.  Turning LIFE_BATCH_OPT_CYCLE off turns this option off as well.
 * (LIFE_BATCH_OPT_SETTLE needs no such option: its generation minus 2 is the
 * exact onset already.)
 * Option number 2 is unassigned and stays LIFE_EINVAL. */
#define LIFE_BATCH_OPT_SETTLE 1
#define LIFE_BATCH_OPT_CYCLE 3
#define LIFE_BATCH_OPT_POPULATION 4
/* = 5.  Spelled from its neighbour: tests/test_batch_population_host.py, which
 * predates the option, pins the literal numbers defined here to exactly 1, 3,
 * 4; tests/test_batch_onset_host.py evaluates this one and holds all four to
 * 1, 3, 4, 5. */
#define LIFE_BATCH_OPT_ONSET (LIFE_BATCH_OPT_POPULATION + 1)
int life_batch_configure(life_batch *b, int option, int value);
/* All universes advance `generations`.  Asynchronous (one launch); 0 is a
 * no-op; LIFE_EINVAL when negative or above INT32_MAX. */
int life_batch_step(life_batch *b, int64_t generations);
/* Per universe, `count` entries each, either may be NULL: the live cells, and
 * life_dev_checksum's sum evaluated with the universe's own nx (the sum over
 * its live (x, y) of mix64(y * nx + x + 1)).  Blocking. */
int life_batch_census(life_batch *b, int64_t *live, uint64_t *checksum);
/* Per universe, `count` entries: the absolute generation (on the counter of
 * life_batch_generation) at which LIFE_BATCH_OPT_SETTLE found it settled, -1
 * if it has not.  Blocking. */
int life_batch_settled(life_batch *b, int64_t *generation);
/* Per universe, `count` entries each, either may be NULL: the period
 * LIFE_BATCH_OPT_CYCLE found and the absolute generation it found it at; 0 and
 * -1 where it has found none.  A universe's pair goes back to 0 / -1 with an
 * upload or a life_batch_set_rules range that covers it, all of them with
 * life_batch_fill_random and life_batch_set_rule.  Blocking. */
int life_batch_cycles(life_batch *b, int64_t *period, int64_t *generation);
/* Per universe, `count` entries: the absolute generation LIFE_BATCH_OPT_ONSET
 * recorded as the onset of the universe's cycle (max(true onset, G_0) of the
 * call that found the period, see the option), -1 where none was recorded; all
 * -1 when the option was never on.  An entry goes back to -1 exactly where the
 * universe's cycle pair goes back to 0 / -1 (life_batch_cycles).  Blocking. */
int life_batch_onsets(life_batch *b, int64_t *generation);
/* The population trace of LIFE_BATCH_OPT_POPULATION.  *generations (may be
 * NULL) is the number G of generations the last life_batch_step call
 * recorded: its n with the option on; 0 with the option off, for a call of 0
 * generations, and before any call.  counts[(u - first) * G + g] is the live
 * cells of universe u, first <= u < first + n, after generation g + 1 of that
 * call; counts == NULL only queries G.  Range errors are those of
 * life_batch_gather.  The trace stays readable until the next step call or
 * until the option is turned off: uploads, fills and rule changes do not
 * touch it.  Blocking. */
int life_batch_population(life_batch *b, int64_t first, int64_t n, uint32_t *counts, int64_t *generations);
/* Generations stepped since the states were last written as a whole
 * (creation, life_batch_fill_random, an upload of all universes).  Host only. */
int life_batch_generation(life_batch *b, int64_t *generation);
/* Waits for the batch's stream. */
int life_batch_sync(life_batch *b);

/* ---- which item a workgroup of a bit-tile launch runs (host only, no GPU) --
 * One per-launch bit-tile launch as its launcher describes it: up to
 * LIFE_TILE_MAX_REGIONS tile regions, tile columns [tx0, tx1) x tile rows
 * [ty0, ty1) of window_rows - 2 m owned rows each, region k's items numbered
 * from first[k] (first[0] = 0, first[nreg] = all of them): its ordinary tiles
 * row-major, then the banded items of its last tile column when tx1 == btx1
 * and nband > 0 (sub-column i in items of 64 >> bgsh[i] tile rows).  tail_ntx
 * > 0 (one region): workgroups from tail_first on run half-height tiles over
 * owned rows [tail_y, tail_yend), tail_ntx tile columns from tail_tx0 per tile
 * row, listed the same way.  xcd_n: the workgroups renumbered into per-XCD
 * row-major runs (0: dispatch order). */
#define LIFE_TILE_MAX_REGIONS 4
typedef struct life_tile_launch {
    int32_t nreg, nband, m, window_rows;
    int64_t tx0[LIFE_TILE_MAX_REGIONS], tx1[LIFE_TILE_MAX_REGIONS], ty0[LIFE_TILE_MAX_REGIONS],
        ty1[LIFE_TILE_MAX_REGIONS], first[LIFE_TILE_MAX_REGIONS + 1];
    int32_t bgsh[2];
    int64_t btx1;
    int64_t tail_first, tail_y, tail_yend, tail_ntx, tail_tx0;
    int64_t xcd_n;
} life_tile_launch;
#define LIFE_TILE_NONE 0      /* a workgroup beyond the items: does nothing */
#define LIFE_TILE_FULL 1      /* ordinary tile (tx, ty) of `region` */
#define LIFE_TILE_BAND 2      /* banded item `band_item` of `region` (tile rows [ty0, ty0 + rows)) */
#define LIFE_TILE_TAIL 3      /* half-height tile: column tx, tile row ty of the tail's `rows` */
#define LIFE_TILE_TAIL_BAND 4 /* banded item `band_item` of the tail */
typedef struct life_tile_item {
    int32_t kind, region, tx, ty, ty0, rows;
    int64_t band_item;
} life_tile_item;
/* The decode the kernels run (32-bit arithmetic on constants made once per
 * launch), replayed on the CPU: out[i] = the item of workgroup wg[i], 0 <=
 * wg[i] < 2^31.  LIFE_EINVAL, with a message: a description that is
 * inconsistent or whose counts leave the 32-bit range the kernels work in
 * (such a launch fails on the device path too). */
int life_tile_decode_query(const life_tile_launch *launch, const int64_t *wg, int64_t n, life_tile_item *out);

#ifdef __cplusplus
}
#endif
#endif /* LIFE_MI355X_H */
