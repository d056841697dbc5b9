/*
 * life.c -- reference-compatible driver over the MI355X C ABI.
 *
 * Drop-in for the reference programs' main() (6-cartesian/life_cart.c:51-85,
 * 5-gather/life_mpi.c:36-63, 3-life/life_mpi.c:38-72):
 *
 *   life_mi355x file.cfg            same .cfg, same vtk/life_%06d.vtk bytes,
 *                                   same "%f\n" elapsed seconds on stdout
 *
 * Extensions (all optional; without them the program behaves as the
 * reference with one process and one GPU):
 *   --gpus N          shards driven by this process (one per GPU; with more
 *                     shards than GPUs they share devices, LOCAL transport)
 *   --kernel byte|bit cell encoding (default bit)
 *   --partition cart|rows|cols|auto   shard shape (life_dims_choose; default
 *                     cart = MPI_Dims_create as life_cart.c:117-118; rows =
 *                     the 1-D strips of 3-life/5-gather; the grid is the same)
 *   --nx N --ny N --steps N --save-steps N   override the .cfg header
 *   --random SEED[,DENSITY]                  device-side random init instead
 *                                            of the .cfg cells (no file needed)
 *   --no-vtk          skip frame output (timing runs)
 *   --format vtk|bits frame format: the reference's VTK text (default) or a
 *                     packed binary dump vtk/life_%06d.bits (checkpoint)
 *   --format density:FX[xFY]   frames are block-summed live counts
 *                     (life_dev_gather_density): vtk/life_%06d.dens holds the
 *                     line "LIFEDENS 1 nx ny fx fy generation\n", then
 *                     ceil(ny/FY) rows of ceil(nx/FX) little-endian uint32;
 *                     FY defaults to FX; only the map is allocated for frames
 *   --sparse          the .cfg cells go to the device as a coordinate list
 *                     (life_dev_clear + life_dev_set_cells): the nx*ny host
 *                     grid is never allocated; same cells, same frames.  With
 *                     --format density a pattern in a 65536^2 universe needs
 *                     kilobytes on the host
 *   --skip-dead       step only the tiles whose window may hold a live cell
 *                     (LIFE_OPT_SKIP_DEAD, set before the first step): the run
 *                     time follows the pattern, not the universe; same frames
 *                     and dumps.  Independent of --sparse, which is I/O only;
 *                     no effect where the device does not qualify (byte
 *                     kernel, several GPUs, a width that is no multiple of 64)
 *   --resume FILE     start from a .bits dump instead of the .cfg cells: the
 *                     dump sets nx and ny and goes to the device packed
 *                     (life_dev_upload_bits); frames continue its numbering
 *   --at X,Y          with --resume: the dump is a pattern, pasted with its
 *                     first cell at (X, Y) (any integers, wrapped) into an
 *                     empty universe of --nx x --ny cells (both required;
 *                     life_dev_clear + life_dev_set_rect); the dump must fit
 *   --rule TEXT       the Life-like rule, "B36/S23" or Golly's "23/36" (S/B)
 *                     (life_rule_parse, life_dev_set_rule; default B3/S23, the
 *                     reference's rule; bit kernel only, no B0 rules)
 *   --population FILE write the population curve: one line "generation live"
 *                     ("%lld %lld\n") for the starting generation (a
 *                     life_dev_live_count before the first step) and for every
 *                     generation of the run (LIFE_OPT_POPULATION: counted inside
 *                     the stepping kernels, read with life_dev_population after
 *                     each step call, between frames); frames and the printed
 *                     time keep their format
 *   --live            print the live-cell count after the run to stderr
 *   --rank-mode       one-process-per-GPU mode even without a launcher (world 1)
 *
 * Under a launcher -- `torchrun --nproc-per-node P`, `mpirun -np P`
 * (MPICH: PMI_RANK/PMI_SIZE, Open MPI: OMPI_COMM_WORLD_*), as the reference
 * is run (3-life/job_life.sh:8) -- every process drives the one Cartesian
 * block of its rank on GPU LOCAL_RANK; the RCCL unique id goes from rank 0 to
 * the others over TCP (bootstrap.c); rank P-1 (the root of life_collect,
 * life_cart.c:283-286) writes the frames and prints the time.
 *
 * Frames: the VTK cell text is formatted on the device
 * (life_dev_gather_vtk) and written while the next generations run (the
 * step call is asynchronous), inside the reference's timed region.
 *
 * Differences from the reference, on purpose: malformed .cfg files and
 * save_steps <= 0 are errors (the reference loops forever / raises SIGFPE),
 * coordinates wrap with a true modulo (the reference's (i+nx)%nx is only
 * defined for i >= -nx), and sizes are 64-bit.
 */
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "bootstrap.h"
#include "life_mi355x.h"

static void die(const char *what, int rc) {
    fprintf(stderr, "life_mi355x: %s: %s%s%s\n", what, life_strerror(rc), *life_last_error() ? ": " : "",
            life_last_error());
    exit(1);
}

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

static int64_t wrapi(int64_t i, int64_t n) { return ((i % n) + n) % n; }

typedef struct {
    int64_t steps, save_steps, nx, ny;
    uint8_t *grid; /* nx*ny 0/1 cells, row-major (NULL until loaded) */
    int64_t *cells; /* --sparse: ncells (i, j) pairs as written in the file, instead of grid */
    int64_t ncells;
} cfg_t;

/* .cfg loader: life_cart.c:92-111.  "steps\n save_steps\n nx ny\n" then one
 * "i j" live cell per line until EOF; cell (i, j) wraps periodically
 * (life_cart.c:106-109).  The file is mapped and the cell lines are parsed by
 * up to 16 threads, each on a line-aligned chunk writing straight into the
 * grid (a 32768^2 random pattern is a ~6 GB file).  A chunk whose token count
 * is odd (pairs not one per line) sends the whole body to the sequential
 * parser, which pairs tokens across lines like the reference's fscanf loop. */
typedef struct {
    const char *p, *end;
    int64_t nx, ny;
    uint8_t *grid;
    int status; /* 0 ok, 1 odd token count, 2 malformed */
} parse_job;

static int next_int(const char **pp, const char *end, long long *v) {
    const char *p = *pp;
    while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++;
    if (p == end) {
        *pp = p;
        return 0; /* EOF */
    }
    int neg = 0;
    if (*p == '-' || *p == '+') neg = *p++ == '-';
    if (p == end || *p < '0' || *p > '9') return -1;
    long long x = 0;
    while (p < end && *p >= '0' && *p <= '9') x = x * 10 + (*p++ - '0');
    if (p < end && !(*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) return -1;
    *v = neg ? -x : x;
    *pp = p;
    return 1;
}

static void *parse_cells(void *arg) {
    parse_job *jb = (parse_job *)arg;
    const char *p = jb->p;
    long long i, j;
    for (;;) {
        int r = next_int(&p, jb->end, &i);
        if (r == 0) break;
        if (r < 0) {
            jb->status = 2;
            return NULL;
        }
        r = next_int(&p, jb->end, &j);
        if (r == 0) {
            jb->status = 1;
            return NULL;
        }
        if (r < 0) {
            jb->status = 2;
            return NULL;
        }
        /* u0[ind(i, j)] = 1; threads may store the same cell (duplicates,
         * wrapped coordinates): relaxed atomic stores, no data race */
        __atomic_store_n(&jb->grid[wrapi(j, jb->ny) * jb->nx + wrapi(i, jb->nx)], (uint8_t)1, __ATOMIC_RELAXED);
    }
    jb->status = 0;
    return NULL;
}

/* --sparse: the cell lines as a list of (i, j) pairs, unwrapped
 * (life_dev_set_cells wraps them); tokens pair up across lines like the
 * reference's fscanf loop. */
static int parse_cell_list(const char *p, const char *end, cfg_t *c) {
    int64_t cap = 0;
    for (;;) {
        long long v[2];
        int r = next_int(&p, end, &v[0]);
        if (r == 0) return LIFE_OK;
        if (r < 0 || next_int(&p, end, &v[1]) != 1) return LIFE_EIO;
        if (c->ncells == cap) {
            cap = cap ? 2 * cap : 1024;
            int64_t *q = (int64_t *)realloc(c->cells, (size_t)cap * 2 * sizeof *q);
            if (!q) return LIFE_ENOMEM;
            c->cells = q;
        }
        c->cells[2 * c->ncells] = v[0];
        c->cells[2 * c->ncells + 1] = v[1];
        c->ncells++;
    }
}

static int load_cfg(const char *path, cfg_t *c, int64_t o_nx, int64_t o_ny, int sparse) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return LIFE_EIO;
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(fd);
        return LIFE_EIO;
    }
    const size_t len = (size_t)st.st_size;
    const char *base = len ? (const char *)mmap(NULL, len, PROT_READ, MAP_PRIVATE, fd, 0) : "";
    close(fd);
    if (base == MAP_FAILED) return LIFE_EIO;
    const char *p = base, *end = base + len;
    long long v[4];
    int rc = LIFE_OK;
    for (int k = 0; k < 4 && rc == LIFE_OK; k++)
        if (next_int(&p, end, &v[k]) != 1) rc = LIFE_EIO;
    if (rc == LIFE_OK && (v[2] <= 0 || v[3] <= 0)) rc = LIFE_EIO;
    if (rc == LIFE_OK) {
        c->steps = v[0];
        c->save_steps = v[1];
        c->nx = o_nx > 0 ? o_nx : v[2]; /* --nx/--ny override the header before the cells wrap */
        c->ny = o_ny > 0 ? o_ny : v[3];
        if (!sparse) {
            c->grid = (uint8_t *)calloc((size_t)(c->nx * c->ny), 1);
            if (!c->grid) rc = LIFE_ENOMEM;
        }
    }
    if (rc == LIFE_OK && sparse) {
        rc = parse_cell_list(p, end, c);
    } else if (rc == LIFE_OK) {
        enum { kMaxThreads = 16 };
        long np = sysconf(_SC_NPROCESSORS_ONLN);
        int nt = (int)((size_t)(end - p) / (1 << 22)); /* >= 4 MiB per thread */
        if (nt > kMaxThreads) nt = kMaxThreads;
        if (nt > np) nt = (int)np;
        if (nt < 1) nt = 1;
        parse_job jobs[kMaxThreads];
        pthread_t th[kMaxThreads];
        const char *q = p;
        for (int t = 0; t < nt; t++) { /* line-aligned chunks */
            const char *e = t == nt - 1 ? end : p + (size_t)(end - p) * (size_t)(t + 1) / (size_t)nt;
            while (e < end && *e != '\n') e++;
            jobs[t] = (parse_job){q, e, c->nx, c->ny, c->grid, 0};
            q = e;
        }
        int started = 0;
        for (int t = 1; t < nt; t++)
            if (pthread_create(&th[t], NULL, parse_cells, &jobs[t]) == 0) started = t;
            else break;
        parse_cells(&jobs[0]);
        for (int t = 1; t <= started; t++) pthread_join(th[t], NULL);
        for (int t = started + 1; t < nt; t++) parse_cells(&jobs[t]); /* threads that did not start */
        int odd = 0;
        for (int t = 0; t < nt; t++) {
            if (jobs[t].status == 2) rc = LIFE_EIO;
            odd |= jobs[t].status == 1;
        }
        if (rc == LIFE_OK && odd) { /* pairs split across lines: one sequential pass */
            parse_job all = {p, end, c->nx, c->ny, c->grid, 0};
            parse_cells(&all);
            if (all.status) rc = LIFE_EIO;
        }
    }
    if (len) munmap((void *)base, len);
    if (rc != LIFE_OK) {
        free(c->grid);
        free(c->cells);
        c->grid = NULL;
        c->cells = NULL;
        c->ncells = 0;
    }
    return rc;
}

static FILE *open_frame(const char *path) {
    struct stat st;
    if (stat("vtk", &st) == -1) mkdir("vtk", 0700); /* life_cart.c:163-166 */
    return fopen(path, "w");
}

/* life_save_vtk: life_cart.c:159-187, byte-identical output; `body` is the
 * "%d\n"-per-cell text (y outer, x inner) formatted by life_dev_gather_vtk. */
static int save_vtk(const char *path, int64_t nx, int64_t ny, const char *body) {
    FILE *f = open_frame(path);
    if (!f) return LIFE_EIO;
    fprintf(f, "# vtk DataFile Version 3.0\n");
    fprintf(f, "Created by write_to_vtk2d\n");
    fprintf(f, "ASCII\n");
    fprintf(f, "DATASET STRUCTURED_POINTS\n");
    fprintf(f, "DIMENSIONS %lld %lld 1\n", (long long)nx + 1, (long long)ny + 1);
    fprintf(f, "SPACING %d %d 0.0\n", 1, 1);
    fprintf(f, "ORIGIN %d %d 0.0\n", 0, 0);
    fprintf(f, "CELL_DATA %lld\n", (long long)(nx * ny));
    fprintf(f, "SCALARS life int 1\n");
    fprintf(f, "LOOKUP_TABLE life_table\n");
    const size_t n = (size_t)(2 * nx * ny);
    const int ok = fwrite(body, 1, n, f) == n;
    return fclose(f) == 0 && ok ? LIFE_OK : LIFE_EIO;
}

/* Packed binary frame (extension, not in the reference): a text line
 * "LIFEBITS 1 <nx> <ny> <generation>\n", then ny rows of ceil(nx/8) bytes,
 * cell x of a row at bit (x & 7) of byte (x >> 3) -- packed on the device
 * (life_dev_gather_bits), written as one block. */
static int save_bits(const char *path, int64_t nx, int64_t ny, int64_t gen, const uint8_t *packed) {
    FILE *f = open_frame(path);
    if (!f) return LIFE_EIO;
    fprintf(f, "LIFEBITS 1 %lld %lld %lld\n", (long long)nx, (long long)ny, (long long)gen);
    const size_t n = (size_t)(ny * ((nx + 7) / 8));
    const int ok = fwrite(packed, 1, n, f) == n;
    return fclose(f) == 0 && ok ? LIFE_OK : LIFE_EIO;
}

/* Density frame (extension): "LIFEDENS 1 <nx> <ny> <fx> <fy> <generation>\n",
 * then ceil(ny/fy) rows of ceil(nx/fx) uint32 live counts as
 * life_dev_gather_density wrote them (little-endian hosts). */
static int save_density(const char *path, int64_t nx, int64_t ny, int64_t fx, int64_t fy, int64_t gen,
                        const uint32_t *counts) {
    FILE *f = open_frame(path);
    if (!f) return LIFE_EIO;
    fprintf(f, "LIFEDENS 1 %lld %lld %lld %lld %lld\n", (long long)nx, (long long)ny, (long long)fx, (long long)fy,
            (long long)gen);
    const size_t n = (size_t)(((nx + fx - 1) / fx) * ((ny + fy - 1) / fy));
    const int ok = fwrite(counts, sizeof *counts, n, f) == n;
    return fclose(f) == 0 && ok ? LIFE_OK : LIFE_EIO;
}

/* A save_bits frame, still packed: ny rows of ceil(nx/8) bytes read as one
 * block (what life_dev_upload_bits takes; no nx*ny grid). */
static int load_bits(const char *path, int64_t *nx, int64_t *ny, int64_t *gen, uint8_t **packed) {
    FILE *f = fopen(path, "r");
    if (!f) return LIFE_EIO;
    long long v, a, b, g;
    if (fscanf(f, "LIFEBITS %lld %lld %lld %lld", &v, &a, &b, &g) != 4 || v != 1 || a <= 0 || b <= 0 || g < 0 ||
        fgetc(f) != '\n') {
        fclose(f);
        return LIFE_EIO;
    }
    const size_t n = (size_t)(b * ((a + 7) / 8));
    uint8_t *out = (uint8_t *)malloc(n);
    const int ok = out && fread(out, 1, n, f) == n;
    fclose(f);
    if (!ok) {
        free(out);
        return LIFE_EIO;
    }
    *nx = a;
    *ny = b;
    *gen = g;
    *packed = out;
    return LIFE_OK;
}

/* --at: the dump as a dense window of its own size, cells[j*w + i] 0/1 (what
 * life_dev_set_rect takes). */
static uint8_t *unpack_bits(const uint8_t *packed, int64_t w, int64_t h) {
    const int64_t rb = (w + 7) / 8;
    uint8_t *out = (uint8_t *)malloc((size_t)(w * h));
    if (!out) return NULL;
    for (int64_t y = 0; y < h; y++)
        for (int64_t x = 0; x < w; x++) out[y * w + x] = (uint8_t)((packed[y * rb + (x >> 3)] >> (x & 7)) & 1u);
    return out;
}

int main(int argc, char **argv) {
    const char *cfg_path = NULL, *resume = NULL, *pop_path = NULL;
    int gpus = 1, kernel = LIFE_KERNEL_BIT, vtk = 1, live = 0, have_random = 0, bits = 0, force_rank = 0;
    int partition = LIFE_PARTITION_CART, sparse = 0, have_at = 0, skip_dead = 0;
    long long at_x = 0, at_y = 0; /* --at X,Y */
    long long dfx = 0, dfy = 0; /* --format density:FX[xFY] (bits == 2) */
    long long o_nx = -1, o_ny = -1, o_steps = -1, o_save = -1;
    unsigned long long seed = 0;
    double density = 0.5;
    uint32_t birth = LIFE_RULE_CONWAY_BIRTH, survive = LIFE_RULE_CONWAY_SURVIVE; /* --rule */
    int have_rule = 0;
    for (int a = 1; a < argc; a++) {
        const char *s = argv[a];
        const int more = a + 1 < argc;
        if (!strcmp(s, "--gpus") && more) gpus = atoi(argv[++a]);
        else if (!strcmp(s, "--partition") && more) {
            const char *p = argv[++a];
            partition = !strcmp(p, "cart")   ? LIFE_PARTITION_CART
                        : !strcmp(p, "rows") ? LIFE_PARTITION_ROWS
                        : !strcmp(p, "cols") ? LIFE_PARTITION_COLS
                        : !strcmp(p, "auto") ? LIFE_PARTITION_AUTO
                                             : -1;
        }
        else if (!strcmp(s, "--kernel") && more) {
            const char *k = argv[++a];
            kernel = !strcmp(k, "byte") ? LIFE_KERNEL_BYTE : !strcmp(k, "bit") ? LIFE_KERNEL_BIT : -1;
        } else if (!strcmp(s, "--nx") && more) o_nx = atoll(argv[++a]);
        else if (!strcmp(s, "--ny") && more) o_ny = atoll(argv[++a]);
        else if (!strcmp(s, "--steps") && more) o_steps = atoll(argv[++a]);
        else if (!strcmp(s, "--save-steps") && more) o_save = atoll(argv[++a]);
        else if (!strcmp(s, "--random") && more) {
            have_random = 1;
            char *end;
            seed = strtoull(argv[++a], &end, 10);
            if (*end == ',') {
                char *dend;
                density = strtod(end + 1, &dend);
                if (*dend || !(density >= 0.0 && density <= 1.0)) {
                    fprintf(stderr, "life_mi355x: --random density must be in [0, 1]\n");
                    return 1;
                }
            }
        } else if (!strcmp(s, "--no-vtk")) vtk = 0;
        else if (!strcmp(s, "--format") && more) {
            const char *fm = argv[++a];
            bits = !strcmp(fm, "bits") ? 1 : !strcmp(fm, "vtk") ? 0 : -1;
            if (!strncmp(fm, "density:", 8)) {
                char *end;
                dfx = dfy = strtoll(fm + 8, &end, 10);
                if (*end == 'x') dfy = strtoll(end + 1, &end, 10);
                bits = !*end && end != fm + 8 && dfx >= 1 && dfy >= 1 ? 2 : -1;
            }
        } else if (!strcmp(s, "--sparse")) sparse = 1;
        else if (!strcmp(s, "--skip-dead")) skip_dead = 1;
        else if (!strcmp(s, "--resume") && more) resume = argv[++a];
        else if (!strcmp(s, "--at") && more) {
            char *end;
            at_x = strtoll(argv[++a], &end, 10);
            have_at = end != argv[a] && *end == ',';
            if (have_at) {
                const char *ys = end + 1;
                at_y = strtoll(ys, &end, 10);
                have_at = end != ys && !*end;
            }
            if (!have_at) {
                fprintf(stderr, "life_mi355x: --at takes X,Y (two integers)\n");
                return 1;
            }
        }
        else if (!strcmp(s, "--rule") && more) {
            if (life_rule_parse(argv[++a], &birth, &survive) != LIFE_OK) {
                fprintf(stderr, "life_mi355x: --rule: %s\n", life_last_error());
                return 1;
            }
            have_rule = 1;
        }
        else if (!strcmp(s, "--population") && more) pop_path = argv[++a];
        else if (!strcmp(s, "--live")) live = 1;
        else if (!strcmp(s, "--rank-mode")) force_rank = 1;
        else if (s[0] != '-' && !cfg_path) cfg_path = s;
        else {
            cfg_path = NULL;
            have_random = 0;
            break;
        }
    }
    if (have_at && !resume) {
        fprintf(stderr, "life_mi355x: --at places a --resume dump: it needs --resume FILE\n");
        return 1;
    }
    if (!cfg_path && !have_random && !resume) {
        printf("Usage: %s input file.\n", argv[0]); /* life_cart.c:53-56 */
        return 0;
    }
    if (have_at && (o_nx <= 0 || o_ny <= 0)) {
        fprintf(stderr, "life_mi355x: --at needs the universe's size: --nx N --ny N\n");
        return 1;
    }
    if (kernel < 0 || gpus < 1 || bits < 0 || partition < 0) {
        fprintf(stderr, "life_mi355x: bad --kernel/--gpus/--format/--partition\n");
        return 1;
    }
    /* one process per GPU under a launcher (life_cart.c:114-115 takes rank and
     * size from MPI; here from the launcher's environment) */
    int rank = 0, world = 1, local_rank = 0;
    const int launched = life_launcher_ranks(&rank, &world, &local_rank);
    if (launched < 0) {
        fprintf(stderr, "life_mi355x: inconsistent launcher rank variables\n");
        return 1;
    }
    const int rank_mode = launched == 1 || force_rank;
    if (rank_mode && gpus != 1) {
        fprintf(stderr, "life_mi355x: --gpus drives several GPUs from one process; under a launcher every "
                        "rank drives its own GPU (drop --gpus)\n");
        return 1;
    }
    const int root = world - 1; /* life_collect's root: cart rank (dims0-1, dims1-1) = size-1 */

    cfg_t c = {0, 1, 0, 0, NULL, NULL, 0};
    if (cfg_path && load_cfg(cfg_path, &c, resume ? -1 : o_nx, resume ? -1 : o_ny, sparse) != LIFE_OK) {
        fprintf(stderr, "life_mi355x: cannot read config '%s'\n", cfg_path);
        return 1;
    }
    uint8_t *resumed = NULL; /* the dump's packed rows */
    int64_t gen0 = 0; /* generation the run starts from (a --resume dump's) */
    int64_t dump_nx = 0, dump_ny = 0;
    if (resume && load_bits(resume, &dump_nx, &dump_ny, &gen0, &resumed) != LIFE_OK) {
        fprintf(stderr, "life_mi355x: cannot read dump '%s'\n", resume);
        return 1;
    }
    if (resume && !have_at) { /* the dump is the universe */
        c.nx = dump_nx;
        c.ny = dump_ny;
    }
    if (o_nx > 0 && (!resume || have_at)) c.nx = o_nx;
    if (o_ny > 0 && (!resume || have_at)) c.ny = o_ny;
    if (have_at && (dump_nx > c.nx || dump_ny > c.ny)) {
        fprintf(stderr, "life_mi355x: the dump '%s' (%lld x %lld) does not fit the %lld x %lld universe\n", resume,
                (long long)dump_nx, (long long)dump_ny, (long long)c.nx, (long long)c.ny);
        return 1;
    }
    if (o_steps >= 0) c.steps = o_steps;
    if (o_save >= 0) c.save_steps = o_save;
    if (c.nx <= 0 || c.ny <= 0 || c.steps < 0 || c.save_steps <= 0) {
        fprintf(stderr, "life_mi355x: bad sizes nx=%lld ny=%lld steps=%lld save_steps=%lld\n",
                (long long)c.nx, (long long)c.ny, (long long)c.steps, (long long)c.save_steps);
        return 1;
    }

    life_dev *d = NULL;
    int dims[2];
    int rc = life_dims_choose(c.nx, c.ny, rank_mode ? world : gpus, partition, dims);
    if (rc == LIFE_OK && rank_mode) {
        uint8_t uid[LIFE_UID_BYTES];
        memset(uid, 0, sizeof uid);
        if (rank == 0 && (rc = life_get_unique_id(uid)) != LIFE_OK) die("unique id", rc);
        if (life_bootstrap_id(rank, world, uid, 120.0) != 0) {
            fprintf(stderr, "life_mi355x: rank %d/%d: RCCL id bootstrap over TCP failed\n", rank, world);
            return 1;
        }
        const int ndev = life_device_count();
        if (ndev <= 0) die("no HIP device", LIFE_EHIP);
        /* RCCL prints its version banner to stdout when a communicator is
         * made; stdout carries only the elapsed time (as the reference's,
         * which run_life.sh appends to times.txt): send the banner to stderr */
        fflush(stdout);
        const int saved = dup(STDOUT_FILENO);
        if (saved >= 0) dup2(STDERR_FILENO, STDOUT_FILENO);
        rc = life_dev_create_rank(c.nx, c.ny, kernel, rank, world, dims[0], dims[1], uid, local_rank % ndev, &d);
        fflush(stdout);
        if (saved >= 0) {
            dup2(saved, STDOUT_FILENO);
            close(saved);
        }
    } else if (rc == LIFE_OK) {
        rc = life_dev_create_ex(c.nx, c.ny, gpus, dims[0], dims[1], kernel, LIFE_XPORT_AUTO, &d);
    }
    if (rc) die("create", rc);
    if (have_rule && (rc = life_dev_set_rule(d, birth, survive)) != LIFE_OK) die("--rule", rc);
    if (skip_dead && (rc = life_dev_configure(d, LIFE_OPT_SKIP_DEAD, 1)) != LIFE_OK) die("--skip-dead", rc);
    if (pop_path && (rc = life_dev_configure(d, LIFE_OPT_POPULATION, 1)) != LIFE_OK) die("--population", rc);
    const int writer = !rank_mode || rank == root; /* the process that writes frames and prints */
    uint8_t *grid = NULL; /* packed rows: bits frames */
    char *body = NULL;    /* VTK cell text */
    uint32_t *dens = NULL; /* density map (every rank: the readout is collective and lands on all) */
    int64_t fx = dfx, fy = dfy;
    if (vtk && bits == 2) {
        if (fx > c.nx) fx = c.nx; /* factors beyond the grid: one bin */
        if (fy > c.ny) fy = c.ny;
        dens = (uint32_t *)calloc((size_t)(((c.nx + fx - 1) / fx) * ((c.ny + fy - 1) / fy)), sizeof *dens);
        if (!dens) die("host density map", LIFE_ENOMEM);
    }
    if (vtk && bits == 1 && writer) {
        grid = (uint8_t *)calloc((size_t)(c.ny * ((c.nx + 7) / 8)), 1);
        if (!grid) die("host grid", LIFE_ENOMEM);
    }
    if (vtk && !bits && writer) {
        body = (char *)malloc((size_t)(2 * c.nx * c.ny));
        if (!body) die("host frame", LIFE_ENOMEM);
    }
    if (resume && have_at) {
        uint8_t *win = unpack_bits(resumed, dump_nx, dump_ny);
        if (!win) die("host window", LIFE_ENOMEM);
        if ((rc = life_dev_clear(d)) == LIFE_OK) rc = life_dev_set_rect(d, at_x, at_y, dump_nx, dump_ny, win);
        free(win);
        free(resumed);
    } else if (resume) {
        rc = life_dev_upload_bits(d, resumed);
        free(resumed);
    } else if (have_random) {
        rc = life_dev_fill_random(d, seed, density >= 1.0 ? 0xFFFFFFFFu : (uint32_t)(density * 4294967296.0));
    } else if (sparse) {
        if ((rc = life_dev_clear(d)) == LIFE_OK) rc = life_dev_set_cells(d, c.cells, c.ncells, 1);
    } else {
        rc = life_dev_upload(d, c.grid);
    }
    if (rc) die("init", rc);
    free(c.grid);
    free(c.cells);
    c.grid = NULL;
    c.cells = NULL;

    /* life_cart.c:62-80: the timer starts after init and covers the frame
     * collects + VTK writes and every generation.  Generations and frame
     * numbers are absolute: a resumed run continues the dump's sequence and
     * --steps counts from generation 0. */
    /* --population: generation gen0 now, the others after each step call (collective in rank mode) */
    enum { POP_CHUNK = 65536 }; /* generations per step call at most while recording */
    FILE *pop_file = NULL;
    int64_t *pop = NULL;
    if (pop_path) {
        const int64_t n0 = life_dev_live_count(d);
        if (n0 < 0) die("--population", (int)n0);
        pop = (int64_t *)malloc(POP_CHUNK * sizeof *pop);
        if (!pop) die("host trace", LIFE_ENOMEM);
        if (writer) {
            pop_file = fopen(pop_path, "w");
            if (!pop_file || fprintf(pop_file, "%lld %lld\n", (long long)gen0, (long long)n0) < 0)
                die(pop_path, LIFE_EIO);
        }
    }
    if ((rc = life_dev_barrier(d))) die("barrier", rc);
    const double t0 = now_s();
    char path[64];
    for (int64_t i = gen0; i < c.steps;) {
        const int save = vtk && i % c.save_steps == 0;
        if (save) { /* collect (blocking, every rank), then write it while the GPU steps on */
            if ((rc = bits == 2   ? life_dev_gather_density(d, fx, fy, dens)
                      : bits == 1 ? life_dev_gather_bits(d, grid)
                                  : life_dev_gather_vtk(d, body)))
                die("gather", rc);
            snprintf(path, sizeof path,
                     bits == 2   ? "vtk/life_%06lld.dens"
                     : bits == 1 ? "vtk/life_%06lld.bits"
                                 : "vtk/life_%06lld.vtk",
                     (long long)i);
        }
        int64_t n = c.steps - i;
        if (vtk) {
            const int64_t to_save = c.save_steps - i % c.save_steps;
            if (to_save < n) n = to_save;
        }
        if (pop_path && n > POP_CHUNK) n = POP_CHUNK;
        if ((rc = life_dev_step(d, n))) die("step", rc); /* asynchronous */
        if (save && writer &&
            (rc = bits == 2   ? save_density(path, c.nx, c.ny, fx, fy, i, dens)
                  : bits == 1 ? save_bits(path, c.nx, c.ny, i, grid)
                              : save_vtk(path, c.nx, c.ny, body)))
            die(path, rc);
        if (pop_path) { /* (blocking: after the frame is written) */
            int64_t got = 0;
            if ((rc = life_dev_population(d, pop, n, &got)) || got != n) die("population", rc ? rc : LIFE_ESTATE);
            for (int64_t g = 0; g < n && pop_file; g++)
                if (fprintf(pop_file, "%lld %lld\n", (long long)(i + g + 1), (long long)pop[g]) < 0)
                    die(pop_path, LIFE_EIO);
        }
        i += n;
    }
    if ((rc = life_dev_sync(d))) die("sync", rc);
    if ((rc = life_dev_barrier(d))) die("barrier", rc);
    const double t1 = now_s();
    if (writer) printf("%f\n", t1 - t0);
    if (live) {
        const int64_t n = life_dev_live_count(d); /* collective in rank mode */
        if (writer) fprintf(stderr, "live %lld\n", (long long)n);
    }
    if (pop_file && fclose(pop_file) != 0) die(pop_path, LIFE_EIO);
    free(pop);
    life_dev_destroy(d);
    free(grid);
    free(body);
    free(dens);
    return 0;
}
