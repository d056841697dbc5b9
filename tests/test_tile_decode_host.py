"""Which item a workgroup of a per-launch bit-tile kernel runs, replayed on the
CPU (life_tile_decode_query: csrc/life_tile_decode.h, the function the kernels
call, on the constants the launcher makes).  No GPU.

For every launch description: the workgroup ids map one-to-one onto the
launch's items, and the mapping equals the 64-bit formulas the kernels used
before (tstep_bit_kernel's XCD renumbering, region search, wr % ntx / wr / ntx,
tail_item), restated here in Python integers."""
import ctypes
import random

import pytest

MAXR = 4
NONE, FULL, BAND, TAIL, TAIL_BAND = range(5)


class Launch(ctypes.Structure):
    _fields_ = [("nreg", ctypes.c_int32), ("nband", ctypes.c_int32), ("m", ctypes.c_int32),
                ("window_rows", ctypes.c_int32),
                ("tx0", ctypes.c_int64 * MAXR), ("tx1", ctypes.c_int64 * MAXR), ("ty0", ctypes.c_int64 * MAXR),
                ("ty1", ctypes.c_int64 * MAXR), ("first", ctypes.c_int64 * (MAXR + 1)),
                ("bgsh", ctypes.c_int32 * 2), ("btx1", ctypes.c_int64),
                ("tail_first", ctypes.c_int64), ("tail_y", ctypes.c_int64), ("tail_yend", ctypes.c_int64),
                ("tail_ntx", ctypes.c_int64), ("tail_tx0", ctypes.c_int64), ("xcd_n", ctypes.c_int64)]


class Item(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("region", ctypes.c_int32), ("tx", ctypes.c_int32), ("ty", ctypes.c_int32),
                ("ty0", ctypes.c_int32), ("rows", ctypes.c_int32), ("band_item", ctypes.c_int64)]


def ceil_div(a, b):
    return -(-a // b)


def band_items(rows, gsh):
    return sum(ceil_div(rows, 64 >> g) for g in gsh)


def make(regions, gsh=(), btx1=-1, m=12, window=192, tail=None, xcd=True):
    """regions: (tx0, tx1, ty0, ty1); gsh: log2 lane group of each banded sub-column of tile column btx1 - 1;
    tail: (tail_y, tail_yend) = the owned rows re-tiled at half height below the one region."""
    L = Launch()
    L.nreg, L.nband, L.m, L.window_rows, L.btx1 = len(regions), len(gsh), m, window, btx1
    for i in range(2):
        L.bgsh[i] = gsh[i] if i < len(gsh) else 6
    first = 0
    for k, (tx0, tx1, ty0, ty1) in enumerate(regions):
        L.tx0[k], L.tx1[k], L.ty0[k], L.ty1[k], L.first[k] = tx0, tx1, ty0, ty1, first
        banded = len(gsh) > 0 and tx1 == btx1
        first += (tx1 - tx0 - banded) * (ty1 - ty0) + (band_items(ty1 - ty0, gsh) if banded else 0)
    L.first[len(regions)] = first
    total = first
    if tail:
        tx0, tx1 = regions[0][0], regions[0][1]
        rows = ceil_div(tail[1] - tail[0], window // 2 - 2 * m)
        banded = len(gsh) > 0 and tx1 == btx1
        L.tail_first, L.tail_y, L.tail_yend, L.tail_ntx, L.tail_tx0 = first, tail[0], tail[1], tx1 - tx0, tx0
        total += (tx1 - tx0 - banded) * rows + (band_items(rows, gsh) if banded else 0)
    L.xcd_n = first if xcd else 0
    return L, total


def decode_ref(L, wg):
    """tstep_bit_kernel before the 32-bit decode, in unbounded integers."""
    if wg < L.xcd_n:
        n, x, k = L.xcd_n, wg & 7, wg >> 3
        per, rem = n >> 3, n & 7
        wg = (x * (per + 1) if x < rem else rem * (per + 1) + (x - rem) * per) + k
    if L.tail_ntx > 0 and wg >= L.tail_first:
        i = wg - L.tail_first
        ts = L.window_rows // 2 - 2 * L.m
        rows = (L.tail_yend - L.tail_y + ts - 1) // ts
        band = L.nband > 0 and L.tail_tx0 + L.tail_ntx == L.btx1
        ntxs = L.tail_ntx - (1 if band else 0)
        nfull = ntxs * rows
        if i < nfull:
            return (TAIL, L.tail_tx0 + i % ntxs, i // ntxs, rows)
        return (TAIL_BAND, i - nfull, rows)
    if wg >= L.first[L.nreg]:
        return (NONE,)
    k = 0
    while k + 1 < L.nreg and wg >= L.first[k + 1]:
        k += 1
    wr = wg - L.first[k]
    bands = L.nband > 0 and L.tx1[k] == L.btx1
    ntx = L.tx1[k] - L.tx0[k] - (1 if bands else 0)
    nfull = ntx * (L.ty1[k] - L.ty0[k])
    if wr < nfull:
        return (FULL, k, L.tx0[k] + wr % ntx, L.ty0[k] + wr // ntx)
    return (BAND, k, wr - nfull, L.ty0[k], L.ty1[k] - L.ty0[k])


def decode_lib(lm, L, wgs):
    n = len(wgs)
    out = (Item * n)()
    rc = lm._lib().life_tile_decode_query(ctypes.byref(L), (ctypes.c_int64 * n)(*wgs), ctypes.c_int64(n), out)
    assert rc == 0, lm._lib().life_last_error()
    got = []
    for it in out:
        got.append({NONE: (NONE,), FULL: (FULL, it.region, it.tx, it.ty),
                    BAND: (BAND, it.region, it.band_item, it.ty0, it.rows),
                    TAIL: (TAIL, it.tx, it.ty, it.rows), TAIL_BAND: (TAIL_BAND, it.band_item, it.rows)}[it.kind])
    return got


def expected_items(L):
    """Every item of the launch, each once."""
    want = []
    gsh = [L.bgsh[i] for i in range(L.nband)]
    for k in range(L.nreg):
        banded = L.nband > 0 and L.tx1[k] == L.btx1
        rows = L.ty1[k] - L.ty0[k]
        want += [(FULL, k, tx, ty) for ty in range(L.ty0[k], L.ty1[k]) for tx in range(L.tx0[k], L.tx1[k] - banded)]
        if banded:
            want += [(BAND, k, i, L.ty0[k], rows) for i in range(band_items(rows, gsh))]
    if L.tail_ntx > 0:
        rows = ceil_div(L.tail_yend - L.tail_y, L.window_rows // 2 - 2 * L.m)
        banded = L.nband > 0 and L.tail_tx0 + L.tail_ntx == L.btx1
        want += [(TAIL, tx, ty, rows) for ty in range(rows)
                 for tx in range(L.tail_tx0, L.tail_tx0 + L.tail_ntx - banded)]
        if banded:
            want += [(TAIL_BAND, i, rows) for i in range(band_items(rows, gsh))]
    return want


def launches():
    out = {}
    for xcd in (True, False):
        x = "xcd" if xcd else "plain"
        # 65536^2 at m = 12: 1024 pairs = 16 tile columns + 32 pairs as sub-columns of 30 (G = 32) and 2 (G = 4);
        # 391 tile rows of 168; the pipelined passes' four row regions, each a launch of its own ...
        g64k = dict(gsh=(5, 2), btx1=17, xcd=xcd)
        for i, (ty0, ty1) in enumerate(((0, 96), (96, 192), (192, 288), (288, 391))):
            out[f"65536-region{i}-{x}"] = make([(0, 17, ty0, ty1)], **g64k)
        out[f"65536-four-regions-{x}"] = make([(0, 17, 0, 96), (0, 17, 96, 192), (0, 17, 192, 288), (0, 17, 288, 391)],
                                              **g64k)
        # ... and one launch whose last rows run as half-height tiles (72 owned rows each)
        out[f"65536-tail-{x}"] = make([(0, 17, 0, 385)], tail=(385 * 168, 65536), **g64k)
        # 32768^2: 512 pairs = 8 columns + 16 pairs in one band (G = 32), 196 tile rows
        out[f"32768-{x}"] = make([(0, 9, 0, 196)], gsh=(5,), btx1=9, xcd=xcd)
        # 16384 x 32768: 256 pairs = 4 columns + 8 pairs (G = 16); one round and a half-height tail
        out[f"16384x32768-{x}"] = make([(0, 5, 0, 190)], gsh=(4,), btx1=5, tail=(190 * 168, 32768), xcd=xcd)
        # the boundary ring of a partitioned shard under a deep halo: top, bottom, left and right (banded) strips
        out[f"ring-{x}"] = make([(0, 9, 0, 2), (0, 9, 47, 49), (0, 1, 2, 47), (8, 9, 2, 47)], gsh=(5,), btx1=9,
                                m=8, xcd=xcd)
        # a wide, short region (one tile row, 771 items for 768 slots): the tail plan re-tiles it from its first
        # tile row on, so the region keeps no row and every workgroup is a tail item (plain and banded)
        out[f"all-tail-{x}"] = make([(0, 800, 0, 0)], tail=(0, 100), xcd=xcd)
        out[f"all-tail-banded-{x}"] = make([(0, 770, 0, 0)], gsh=(5, 2), btx1=770, tail=(0, 100), xcd=xcd)
    return out


LAUNCHES = launches()


def test_item_counts_of_the_default_shape():
    assert [LAUNCHES[f"65536-region{i}-xcd"][1] for i in range(4)] == [1590, 1590, 1590, 1707]


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_workgroups_map_one_to_one_onto_the_items(lm, name):
    L, total = LAUNCHES[name]
    wgs = list(range(total))
    got = decode_lib(lm, L, wgs)
    assert got == [decode_ref(L, w) for w in wgs]
    assert sorted(got) == sorted(expected_items(L)) and len(set(got)) == total
    if L.tail_ntx == 0:  # workgroups past the items do nothing
        assert decode_lib(lm, L, [total, total + 1, 2**30, 2**31 - 1]) == [(NONE,)] * 4


def test_reciprocal_is_exact(lm):
    """wr / ntx and wr % ntx by the multiply-high reciprocal: 2000 seeded ntx up to 2^20, every wr in the first
    and last 64 of [0, nfull) and at the multiples of ntx (first, last and 64 seeded ones) - 1, + 0, + 1."""
    rng = random.Random(20240521)
    for n in range(2000):
        ntx = rng.choice((1, 2, 3, 2**20, 2**20 - 1)) if n < 10 else rng.randint(1, 2**20)
        rows = rng.randint(1, max(1, min(2**20, (2**31 - 1) // ntx - 1)))
        nfull = ntx * rows
        L, total = make([(3, 3 + ntx, 5, 5 + rows)], xcd=False)
        assert total == nfull < 2**31
        ks = set(range(min(rows, 33))) | set(range(max(0, rows - 33), rows)) | {rng.randrange(rows) for _ in range(64)}
        wrs = set(range(min(64, nfull))) | set(range(max(0, nfull - 64), nfull))
        wrs |= {k * ntx + d for k in ks for d in (-1, 0, 1) if 0 <= k * ntx + d < nfull}
        wrs = sorted(wrs)
        assert decode_lib(lm, L, wrs) == [(FULL, 0, 3 + wr % ntx, 5 + wr // ntx) for wr in wrs], ntx


def test_out_of_range_launch_is_refused(lm):
    L, _ = make([(0, 2**26, 0, 4)], xcd=False)  # pair columns beyond 2^31
    assert lm._lib().life_tile_decode_query(ctypes.byref(L), None, ctypes.c_int64(0), None) != 0
    L, _ = make([(0, 40000, 0, 60000)], xcd=False)  # 2.4e9 items
    assert lm._lib().life_tile_decode_query(ctypes.byref(L), None, ctypes.c_int64(0), None) != 0
