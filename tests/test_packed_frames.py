"""Packed LIFEBITS frames on the host: load_bits_packed reads what bits_bytes
writes without unpacking it, and the two entry points that take packed frames
and windows back into a device are part of the ABI."""
import re
import subprocess

import numpy as np
import pytest


def _grid(nx, ny):
    return (np.random.default_rng(nx * 31 + ny).random((ny, nx)) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("nx,ny,gen", [(10, 10, 0), (13, 9, 40), (64, 3, 123456)])
def test_load_bits_packed_round_trip(lm, tmp_path, nx, ny, gen):
    grid = _grid(nx, ny)
    path = tmp_path / "frame.bits"
    path.write_bytes(lm.bits_bytes(grid, gen))
    g, nx2, ny2, packed = lm.load_bits_packed(str(path))
    assert (g, nx2, ny2) == (gen, nx, ny)
    assert packed.dtype == np.uint8 and packed.shape == (ny, (nx + 7) // 8)
    np.testing.assert_array_equal(np.unpackbits(packed, axis=1, bitorder="little")[:, :nx], grid)
    g, unpacked = lm.load_bits(str(path))  # the unpacking loader reads the same frame
    assert g == gen
    np.testing.assert_array_equal(unpacked, grid)


def test_load_bits_packed_rejects_bad_frames(lm, tmp_path):
    good = lm.bits_bytes(_grid(13, 9), 7)
    bad_magic = tmp_path / "magic.bits"
    bad_magic.write_bytes(good.replace(b"LIFEBITS", b"LIFEBYTE", 1))
    short = tmp_path / "short.bits"
    short.write_bytes(good[:-1])
    for path in (bad_magic, short):
        with pytest.raises(ValueError):
            lm.load_bits_packed(str(path))
        with pytest.raises(ValueError):
            lm.load_bits(str(path))


def test_new_entry_points_are_bound_and_exported(lm):
    names = {"life_dev_upload_bits", "life_dev_set_rect"}
    assert names <= set(lm.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", lm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert names <= set(re.findall(r"\bT (life_[a-z_]+)$", out, flags=re.M))
