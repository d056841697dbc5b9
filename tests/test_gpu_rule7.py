"""The 7-gate arm of the B3/S23 bit tiles (LIFE_OPT_RULE7; ConwayRule7 in
csrc/life_bitops.h, tstep_bit7_kernel / tflow7_kernel in life_kernels.hip).

The rule is computed per bit, so what can go wrong is which kernel a launch
form selects and the geometry it is given, not the size: one shape, 4160 x
1400 at 50 % (65 pairs: one full tile column and a banded one of 3 pairs; its
5.8 M cells meet all 512 neighbourhoods), 25 generations, on every launch form
that has a 7-gate instance.  Each run is compared cell for cell with the
oracle, by checksum and live count with the 8-gate arm on the same form, and
life_dev_last_rule_arm says which arm each side really ran -- the test cannot
pass with one arm on both sides.
"""
import numpy as np
import pytest

from test_gpu_pipeline import reference

pytestmark = pytest.mark.gpu

NX, NY, SEED, GENS = 4160, 1400, 3, 25


def run(gpu, oracle, arm, want_arm, gens=GENS, path="tiles", setup=None, nx=NX, **kw):
    """One device on the form `kw` / `setup` select, LIFE_OPT_RULE7 = arm: the oracle's cells, and
    (checksum, live count); the arm the call ran is `want_arm`."""
    kw.setdefault("flow", 0)
    with gpu.Life(nx, NY, kernel="bit", small_grid=False, **kw) as life:
        life.configure(gpu.OPT_RULE7, arm)
        if setup:
            setup(life)
        life.upload(reference(oracle, nx, NY, SEED, 0))
        assert life.last_rule7() == 0  # nothing stepped yet
        life.step(gens)
        assert life.last_path() == path
        assert life.last_rule7() == want_arm
        want = reference(oracle, nx, NY, SEED, gens)
        np.testing.assert_array_equal(life.gather(), want)
        census = (life.checksum(), life.live_count())
        assert census == (oracle.checksum(want), int(want.sum()))
        return census


def both(gpu, oracle, arm, want_arm, **kw):
    seven = run(gpu, oracle, arm, want_arm, **kw)
    eight = run(gpu, oracle, 0, 0, **kw)
    assert seven == eight


def test_per_launch_tiles(gpu, oracle):
    """LIFE_OPT_FLOW 0: whole launches, the banded column and the half-height tail."""
    both(gpu, oracle, gpu.RULE7_TILES, gpu.RULE7_TILES)
    # the dataflow bit alone leaves the per-launch tiles on 8 gates
    run(gpu, oracle, gpu.RULE7_FLOW, 0)


@pytest.mark.parametrize("flow", [1, 2])
def test_dataflow(gpu, oracle, flow):
    """4 dataflow passes of 6 (the banded instance: the last column owns 3 pairs) and one
    generation of per-launch tiles behind them: each form follows its own bit."""
    six = lambda life: life.configure(gpu.OPT_BLOCK_GENS, 6)  # noqa: E731
    both(gpu, oracle, gpu.RULE7_FLOW, gpu.RULE7_FLOW, path="flow", setup=six, flow=flow)
    run(gpu, oracle, gpu.RULE7_FLOW | gpu.RULE7_TILES, gpu.RULE7_FLOW | gpu.RULE7_TILES, path="flow", setup=six,
        flow=flow)
    run(gpu, oracle, gpu.RULE7_TILES, gpu.RULE7_TILES, path="flow", setup=six, flow=flow)


def test_dataflow_without_a_banded_column(gpu, oracle):
    """3968 wide: 62 pairs, one tile column exactly -- the dataflow instance without banded items."""
    six = lambda life: life.configure(gpu.OPT_BLOCK_GENS, 6)  # noqa: E731
    both(gpu, oracle, gpu.RULE7_FLOW, gpu.RULE7_FLOW, path="flow", setup=six, flow=1, nx=3968)


def test_pipelined_call(gpu, oracle):
    """48 generations as 4 passes of 12, each 4 region launches over two streams."""
    four = lambda life: life.configure(gpu.OPT_PIPELINE, 4)  # noqa: E731
    both(gpu, oracle, gpu.RULE7_TILES, gpu.RULE7_TILES, gens=48, setup=four)


@pytest.mark.parametrize("dims", [(2, 1), (1, 2)], ids=["cut_x", "cut_y"])
def test_two_local_shards(gpu, oracle, dims):
    """Two shards in one process, cut along x (blocks of 32.5 pairs) or along y: the instances that
    do not wrap the cut axis, ring and interior launches, and the deep-halo passes that also
    advance the apron."""
    both(gpu, oracle, gpu.RULE7_TILES, gpu.RULE7_TILES, shards=2, dims=dims, transport=gpu.XPORT_LOCAL)


def test_option_values(gpu):
    with gpu.Life(256, 256, kernel="bit") as life:
        for bad in (-1, 4):
            with pytest.raises(RuntimeError):
                life.configure(gpu.OPT_RULE7, bad)
    # accepted where it has no effect: the byte tiles have one arm
    with gpu.Life(2048, 1000, kernel="byte", small_grid=False) as life:
        life.configure(gpu.OPT_RULE7, 3)
        life.fill_random(3, 0.5)
        life.step(40)
        assert life.last_rule7() == 0
    # a rule other than B3/S23 runs the table tail, whatever the option says
    with gpu.Life(2048, 1000, kernel="bit", small_grid=False, rule="B36/S23") as life:
        life.configure(gpu.OPT_RULE7, 3)
        life.fill_random(3, 0.5)
        life.step(40)
        assert life.last_rule7() == 0
