"""The batch plan without a GPU (life_batch_query, csrc/life_plan.cpp
batch_plan): which tier a shape runs in, what a universe takes on the device,
and the refusals."""
import pytest

WAVE = [(1, 1), (2, 3), (33, 7), (128, 64)]
GROUP = [(500, 500), (2048, 16), (160, 96),
         (129, 67)]  # 5 words round up to 8 lanes per strip: 67 one-row strips take 536 of the 1024 threads
# neither tier: too wide; empty; 131 is prime and 131 one-row strips of 8 lanes do not fit 1024 threads
REFUSED = [(4096, 4096), (0, 5), (129, 131)]


@pytest.mark.parametrize("nx,ny", WAVE)
def test_wave_tier(lm, nx, ny):
    assert lm.batch_query(nx, ny) == ("wave", 4 * -(-nx // 32) * ny)


@pytest.mark.parametrize("nx,ny", GROUP)
def test_group_tier(lm, nx, ny):
    assert lm.batch_query(nx, ny) == ("group", 4 * -(-nx // 32) * ny)


def test_tier_boundary(lm):
    """Every shape up to 128 x 64 is the wave tier; one more column or row is not."""
    for nx in range(1, 129):
        for ny in (1, 2, 37, 64):
            assert lm.batch_query(nx, ny)[0] == "wave", (nx, ny)
    assert lm.batch_query(129, 64)[0] == "group" and lm.batch_query(128, 65)[0] == "group"


@pytest.mark.parametrize("nx,ny", REFUSED)
def test_refused_shapes(lm, nx, ny):
    with pytest.raises(lm.LifeError) as e:
        lm.batch_query(nx, ny)
    assert e.value.rc == -1  # LIFE_EINVAL
    detail = lm._lib().life_last_error().decode()
    assert detail and "128" in detail and "2048" in detail  # names both limits


def test_query_out_pointers_are_optional(lm):
    assert lm._lib().life_batch_query(33, 7, None, None) == 0


def test_no_cpu_fallback_without_gpu(lm):
    from conftest import gpu_available

    if gpu_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(lm.LifeError):
        lm.LifeBatch(16, 16, 3)
