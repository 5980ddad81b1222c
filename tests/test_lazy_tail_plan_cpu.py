"""Where an InstanceNorm backward tail runs inside the kernel that consumes it is ONE decision (csrc/lazy_tail_plan.hpp), queried through the C ABI
(rsuper_maxpool2_bwd_lazy_plan / rsuper_upsample_bwd_lazy_plan) by the modules before they hand out a differentiable statistics tensor and read again by
the launches.  This pins its answers for the shapes of the UNet step (B = 2, 96^3, base 32) and for what the fused kernels do not take.  Pure host
code: no GPU."""
import pytest

N = 2
POOL_STEP = [(96, 32), (48, 64), (24, 128), (12, 256)]                  # input of the pooling layer of down1 .. down4
UP_STEP = [(48, 96, 64), (24, 48, 128), (12, 24, 256), (6, 12, 320)]    # trilinear input, output, channels of up4 .. up1


@pytest.fixture
def L():
    from rsuper_amd.hip import lib
    L = lib.lib()
    assert L.rsuper_lazy_tails(-1) == 1
    yield L
    assert L.rsuper_lazy_tails(1) == 1


def test_pool_plan(L):
    from rsuper_amd.hip import lib
    for dt in (lib.BF16, lib.F32):
        for S, C in POOL_STEP:
            assert L.rsuper_maxpool2_bwd_lazy_plan(dt, N, S, S, S, C) == 1, (dt, S, C)
        assert L.rsuper_maxpool2_bwd_lazy_plan(dt, N, 4, 4, 6, 8) == 1
        for odd in ((5, 4, 6), (4, 5, 6), (4, 4, 7)):            # the never-pooled trailing plane takes the skip gradient alone
            assert L.rsuper_maxpool2_bwd_lazy_plan(dt, N, *odd, 8) == 0, odd
        assert L.rsuper_maxpool2_bwd_lazy_plan(dt, N, 4, 4, 6, 4) == 0          # no entry of the library takes C % 8 != 0
        assert L.rsuper_maxpool2_bwd_lazy_plan(dt, 65536, 4, 4, 6, 8) == 0      # N is a grid dimension
    assert L.rsuper_maxpool2_bwd_lazy_plan(lib.BF16, N, 4, 4, 6, 8 * 257) == 0  # more than 256 vectors per voxel
    assert L.rsuper_maxpool2_bwd_lazy_plan(lib.F32, N, 4, 4, 6, 8 * 129) == 0


def test_upsample_plan(L):
    from rsuper_amd.hip import lib
    got = [L.rsuper_upsample_bwd_lazy_plan(lib.BF16, N, I, I, I, O, O, O, C) for I, O, C in UP_STEP]
    assert got == UP_STEP_ANSWERS, got
    for I, O, C in UP_STEP:
        assert L.rsuper_upsample_bwd_lazy_plan(lib.F32, N, I, I, I, O, O, O, C) == 0       # f32 finalises first
    assert L.rsuper_upsample_bwd_lazy_plan(lib.BF16, N, 3, 3, 4, 6, 6, 8, 12) == 0          # C % 8
    assert L.rsuper_lazy_tails(2) == 2                                                      # the measuring switch admits every bf16 shape
    assert [L.rsuper_upsample_bwd_lazy_plan(lib.BF16, N, I, I, I, O, O, O, C) for I, O, C in UP_STEP] == [1, 1, 1, 1]
    assert L.rsuper_upsample_bwd_lazy_plan(lib.F32, N, 3, 3, 4, 6, 6, 8, 8) == 0


def test_switch_and_bad_arguments(L):
    from rsuper_amd.hip import lib
    assert L.rsuper_lazy_tails(0) == 0 and L.rsuper_lazy_tails(-1) == 0 and L.rsuper_lazy_tails(7) == 0
    assert all(L.rsuper_maxpool2_bwd_lazy_plan(lib.BF16, N, S, S, S, C) == 0 for S, C in POOL_STEP)
    assert all(L.rsuper_upsample_bwd_lazy_plan(lib.BF16, N, I, I, I, O, O, O, C) == 0 for I, O, C in UP_STEP)
    assert L.rsuper_lazy_tails(1) == 1
    good = (lib.BF16, N, 4, 4, 6, 8)
    for i, bad in ((0, 5), (1, 0), (2, 0), (3, -2), (4, 0), (5, 0)):
        a = list(good); a[i] = bad
        assert L.rsuper_maxpool2_bwd_lazy_plan(*a) < 0, (i, bad)
    good = (lib.BF16, N, 3, 3, 4, 6, 6, 8, 8)
    for i, bad in ((0, 5), (1, 0), (2, 0), (5, 0), (8, -8)):
        a = list(good); a[i] = bad
        assert L.rsuper_upsample_bwd_lazy_plan(*a) < 0, (i, bad)


# the rule of lazy_up_plan at the step's four shapes: the fused trilinear backward measured no faster at 96^3 and slower at the other three
# (profiles/lazy_in_bwd_tails.md), so all four stay on two launches
UP_STEP_ANSWERS = [0, 0, 0, 0]
