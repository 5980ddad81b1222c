"""The kernels of MedFormer's attention stages (csrc/pointwise.hip, depthwise.hip, instnorm.hip) at the shapes on either side of every rung of their
dispatch (csrc/mf_plan.hpp; the launches themselves are pinned by tests/test_mf_plan_cpu.py against tests/golden/mf_launches.json): the result checks
of tests/gpu_checks.py, at their tolerances, where a grid, a template argument or the kernel changes."""
import pytest
import torch

import gpu_checks as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def native():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X; the product path has no CPU fallback')
    from rsuper_amd.hip import lib
    lib.require_device()


def _ok(r):
    assert r['ok'], f"{r['name']}: err {r['err']:.3e} > tol {r['tol']:.1e}"


# forward / data gradient: 1, ragged 2, 2 and 4 tiles of 32 output channels; the reduction split over the waves from 8 k-steps (the nearest K with
# whole float4 rows: 112 | 116 bf16, 56 | 60 f32) and no longer from 128 whole-K row blocks (R = 16256 | 16257).  Weight gradient of the same call:
# WNW 1 / 4 / 2 (N, K on either side of 64), one slab | two slabs + reduce (R = 64 | 65), the slab count capped by 256 / tiles, ragged slabs
POINTWISE = [('bf16', 200, 32, 32), ('bf16', 200, 32, 36), ('f32', 200, 32, 64), ('bf16', 200, 32, 128), ('bf16', 200, 112, 64), ('bf16', 200, 116, 64),
             ('f32', 200, 56, 64), ('f32', 200, 60, 64), ('bf16', 16256, 128, 128), ('bf16', 16257, 128, 128), ('f32', 16256, 128, 128),
             ('f32', 16257, 128, 128), ('bf16', 64, 64, 64), ('bf16', 65, 64, 64), ('f32', 65, 64, 64), ('bf16', 4096, 64, 68), ('bf16', 4096, 68, 64),
             ('bf16', 4096, 68, 68), ('f32', 4096, 68, 68), ('bf16', 16448, 64, 64), ('bf16', 4160, 256, 256), ('bf16', 1000, 64, 64)]


@pytest.mark.parametrize('mode,R,K,N', POINTWISE)
def test_pointwise_at_the_rungs(mode, R, K, N):
    _ok(gc.check_pointwise(mode, R, K, N, True))


# the LDS kernel from 6 x 32 x 32 and the register-run kernel just below on each axis; two D segments from D = 12; partial channel groups of both
# kernels (32 / 64 channels per block); the register kernel's grid at its 1024-block floor and its 2048 cap; weight-gradient rows 1 | 2 (128 | 129
# voxels) and 1024 reached | kept (131072 | 131073)
DEPTHWISE = [(32, (6, 32, 32)), (32, (5, 32, 32)), (32, (6, 31, 32)), (32, (6, 32, 31)), (32, (11, 32, 32)), (32, (12, 32, 32)), (4, (6, 32, 32)),
             (36, (6, 32, 32)), (68, (6, 32, 32)), (4, (4, 6, 7)), (36, (4, 6, 7)), (68, (4, 6, 7)), (4, (5, 256, 256)), (4, (5, 512, 512)),
             (4, (1, 8, 16)), (4, (1, 3, 43)), (4, (32, 64, 64)), (4, (1, 3, 43691))]


@pytest.mark.parametrize('C,dims', DEPTHWISE, ids=[f'C{c}_{"x".join(map(str, d))}' for c, d in DEPTHWISE])
def test_depthwise_at_the_rungs(C, dims):
    _ok(gc.check_depthwise(C, dims, 1))


# one launch | three launches (512 | 513 voxels), the apply grid capped at 2048 blocks (32768 | 32769), 512 statistics rows capped (65536 | 65537);
# one partial and two channel groups; with and without the ReLU
CNORM = [(4, (8, 8, 8), False, 1), (4, (1, 19, 27), False, 1), (68, (8, 8, 8), True, 2), (68, (1, 19, 27), True, 2), (4, (32, 32, 32), True, 1),
         (4, (1, 3, 10923), False, 1), (4, (64, 32, 32), False, 1), (4, (1, 1, 65537), True, 1)]


@pytest.mark.parametrize('C,dims,relu,N', CNORM, ids=[f'C{c}_{"x".join(map(str, d))}_r{int(r)}' for c, d, r, _ in CNORM])
def test_channel_norm_at_the_rungs(C, dims, relu, N):
    _ok(gc.check_cnorm(C, dims, relu, N))


@pytest.mark.parametrize('r', [16, 17, 32, 33])      # 16 hidden units per block forward, 32 backward
def test_squeeze_excite_at_the_rungs(r):
    _ok(gc.check_squeeze_excite(4 * r, (4, 5, 5), 2))


@pytest.mark.parametrize('N,dims,C,K', [(2, (10, 10, 10), 64, 64), (1, (1, 3, 43), 8, 3), (2, (5, 5, 6), 64, 1)])
def test_cl_planar_at_the_rungs(N, dims, C, K):
    _ok(gc.check_cl_planar(N, dims, C, K))


def test_cl_planar_refuses_more_than_64_channels():
    from rsuper_amd.hip import ops
    src, dst = torch.zeros((2, 1000, 68), device='cuda'), torch.full((2, 4, 1000), 7.0, device='cuda')
    assert ops._L().rsuper_cl_planar(ops._ptr(src), ops._ptr(dst), 2, 1000, 68, 4, 0, ops._stream()) == 3      # RSUPER_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
