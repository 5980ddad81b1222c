"""The tuned bandwidth-bound kernels around the convolutions (csrc/unet_misc.hip, csrc/loss.hip: in_bwd_finalize2, maxpool_fwd2, the channel-split
grids of the statistics-row kernels, upsample_fwd3, the pipelined plane_partials_fwd) against the kernels they replaced, both through the C ABI
(`rsuper_glue_variant(0)` selects the previous kernels and grids).  No kernel changed which thread adds which voxel, so every output -- tensors,
statistics rows `part`, per-block loss sums -- must be equal bit for bit; outputs are pre-filled with NaN, so a voxel that is not written fails too.

Shapes: the UNet step's own (config 2: B = 2, 96^3, base 32: every level of the tail and of pooling, the four up-sampling outputs 96^3 x 64, 48^3 x 128,
24^3 x 256, 12^3 x 320), one ragged case per kernel (odd sizes, C = 8), and the f32 mode.  The trilinear backward and plane_partials_bwd kernels are
unchanged and are not compared here.  The independent anchor of this bit-for-bit chain is tests/test_gpu_glue_ref.py: the default kernels against float64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTS = {'f32': torch.float32, 'bf16': torch.bfloat16}


@pytest.fixture(scope='module', autouse=True)
def native():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X; the product path has no CPU fallback')
    from rsuper_amd.hip import lib
    lib.require_device()


def _both(run):
    """run() under the previous kernels, then under the default ones; the default is restored whatever happens."""
    from rsuper_amd.hip import ops
    L = ops._L()
    assert L.rsuper_glue_variant(-1) == 1
    try:
        assert L.rsuper_glue_variant(0) == 0
        old = run()
        torch.cuda.synchronize()
    finally:
        assert L.rsuper_glue_variant(1) == 1
    new = run()
    torch.cuda.synchronize()
    return old, new


def _assert_equal(old, new, names):
    for o, n, name in zip(old, new, names):
        assert not bool(torch.isnan(n.float()).any()), f'{name}: NaN (unwritten) in the new kernel\'s output'
        assert torch.equal(o, n), f'{name}: {int((o != n).sum())} of {o.numel()} elements differ'


def _randn(shape, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV, dtype=torch.float32).to(dt)


def _nan(shape, dt):
    return torch.full(shape, float('nan'), device=DEV, dtype=dt)


# ------------------------------------------------------------------------------------------------ InstanceNorm backward tail
IN_BWD = [  # (mode, N, vox, C, number of added gradients)
    ('bf16', 2, 96 ** 3, 32, 0), ('bf16', 2, 48 ** 3, 64, 0), ('bf16', 2, 48 ** 3, 64, 1), ('bf16', 2, 48 ** 3, 128, 2), ('bf16', 2, 24 ** 3, 128, 0),
    ('bf16', 2, 24 ** 3, 128, 1), ('bf16', 2, 24 ** 3, 256, 1), ('bf16', 2, 12 ** 3, 256, 0), ('bf16', 2, 12 ** 3, 320, 1), ('bf16', 2, 6 ** 3, 320, 0),
    ('bf16', 1, 7 * 9 * 11, 8, 1), ('bf16', 3, 37 * 41 * 43, 16, 2),
    ('f32', 2, 48 ** 3, 64, 1), ('f32', 2, 24 ** 3, 128, 0), ('f32', 1, 7 * 9 * 11, 8, 2),
    # either side of the dispatch thresholds (csrc/glue_plan.hpp): 255 | 256, 1023 | 1024, 8192 | 8193 blocks' worth of vectors; vector counts per
    # voxel that are no power of two
    ('bf16', 1, 65280, 8, 0), ('bf16', 1, 65281, 8, 1), ('bf16', 1, 261888, 8, 0), ('bf16', 1, 261889, 8, 2), ('bf16', 1, 2097152, 8, 1),
    ('bf16', 1, 2097153, 8, 0), ('bf16', 1, 48 ** 3, 24, 1), ('bf16', 1, 24 ** 3, 320, 0),
]


@pytest.mark.parametrize('mode,N,vox,C,nadd', IN_BWD)
def test_in_bwd_finalize_matches_previous_kernel(mode, N, vox, C, nadd):
    from rsuper_amd.hip import ops, lib
    dt = DTS[mode]
    g, x = _randn((N, vox, C), dt, 1), _randn((N, vox, C), dt, 2)
    adds = [_randn((N, vox, C), dt, 3 + i) for i in range(nadd)] + [None, None]
    mr = torch.stack([_randn((N, C), torch.float32, 7), _randn((N, C), torch.float32, 8).abs() + 0.5], -1).contiguous()
    gm = (_randn((N, C, 2), torch.float32, 9) * 0.1).contiguous()

    def run():
        out = _nan((N, vox, C), dt)
        lib.check(ops._L().rsuper_in_bwd_finalize(ops._DT[dt], ops._ptr(g), C, ops._ptr(x), C, ops._ptr(mr), ops._ptr(gm), ops._ptr(adds[0]), C,
                                                  ops._ptr(adds[1]), C, ops._ptr(out), C, N, vox, C, ops._stream()), 'in_bwd_finalize')
        return (out,)
    _assert_equal(*_both(run), ('dx',))


def test_in_bwd_finalize_strided_views():
    """Operands that are channel slices of wider tensors (ld > C), as the concatenated decoder inputs are."""
    from rsuper_amd.hip import ops, lib
    dt, N, vox, C, LD = torch.bfloat16, 2, 24 ** 3, 64, 128
    g, x, a = _randn((N, vox, LD), dt, 1), _randn((N, vox, LD), dt, 2), _randn((N, vox, LD), dt, 3)
    mr = torch.stack([_randn((N, C), torch.float32, 7), _randn((N, C), torch.float32, 8).abs() + 0.5], -1).contiguous()
    gm = (_randn((N, C, 2), torch.float32, 9) * 0.1).contiguous()

    def run():
        out = torch.zeros((N, vox, LD), device=DEV, dtype=dt)
        lib.check(ops._L().rsuper_in_bwd_finalize(ops._DT[dt], ops._ptr(g, 64), LD, ops._ptr(x), LD, ops._ptr(mr), ops._ptr(gm), ops._ptr(a, 64), LD,
                                                  None, 0, ops._ptr(out, 64), LD, N, vox, C, ops._stream()), 'in_bwd_finalize')
        return (out,)
    old, new = _both(run)
    _assert_equal(old, new, ('dx',))
    assert not bool(new[0][..., :64].any())                      # nothing outside the slice is written


# ------------------------------------------------------------------------------------------------ max pool / subsample
POOL = [  # (mode, N, (D, H, W), C)
    ('bf16', 2, (96, 96, 96), 32), ('bf16', 2, (48, 48, 48), 64), ('bf16', 2, (24, 24, 24), 128), ('bf16', 2, (12, 12, 12), 256),
    ('bf16', 1, (7, 9, 11), 8), ('bf16', 1, (6, 10, 14), 8), ('bf16', 3, (10, 6, 14), 320),
    ('f32', 2, (24, 24, 24), 128), ('f32', 2, (12, 12, 12), 256), ('f32', 1, (7, 9, 11), 8),
    # 1008 | 1024 statistics rows forward, 496 | 512 blocks backward; the channel split at 24^3 and 12^3
    ('bf16', 1, (126, 64, 64), 8), ('bf16', 1, (128, 64, 64), 8), ('bf16', 1, (128, 128, 62), 8), ('bf16', 1, (128, 128, 64), 8),
    ('bf16', 2, (24, 24, 24), 256), ('bf16', 2, (24, 24, 24), 320), ('bf16', 2, (12, 12, 12), 128), ('bf16', 2, (12, 12, 12), 320),
]


@pytest.mark.parametrize('mode,N,dims,C', POOL)
def test_maxpool_matches_previous_kernel(mode, N, dims, C):
    from rsuper_amd.hip import ops, lib
    dt = DTS[mode]
    D, H, W = dims
    OD, OH, OW = D // 2, H // 2, W // 2
    x = _randn((N, D, H, W, C), dt, 11)
    dy = _randn((N, OD, OH, OW, C), dt, 12)
    skip = _randn((N, D, H, W, C), dt, 13)
    blocks = ops._stat_blocks(OD * OH * OW)
    even = not ((D | H | W) & 1)

    def run():
        L = ops._L()
        y, part = _nan((N, OD, OH, OW, C), dt), _nan((N, blocks, C, 2), torch.float32)
        lib.check(L.rsuper_maxpool2_fwd(ops._DT[dt], ops._ptr(x), C, ops._ptr(y), C, ops._ptr(part), blocks, N, D, H, W, C, ops._stream()), 'maxpool2_fwd')
        dx = _nan((N, D, H, W, C), dt)
        lib.check(L.rsuper_maxpool2_bwd(ops._DT[dt], ops._ptr(x), C, ops._ptr(dy), C, ops._ptr(dx), C, N, D, H, W, C, ops._stream()), 'maxpool2_bwd')
        res = [y, part, dx]
        if even:
            dx2 = _nan((N, D, H, W, C), dt)
            lib.check(L.rsuper_maxpool2_bwd_add(ops._DT[dt], ops._ptr(x), C, ops._ptr(dy), C, ops._ptr(skip), C, ops._ptr(dx2), C, N, D, H, W, C,
                                                ops._stream()), 'maxpool2_bwd_add')
            res.append(dx2)
        return res
    _assert_equal(*_both(run), ('y', 'part', 'dx', 'dx(+skip)'))


@pytest.mark.parametrize('mode,N,dims,C', [('bf16', 2, (48, 48, 48), 64), ('bf16', 2, (24, 24, 24), 128), ('bf16', 2, (12, 12, 12), 256),
                                           ('bf16', 1, (7, 9, 11), 8), ('f32', 2, (12, 12, 12), 256), ('f32', 1, (7, 9, 11), 8),
                                           ('bf16', 2, (24, 24, 24), 256), ('bf16', 2, (24, 24, 24), 320), ('bf16', 2, (12, 12, 12), 128),
                                           ('bf16', 2, (12, 12, 12), 320)])
def test_subsample_matches_previous_kernel(mode, N, dims, C):
    from rsuper_amd.hip import ops, lib
    dt = DTS[mode]
    D, H, W = dims
    OD, OH, OW = (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    x = _randn((N, D, H, W, C), dt, 21)
    blocks = ops._stat_blocks(OD * OH * OW)

    def run():
        y, part = _nan((N, OD, OH, OW, C), dt), _nan((N, blocks, C, 2), torch.float32)
        lib.check(ops._L().rsuper_subsample2_fwd(ops._DT[dt], ops._ptr(x), C, ops._ptr(y), C, ops._ptr(part), blocks, N, D, H, W, C, ops._stream()),
                  'subsample2_fwd')
        return y, part
    _assert_equal(*_both(run), ('y', 'part'))


# ------------------------------------------------------------------------------------------------ trilinear forward
UP = [  # (mode, N, input dims, output dims, C)
    ('bf16', 2, (48, 48, 48), (96, 96, 96), 64), ('bf16', 2, (24, 24, 24), (48, 48, 48), 128), ('bf16', 2, (12, 12, 12), (24, 24, 24), 256),
    ('bf16', 2, (6, 6, 6), (12, 12, 12), 320), ('bf16', 1, (3, 5, 4), (7, 9, 11), 8), ('bf16', 1, (5, 1, 7), (5, 4, 7), 8),
    ('f32', 2, (12, 12, 12), (24, 24, 24), 256), ('f32', 2, (24, 24, 24), (48, 48, 48), 128), ('f32', 2, (6, 6, 6), (12, 12, 12), 320),
    ('f32', 1, (3, 5, 4), (7, 9, 11), 8),
    # the per-axis tables of upsample_fwd3 stop fitting 64 KB next to the statistics scratch between 3070 and 3071 outputs
    ('bf16', 1, (1, 1, 1536), (1, 1, 3070), 8), ('bf16', 1, (1, 1, 1536), (1, 1, 3071), 8),
]


@pytest.mark.parametrize('mode,N,I,O,C', UP)
def test_upsample_fwd_matches_previous_kernel(mode, N, I, O, C):
    from rsuper_amd.hip import ops, lib
    dt = DTS[mode]
    x = _randn((N,) + I + (C,), dt, 31)
    blocks = ops._stat_blocks(O[0] * O[1] * O[2])

    def run():
        y, part = _nan((N,) + O + (C,), dt), _nan((N, blocks, C, 2), torch.float32)
        lib.check(ops._L().rsuper_upsample_fwd(ops._DT[dt], ops._ptr(x), C, ops._ptr(y), C, ops._ptr(part), blocks, N, *I, *O, C, ops._stream()),
                  'upsample_fwd')
        return y, part
    _assert_equal(*_both(run), ('y', 'part'))


def test_upsample_fwd_strided_views():
    """Input a channel slice of a wider tensor, output written into one half of the concatenated decoder input (ld > C)."""
    from rsuper_amd.hip import ops, lib
    dt, N, I, O, C = torch.bfloat16, 2, (12, 12, 12), (24, 24, 24), 64
    x = _randn((N,) + I + (96,), dt, 32)
    blocks = ops._stat_blocks(24 ** 3)

    def run():
        y, part = torch.zeros((N,) + O + (128,), device=DEV, dtype=dt), _nan((N, blocks, C, 2), torch.float32)
        lib.check(ops._L().rsuper_upsample_fwd(ops._DT[dt], ops._ptr(x, 32), 96, ops._ptr(y, 64), 128, ops._ptr(part), blocks, N, *I, *O, C,
                                               ops._stream()), 'upsample_fwd')
        return y, part
    old, new = _both(run)
    _assert_equal(old, new, ('y', 'part'))
    assert not bool(new[0][..., :64].any())


# ------------------------------------------------------------------------------------------------ loss partial sums
PLANES = [  # (planes, V, label form, known-voxel mask, background mask)
    (52, 96 ** 3, 'bits', False, False), (52, 96 ** 3, 'bits', True, False), (6, 48 ** 3, 'bytes', True, True), (4, 96 ** 3, 'bytes', False, True),
    (6, 12 ** 3, 'bytes', True, True), (3, 7 * 9 * 11, 'bytes', True, False), (26, 40 * 36 * 28, 'bits', True, False),
]


@pytest.mark.parametrize('planes,V,labels,with_k,with_w2', PLANES)
def test_plane_partials_fwd_matches_previous_kernel(planes, V, labels, with_k, with_w2):
    from rsuper_amd.hip import ops, lib
    g = torch.Generator(device=DEV).manual_seed(41)
    x = torch.randn((planes, V), generator=g, device=DEV) * 3
    t = tpk = None
    tP = tC = 0
    if labels == 'bits':                                          # np.packbits along the class axis: class c of a sample is bit 7 - (c & 7) of byte plane c >> 3
        tC = 26 if planes % 26 == 0 else planes
        tP = (tC + 7) // 8
        tpk = torch.randint(0, 256, (planes // tC, tP, V), generator=g, device=DEV, dtype=torch.uint8)
    else:
        t = (torch.rand((planes, V), generator=g, device=DEV) < 0.3).to(torch.uint8)
    k = (torch.rand((planes, V), generator=g, device=DEV) < 0.8).to(torch.uint8) if with_k else None
    w2 = (torch.rand((planes, V), generator=g, device=DEV) < 0.5).to(torch.uint8) if with_w2 else None
    nb = ops._L().rsuper_plane_partials_blocks(V)

    def run():
        L = ops._L()
        pblk = torch.full((planes, nb, 6), float('nan'), device=DEV, dtype=torch.float64)
        sums = _nan((planes, 6), torch.float32)
        lib.check(L.rsuper_plane_partials_fwd3(ops._ptr(x), V, ops._ptr(t), ops._ptr(tpk), tP, tC, ops._ptr(k), None, None, ops._ptr(w2), ops._ptr(pblk), 0,
                                               planes, V, ops._stream()), 'plane_partials_fwd3')
        lib.check(L.rsuper_plane_sums_reduce(ops._ptr(pblk), planes, nb, ops._ptr(sums), ops._stream()), 'plane_sums_reduce')
        return pblk, sums
    _assert_equal(*_both(run), ('per-block sums', 'loss sums'))


def test_variant_switch_reports_and_restores():
    from rsuper_amd.hip import ops
    L = ops._L()
    assert L.rsuper_glue_variant(-1) == 1 and L.rsuper_glue_variant(7) == 1
    assert L.rsuper_glue_variant(0) == 0 and L.rsuper_glue_variant(-1) == 0
    assert L.rsuper_glue_variant(1) == 1
