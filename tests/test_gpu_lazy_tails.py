"""Lazy InstanceNorm backward tails (csrc/lazy_tail_plan.hpp): the max-pool backward and the trilinear backward take the RAW data gradient g of the block
that read their output, with the statistics and the backward means, and apply the tail dx = rstd (g - mean(g) - x_n mean(g x_n)) as they read it.
The fused kernels call the tail function of in_bwd_finalize and round as the finished tensor was rounded, so every comparison here is torch.equal
against the two-launch path of the same build: rsuper_in_bwd_finalize, then the existing pool / trilinear backward.  Outputs are pre-filled with NaN,
so a voxel that is not written fails too.

Shapes are the smallest at which the kernels can go wrong: one 16-byte vector per voxel (C = 8) and a channel count that does not divide the block
(C = 40: the per-thread constants are reloaded per vector), several blocks per sample, gradients that are channel slices of a wider tensor, ties
inside a 2x2x2 cell, an odd size and a non-doubling scale (both must give the fall-back's result).  f32 runs with C = 8: every entry of the library,
rsuper_in_bwd_finalize included, refuses a channel count that is no multiple of 8 (a single f32 vector, C = 4, has no two-launch result to compare
with; the refusal is asserted)."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTS = {'f32': torch.float32, 'bf16': torch.bfloat16}


@pytest.fixture(scope='module', autouse=True)
def native():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X; the product path has no CPU fallback')
    from rsuper_amd.hip import lib
    lib.require_device()


@pytest.fixture
def variant():
    """Set rsuper_lazy_tails for the test; the default is restored whatever happens."""
    from rsuper_amd.hip import ops
    L = ops._L()
    assert L.rsuper_lazy_tails(-1) == 1
    yield L.rsuper_lazy_tails
    assert L.rsuper_lazy_tails(1) == 1


def _randn(shape, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV, dtype=torch.float32).to(dt)


def _nan(shape, dt):
    return torch.full(shape, float('nan'), device=DEV, dtype=dt)


def _tables(N, C, seed):
    """(mean, rstd) and backward means of the size a real step has."""
    mr = torch.stack([_randn((N, C), torch.float32, seed), _randn((N, C), torch.float32, seed + 1).abs() + 0.5], -1).contiguous()
    return mr, (_randn((N, C, 2), torch.float32, seed + 2) * 0.1).contiguous()


def _grad(shape, dt, seed, wide):
    """A gradient tensor of `shape`; wide: the channel slice [8 : 8 + C] of a tensor with C + 24 channels per voxel (what the joint data gradient of a
    two-source block hands over)."""
    if not wide:
        return _randn(shape, dt, seed)
    C = shape[-1]
    return _randn((*shape[:-1], C + 24), dt, seed)[..., 8:8 + C]


def _finalize(g, x, mr, gm):
    """The finished gradient by its own launch (the reference of every comparison)."""
    from rsuper_amd.hip import ops
    return ops.in_bwd_finalize(ops.Src(g.contiguous()), ops.Src(x, mr=mr), gm, g.shape[-1])


def _assert_equal(ref, got, name):
    assert not bool(torch.isnan(got.float()).any()), f'{name}: NaN (unwritten) in the fused kernel\'s output'
    assert torch.equal(ref, got), f'{name}: {int((ref != got).sum())} of {ref.numel()} elements differ'


# ------------------------------------------------------------------------------------------------ max pool, C entry
def _pool_input(N, dims, C, dt, ties):
    if ties:                                                     # three distinct values: most 2x2x2 cells hold their maximum several times
        g = torch.Generator(device=DEV).manual_seed(5)
        return torch.randint(0, 3, (N, *dims, C), generator=g, device=DEV).to(dt) - 1
    return _randn((N, *dims, C), dt, 11)


@pytest.mark.parametrize('lazy', [(True, False), (False, True), (True, True), (False, False)], ids=['add', 'dy', 'both', 'neither'])
@pytest.mark.parametrize('mode,C,wide,ties', [('bf16', 8, False, False), ('bf16', 40, False, False), ('bf16', 40, True, False), ('bf16', 8, False, True),
                                              ('f32', 8, False, False), ('f32', 8, True, True)])
def test_maxpool_backward_with_lazy_gradients_equals_the_two_launches(mode, C, wide, ties, lazy):
    from rsuper_amd.hip import ops, lib
    lazy_add, lazy_dy = lazy
    dt, N, dims = DTS[mode], 2, (4, 4, 6)
    D, H, W = dims
    x = _pool_input(N, dims, C, dt, ties)
    y, mry = ops._maxpool_fwd(x)
    (mrx, gmx), (_, gmy) = _tables(N, C, 20), _tables(N, C, 30)
    gy, ga = _grad(tuple(y.shape), dt, 12, wide), _grad(tuple(x.shape), dt, 13, wide)
    L, st = ops._L(), ops._stream()
    dy = _finalize(gy, y, mry, gmy) if lazy_dy else gy.contiguous()
    add = _finalize(ga, x, mrx, gmx) if lazy_add else ga.contiguous()
    ref = _nan(tuple(x.shape), dt)
    lib.check(L.rsuper_maxpool2_bwd_add(ops._DT[dt], ops._ptr(x), C, ops._ptr(dy), C, ops._ptr(add), C, ops._ptr(ref), C, N, D, H, W, C, st), 'maxpool2_bwd_add')
    got = _nan(tuple(x.shape), dt)
    assert gy.stride(3) == (C + 24 if wide else C)
    lib.check(L.rsuper_maxpool2_bwd_lazy(ops._DT[dt], ops._ptr(x), C, gy.data_ptr(), gy.stride(3), ops._ptr(mry), ops._ptr(gmy) if lazy_dy else None,
                                         ga.data_ptr(), ga.stride(3), ops._ptr(mrx), ops._ptr(gmx) if lazy_add else None, ops._ptr(got), C,
                                         N, D, H, W, C, st), 'maxpool2_bwd_lazy')
    torch.cuda.synchronize()
    _assert_equal(ref, got, 'dx')
    if ties:                                                     # the first maximum of a cell takes the pooled gradient: with the skip gradient zero, one voxel per cell
        z = torch.zeros_like(x)
        lib.check(L.rsuper_maxpool2_bwd_lazy(ops._DT[dt], ops._ptr(x), C, gy.data_ptr(), gy.stride(3), ops._ptr(mry), ops._ptr(gmy) if lazy_dy else None,
                                             ops._ptr(z), C, None, None, ops._ptr(got), C, N, D, H, W, C, st), 'maxpool2_bwd_lazy')
        cells = got.view(N, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, D // 2, H // 2, W // 2, C, 8)
        xc = x.view(N, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, D // 2, H // 2, W // 2, C, 8).float()
        first = (xc == xc.max(-1, keepdim=True).values).float().argmax(-1, keepdim=True)
        want = torch.zeros_like(cells).scatter_(-1, first, dy.unsqueeze(-1))
        assert torch.equal(cells, want)


def test_lazy_entries_refuse_what_the_two_launches_refuse():
    """Odd sizes, a single f32 vector per voxel (C = 4) and the f32 trilinear backward are not taken by the fused entries: UNSUPPORTED (3) sends the caller
    to the two launches, a channel count no entry of the library takes is an argument error (1) as in rsuper_in_bwd_finalize."""
    from rsuper_amd.hip import ops, lib
    L, st = ops._L(), ops._stream()
    t = torch.zeros(2 * 5 * 4 * 6 * 8, device=DEV, dtype=torch.float32)
    tab = torch.ones((2, 8, 2), device=DEV)
    p = t.data_ptr()
    assert L.rsuper_maxpool2_bwd_lazy(lib.BF16, p, 8, p, 8, tab.data_ptr(), tab.data_ptr(), p, 8, tab.data_ptr(), tab.data_ptr(), p, 8, 2, 5, 4, 6, 8, st) == 3
    assert L.rsuper_maxpool2_bwd_lazy(lib.F32, p, 4, p, 4, tab.data_ptr(), tab.data_ptr(), p, 4, tab.data_ptr(), tab.data_ptr(), p, 4, 2, 4, 4, 6, 4, st) == 1
    assert L.rsuper_in_bwd_finalize(lib.F32, p, 4, p, 4, tab.data_ptr(), tab.data_ptr(), None, 0, None, 0, p, 4, 2, 96, 4, st) == 1
    assert L.rsuper_upsample_bwd_lazy(lib.F32, p, 8, p, 8, tab.data_ptr(), tab.data_ptr(), p, 8, 2, 3, 3, 4, 6, 6, 8, 8, st) == 3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ max pool, autograd node
@pytest.mark.parametrize('dims,have', [((5, 4, 6), 'both'), ((4, 4, 6), 'dy'), ((4, 4, 6), 'skip'), ((4, 4, 6), 'both')])
def test_maxpool_skip_lazy_node_falls_back_to_the_finished_gradients(dims, have):
    """MaxPoolSkipLazyFn.backward on an odd size (the fused entry refuses it) and with one gradient missing: the gradients are finalised by their own
    launches and take MaxPoolSkipFn's path."""
    from rsuper_amd.hip import ops
    dt, N, C = torch.bfloat16, 2, 8
    x = _randn((N, *dims, C), dt, 11).requires_grad_()
    (mrx, gmx), (_, gmy) = _tables(N, C, 20), _tables(N, C, 30)
    y, mry, skip, mrs = ops.MaxPoolSkipLazyFn.apply(x, mrx)
    assert mry.requires_grad and mrs.requires_grad and torch.equal(mrs, mrx) and torch.equal(skip, x)
    gy, ga = _randn(tuple(y.shape), dt, 12), _randn(tuple(x.shape), dt, 13)
    outs, grads = [], []
    if have in ('both', 'dy'):
        outs += [y, mry]; grads += [gy, gmy]
    if have in ('both', 'skip'):
        outs += [skip, mrs]; grads += [ga, gmx]
    torch.autograd.backward(outs, grads)
    ref = None
    if have in ('both', 'dy'):
        ref = ops._maxpool_bwd(x.detach(), _finalize(gy, y.detach(), mry.detach(), gmy))
    if have in ('both', 'skip'):
        fa = _finalize(ga, x.detach(), mrx, gmx)
        ref = fa if ref is None else ref + fa
    torch.cuda.synchronize()
    _assert_equal(ref, x.grad, 'dx')


# ------------------------------------------------------------------------------------------------ trilinear
UP = [  # (I, O, C, wide)
    ((3, 3, 4), (6, 6, 8), 8, False), ((3, 3, 4), (6, 6, 8), 64, False), ((3, 3, 4), (6, 6, 8), 64, True),
    ((3, 4, 5), (5, 7, 9), 8, False), ((3, 4, 5), (5, 7, 9), 64, True), ((6, 6, 6), (12, 12, 12), 320, False),
]


@pytest.mark.parametrize('I,O,C,wide', UP)
def test_trilinear_backward_with_a_lazy_gradient_equals_the_two_launches(I, O, C, wide, variant):
    """rsuper_lazy_tails(2): the fused kernel wherever it can take the launch, whatever the plan's per-shape rule says."""
    from rsuper_amd.hip import ops, lib
    assert variant(2) == 2
    dt, N = torch.bfloat16, 2
    x = _randn((N, *I, C), dt, 3)
    u, mru = ops._upsample_fwd(x, O)
    _, gm = _tables(N, C, 40)
    g = _grad(tuple(u.shape), dt, 14, wide)
    ref = ops._upsample_bwd(tuple(x.shape), _finalize(g, u, mru, gm))
    got = _nan(tuple(x.shape), dt)
    rc = ops._L().rsuper_upsample_bwd_lazy(ops._DT[dt], g.data_ptr(), g.stride(3), ops._ptr(u), C, ops._ptr(mru), ops._ptr(gm), ops._ptr(got), C,
                                           N, *I, *O, C, ops._stream())
    lib.check(rc, 'upsample_bwd_lazy')
    torch.cuda.synchronize()
    _assert_equal(ref, got, 'dx')


@pytest.mark.parametrize('mode,I,O', [('f32', (3, 3, 4), (6, 6, 8)), ('bf16', (3, 4, 5), (5, 7, 9)), ('bf16', (3, 3, 3), (9, 9, 9))])
def test_upsample_lazy_node_equals_the_two_launches(mode, I, O, variant):
    """UpsampleLazyFn.backward with and without means: f32 and a scale past the row-sharing kernel's tables (3 -> 9) finalise first."""
    from rsuper_amd.hip import ops
    assert variant(2) == 2
    dt, N, C = DTS[mode], 2, 8
    x = _randn((N, *I, C), dt, 3).requires_grad_()
    u, mru = ops.UpsampleLazyFn.apply(x, O)
    assert mru.requires_grad
    _, gm = _tables(N, C, 40)
    g = _randn(tuple(u.shape), dt, 14)
    torch.autograd.backward([u, mru], [g, gm], retain_graph=True)
    ref = ops._upsample_bwd(tuple(x.shape), _finalize(g, u.detach(), mru.detach(), gm))
    torch.cuda.synchronize()
    _assert_equal(ref, x.grad, 'dx (lazy)')
    x.grad = None
    torch.autograd.backward([u], [g])                            # no means: g is a finished gradient
    ref = ops._upsample_bwd(tuple(x.shape), g)
    torch.cuda.synchronize()
    _assert_equal(ref, x.grad, 'dx (finished)')


# ------------------------------------------------------------------------------------------------ blocks
def _pair(pool, dt):
    from rsuper_amd.model.dim3.unet_utils import down_block, up_block
    torch.manual_seed(0)
    down, up = down_block(32, 64, 2, pool=pool).to(DEV), up_block(64, 32, 2).to(DEV)
    return down, up


def _pair_grads(down, up, x, mr, w):
    for p in list(down.parameters()) + list(up.parameters()):
        p.grad = None
    x = x.detach().requires_grad_()
    x2, m2, skip, ms = down(x, mr, True, True)
    o, _ = up(x2, m2, skip, ms)
    (o.float() * w).sum().backward()
    torch.cuda.synchronize()
    return [x.grad] + [p.grad.clone() for p in list(down.parameters()) + list(up.parameters())]


@pytest.mark.parametrize('mode,pool', [('bf16', True), ('f32', True), ('bf16', False)])
def test_down_up_pair_gradients_equal_the_eager_tails(mode, pool, variant):
    """down_block(32 -> 64) + up_block(64 -> 32) at 8^3, N = 2: the input gradient and every parameter gradient with lazy tails (the plan's choice, and
    everywhere the kernels can take them) against every tail as its own launch.  pool=False: the skip has no pooling node and stays eager."""
    from rsuper_amd.hip import ops
    dt, N, S = DTS[mode], 2, 8
    down, up = _pair(pool, dt)
    x = _randn((N, S, S, S, 32), dt, 1)
    xf = x.float().view(N, -1, 32)
    mr = torch.stack([xf.mean(1), 1.0 / torch.sqrt(xf.var(1, unbiased=False) + 1e-4)], -1).contiguous()
    w = _randn((N, S, S, S, 32), torch.float32, 2)
    assert variant(0) == 0
    eager = _pair_grads(down, up, x, mr, w)
    for v in (1, 2):
        assert variant(v) == v
        assert ops.maxpool_lazy_plan(x) == (v > 0)
        lazy = _pair_grads(down, up, x, mr, w)
        assert len(lazy) == len(eager) >= 9                      # the input and at least two weights per block
        for i, (a, b) in enumerate(zip(eager, lazy)):
            _assert_equal(a, b, f'variant {v}, gradient {i}')


class _PairNet(nn.Module):
    """stem + down_block + up_block + head: the smallest network GraphedNetwork can hold that has a pooling layer with a skip and an up-sampling."""

    def __init__(self):
        super().__init__()
        from rsuper_amd.model.dim3.unet_utils import inconv, down_block, up_block
        self.inc, self.down, self.up = inconv(1, 32), down_block(32, 64, 2), up_block(64, 32, 2)
        self.outc = nn.Conv3d(32, 3, kernel_size=1)

    def forward(self, img):
        from rsuper_amd.hip import ops
        x1, m1 = self.inc(img, torch.bfloat16)
        x2, m2, x1, s1 = self.down(x1, m1, True, True)
        o, _ = self.up(x2, m2, x1, s1)
        return {'segmentation': ops.HeadFn.apply(o, self.outc.weight, self.outc.bias)}


def test_lazy_tails_under_graphed_network(variant):
    """The pair under GraphedNetwork (forward and backward replayed from two hipGraphs): parameter gradients of three replays with lazy tails equal the
    eager module's with every tail as its own launch."""
    from rsuper_amd.graph import GraphedNetwork
    torch.manual_seed(0)
    net = _PairNet().to(DEV).train()
    img = _randn((2, 1, 8, 8, 8), torch.float32, 4)
    w = _randn((2, 3, 8, 8, 8), torch.float32, 5)

    def grads(f):
        for p in net.parameters():
            p.grad = None
        (f(img)['segmentation'].float() * w).sum().backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in net.parameters()]
    assert variant(0) == 0
    eager = grads(net)
    assert variant(2) == 2
    g = GraphedNetwork(net, warmup=1)
    for step in range(3):
        for i, (a, b) in enumerate(zip(eager, grads(g))):
            _assert_equal(a, b, f'replay {step}, gradient {i}')
