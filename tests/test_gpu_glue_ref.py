"""The bandwidth-bound kernels between the convolutions (csrc/unet_misc.hip: in_bwd_finalize{,2}, maxpool_fwd{,2} / maxpool_bwd, subsample_fwd / bwd,
upsample_fwd{,2,3} / upsample_bwd{,2,4}; csrc/loss.hip: plane_partials_fwd with byte and bit-packed labels) against the float64 references of
tests/glue_ref.py, each held to the bound derived there (selection results bit-exact; sums of two values, tails and trilinear results one storage rounding
plus a counted number of f32 roundings; statistics rows exact on integer-valued inputs, 1e-4 of the column's rms otherwise; plane sums the f32 evaluation of
softplus / sigmoid per voxel).  tests/test_glue_ref_cpu.py proves the references and shows that the bounds bite.  This is the independent anchor of the
bit-for-bit chains of tests/test_gpu_glue_kernels.py (tuned kernels == the ones they replaced) and tests/test_gpu_lazy_tails.py (fused tails == two launches).

Every case calls the C entry points with outputs pre-filled with NaN (an unwritten element fails), asserts from rsuper_glue_plan WHICH kernel, selector and
channel split its shape gets (the tables of glue_ref.py; a dispatch change must move the shape, not the assertion), and prints its worst ratio per output;
RSUPER_GLUE_REF_TABLE names a file to collect the lines in (profiles/glue_ref.txt was measured this way).  The small cases also go through the autograd
wrappers of hip/ops.py (MaxPoolFn, MaxPoolSkipFn, UpsampleFn, subsample2, in_bwd_finalize), which must hand back the same bits.

Not covered, on purpose: shapes at or beyond 2^31 elements -- the first-generation trilinear kernels (upsample_fwd_kernel, upsample_bwd_kernel) run only
beyond 32-bit offsets, which no small tensor reaches (tests/test_glue_plan_cpu.py pins those rungs of the plan); NaN inputs (fmaxf and ATen differ by
design); stem and head; the lazy-tail kernels (bit-identical to the two launches pinned here).  The alternative of RSUPER_UPSAMPLE_BWD4 (the gather kernel
for bf16) is reached through the plan by a scale the row-sharing kernel's tables do not hold: case `gather`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def native():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X; the product path has no CPU fallback')
    from rsuper_amd.hip import lib, ops
    lib.require_device()
    assert ops._L().rsuper_glue_variant(-1) == 1


def _report(label, ratios, facts=''):
    line = f'{label}: ' + ' '.join(f'{k} {v:.3f}' if v >= 1e-3 or v == 0 else f'{k} {v:.0e}' for k, v in ratios.items()) + f' | {facts}'
    print(line)
    table = os.environ.get('RSUPER_GLUE_REF_TABLE')
    if table:
        with open(table, 'a') as f:
            f.write(line + '\n')
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f'over the bound: {bad} -- {line}'


def _nan(shape, dt):
    return torch.full(shape, float('nan'), device=DEV, dtype=dt)


def _exact(got, ref):
    """0 if the device tensor equals the float64 reference element for element (NaN never does), else inf: a `ratio` for selection results"""
    return 0.0 if torch.equal(got.detach().cpu().double(), ref) else float('inf')


def _c(name, *a):
    from rsuper_amd.hip import ops, lib
    lib.check(getattr(ops._L(), name)(*a, ops._stream()), name)


def _rows_ratios(part, cnt, y_stored, exact):
    """The statistics rows a forward wrote: on integer-valued inputs their float64 sum equals the integer sums; otherwise finalised (mean, rstd) against
    float64 sums over the stored output.  The finalised table is returned too."""
    from rsuper_amd.hip import ops
    fin = ops.stats_finalize(part, cnt)
    torch.cuda.synchronize()
    if exact:
        return {'rows': 0.0 if torch.equal(R.part_sums(part.cpu()), R.stat_sums_exact(y_stored)) else float('inf')}, fin
    m, r = R.stats_ratio(fin.cpu(), y_stored)
    return {'mean': m, 'rstd': r}, fin


# ================================================================================================ InstanceNorm backward tail
def _tail_tables(N, C):
    gen = torch.Generator().manual_seed(7)
    mr = torch.stack([torch.randn((N, C), generator=gen), torch.randn((N, C), generator=gen).abs() + 0.5], -1).contiguous()
    gm = (torch.randn((N, C, 2), generator=gen) * 0.1).contiguous()
    return mr, gm


@pytest.mark.parametrize('case', R.TAIL_CASES, ids=[c[0] for c in R.TAIL_CASES])
def test_norm_tail(case):
    from rsuper_amd.hip import ops
    name, mode, N, vox, C, nadd, kernel, sel = case
    p = R.glue_plan('in_bwd', mode, N, [vox], C)
    assert (p['kernel'], p['sel']) == (kernel, sel), p
    dt = R.DTYPES[mode]
    g, x = R.stored(1, (N, vox, C), mode), R.stored(2, (N, vox, C), mode)
    adds = [R.stored(3 + i, (N, vox, C), mode) for i in range(nadd)]
    mr, gm = _tail_tables(N, C)
    gd, xd, mrd, gmd = g.to(DEV), x.to(DEV), mr.to(DEV), gm.to(DEV)
    ad = [a.to(DEV) for a in adds] + [None, None]
    out = _nan((N, vox, C), dt)
    _c('rsuper_in_bwd_finalize', ops._DT[dt], ops._ptr(gd), C, ops._ptr(xd), C, ops._ptr(mrd), ops._ptr(gmd), ops._ptr(ad[0]), C, ops._ptr(ad[1]), C,
       ops._ptr(out), C, N, vox, C)
    torch.cuda.synchronize()
    ref, mag = R.in_bwd_tail(g, x, mr, gm, adds)
    ratios = {'dx': R.tail_ratio(out.cpu(), ref, mag, mode)}
    if nadd <= 1:                                                # the wrapper takes one added gradient
        shape5 = (N, 1, 1, vox, C)
        w = ops.in_bwd_finalize(ops.Src(gd.view(shape5)), ops.Src(xd.view(shape5), mr=mrd), gmd, C, add1=ad[0].view(shape5) if nadd else None)
        ratios['wrapper'] = 0.0 if torch.equal(w.view(N, vox, C), out) else float('inf')
    _report(f'tail {name} {mode} {N}x{vox}x{C} +{nadd}', ratios, f"{p['kernel']} U={p['sel']} grid {p['bx']}")


def test_norm_tail_strided_views():
    """Operands that are channel slices of wider tensors (ld 128, C 64, offset 64): the bound inside the slice, no write outside it."""
    from rsuper_amd.hip import ops
    mode, N, vox, C, LD, OFF = 'bf16', 2, 8161, 64, 128, 64
    p = R.glue_plan('in_bwd', mode, N, [vox], C, ld=LD)
    assert (p['kernel'], p['sel']) == ('in_bwd_finalize2_kernel', 2), p
    dt = R.DTYPES[mode]
    g, x, a = (R.stored(s, (N, vox, LD), mode) for s in (1, 2, 3))
    mr, gm = _tail_tables(N, C)
    gd, xd, adv, mrd, gmd = g.to(DEV), x.to(DEV), a.to(DEV), mr.to(DEV), gm.to(DEV)
    out = _nan((N, vox, LD), dt)
    out[..., :OFF] = 0
    _c('rsuper_in_bwd_finalize', ops._DT[dt], ops._ptr(gd, OFF), LD, ops._ptr(xd), LD, ops._ptr(mrd), ops._ptr(gmd), ops._ptr(adv, OFF), LD, None, 0,
       ops._ptr(out, OFF), LD, N, vox, C)
    torch.cuda.synchronize()
    ref, mag = R.in_bwd_tail(g[..., OFF:], x[..., :C], mr, gm, [a[..., OFF:]])
    assert not bool(out[..., :OFF].any())                        # nothing outside the slice is written
    _report(f'tail strided {mode} {N}x{vox}x{C} ld {LD}', {'dx': R.tail_ratio(out[..., OFF:].cpu(), ref, mag, mode)}, f"{p['kernel']} U={p['sel']}")


# ================================================================================================ max pool
def _pool_run(mode, x, dy, add):
    """y, part, dx, dx(+add) of the C entry points on CPU-made stored tensors; odd sizes take the wrapper's two steps for dx + add"""
    from rsuper_amd.hip import ops
    dt = R.DTYPES[mode]
    N, D, H, W, C = x.shape
    OD, OH, OW = D // 2, H // 2, W // 2
    xd, dyd, addd = x.to(DEV), dy.to(DEV), add.to(DEV)
    blocks = ops._stat_blocks(OD * OH * OW)
    y, part = _nan((N, OD, OH, OW, C), dt), _nan((N, blocks, C, 2), torch.float32)
    _c('rsuper_maxpool2_fwd', ops._DT[dt], ops._ptr(xd), C, ops._ptr(y), C, ops._ptr(part), blocks, N, D, H, W, C)
    dx = _nan((N, D, H, W, C), dt)
    _c('rsuper_maxpool2_bwd', ops._DT[dt], ops._ptr(xd), C, ops._ptr(dyd), C, ops._ptr(dx), C, N, D, H, W, C)
    if (D | H | W) & 1:
        dx2 = ops._maxpool_bwd_add(xd, dyd, addd)
    else:
        dx2 = _nan((N, D, H, W, C), dt)
        _c('rsuper_maxpool2_bwd_add', ops._DT[dt], ops._ptr(xd), C, ops._ptr(dyd), C, ops._ptr(addd), C, ops._ptr(dx2), C, N, D, H, W, C)
    torch.cuda.synchronize()
    return xd, dyd, addd, y, part, dx, dx2


def _pool_judge(mode, kind, x, dy, add, y, part, dx, dx2):
    yref = R.maxpool_fwd(x)
    r = {'y': _exact(y, yref)}
    rows, fin = _rows_ratios(part, yref[0, ..., 0].numel(), yref, exact=kind == 'ints')
    r.update(rows)
    dref, _ = R.maxpool_bwd(x, dy)
    r['dx'] = _exact(dx, dref)
    aref, amag = R.maxpool_bwd(x, dy, add)
    r['dx+add'] = R.rounded_sum_ratio(dx2.cpu(), aref, amag, mode)
    return r, fin


@pytest.mark.parametrize('kind', ['ints', 'gauss'])
@pytest.mark.parametrize('case', R.POOL_CASES, ids=[c[0] for c in R.POOL_CASES])
def test_maxpool(case, kind):
    """ints: integer-valued input (exact statistics rows, and every window full of ties); gauss: the general case"""
    name, mode, N, dims, C, kernel, z, bthreads = case
    p, q = R.glue_plan('pool_fwd', mode, N, dims, C), R.glue_plan('pool_bwd', mode, N, dims, C)
    assert (p['kernel'], p['bz'], q['kernel'], q['threads']) == (kernel, z, 'maxpool_bwd_kernel', bthreads), (p, q)
    O = tuple(d // 2 for d in dims)
    x, dy, add = R.stored(11, (N,) + dims + (C,), mode, kind), R.stored(12, (N,) + O + (C,), mode), R.stored(13, (N,) + dims + (C,), mode)
    xd, dyd, addd, y, part, dx, dx2 = _pool_run(mode, x, dy, add)
    r, fin = _pool_judge(mode, kind, x, dy, add, y, part, dx, dx2)
    if x.numel() < 1 << 16:                                      # the autograd wrappers hand back the same bits
        from rsuper_amd.hip import ops
        xa = xd.clone().requires_grad_(True)
        ya, mra = ops.MaxPoolFn.apply(xa)
        ya.backward(dyd)
        xb = xd.clone().requires_grad_(True)
        yb, mrb, skip = ops.MaxPoolSkipFn.apply(xb)
        torch.autograd.backward([yb, skip], [dyd, addd])
        torch.cuda.synchronize()
        same = torch.equal(ya, y) and torch.equal(yb, y) and torch.equal(mra, fin) and torch.equal(mrb, fin) and torch.equal(xa.grad, dx) and \
            torch.equal(xb.grad, dx2)
        r['wrappers'] = 0.0 if same else float('inf')
    _report(f'maxpool {name} {kind} {mode} {N}x{dims}x{C}', r, f"{p['kernel']} z={p['bz']} rows {p['rows']}; bwd {q['threads']} threads x {q['bx']}")


def test_maxpool_ties():
    """bf16 values drawn from five levels: most windows hold their maximum more than once, and the gradient goes to the first in (d, h, w) order"""
    mode, N, dims, C = 'bf16', 1, (6, 10, 14), 8
    x, dy, add = R.stored(14, (N,) + dims + (C,), mode, 'levels'), R.stored(15, (N, 3, 5, 7, C), mode), R.stored(16, (N,) + dims + (C,), mode)
    w = R._windows(x.double())
    assert ((w == w.max(-1, keepdim=True).values).sum(-1) > 1).double().mean().item() > 0.5
    assert not torch.equal(R.maxpool_bwd(x, dy)[0], R.maxpool_bwd(x, dy, last=True)[0])
    _, _, _, y, part, dx, dx2 = _pool_run(mode, x, dy, add)
    r, _ = _pool_judge(mode, 'levels', x, dy, add, y, part, dx, dx2)
    _report(f'maxpool ties {mode} {N}x{dims}x{C}', r)


# ================================================================================================ stride-2 subsample
@pytest.mark.parametrize('kind', ['ints', 'gauss'])
@pytest.mark.parametrize('case', R.SUB_CASES, ids=[c[0] for c in R.SUB_CASES])
def test_subsample(case, kind):
    from rsuper_amd.hip import ops
    name, mode, N, dims, C, z = case
    p, q = R.glue_plan('sub_fwd', mode, N, dims, C), R.glue_plan('sub_bwd', mode, N, dims, C)
    assert (p['kernel'], p['bz'], q['kernel']) == ('subsample_fwd_kernel', z, 'subsample_bwd_kernel'), (p, q)
    dt = R.DTYPES[mode]
    D, H, W = dims
    O = tuple((d + 1) // 2 for d in dims)
    x, dy = R.stored(21, (N,) + dims + (C,), mode, kind), R.stored(22, (N,) + O + (C,), mode)
    xd, dyd = x.to(DEV), dy.to(DEV)
    blocks = ops._stat_blocks(O[0] * O[1] * O[2])
    y, part = _nan((N,) + O + (C,), dt), _nan((N, blocks, C, 2), torch.float32)
    _c('rsuper_subsample2_fwd', ops._DT[dt], ops._ptr(xd), C, ops._ptr(y), C, ops._ptr(part), blocks, N, D, H, W, C)
    dx = _nan((N,) + dims + (C,), dt)
    _c('rsuper_subsample2_bwd', ops._DT[dt], ops._ptr(dyd), C, ops._ptr(dx), C, N, D, H, W, C)
    torch.cuda.synchronize()
    yref = R.subsample_fwd(x)
    r = {'y': _exact(y, yref)}
    rows, fin = _rows_ratios(part, O[0] * O[1] * O[2], yref, exact=kind == 'ints')
    r.update(rows)
    r['dx'] = _exact(dx, R.subsample_bwd(dy, dims))
    if x.numel() < 1 << 16:
        yw, mrw = ops.subsample2(xd)
        wide = torch.zeros((N,) + dims + (2 * C,), device=DEV, dtype=dt)
        ops.subsample2_scatter(dyd, wide, C, (N,) + dims)
        torch.cuda.synchronize()
        same = torch.equal(yw, y) and torch.equal(mrw, fin) and torch.equal(wide[..., C:], dx) and not bool(wide[..., :C].any())
        r['wrappers'] = 0.0 if same else float('inf')
    _report(f'subsample {name} {kind} {mode} {N}x{dims}x{C}', r, f"{p['kernel']} z={p['bz']} rows {p['rows']}")


# ================================================================================================ trilinear forward
def _up_fwd(mode, xd, ldx, xoff, y, ldy, yoff, N, I, O, C):
    from rsuper_amd.hip import ops
    blocks = ops._stat_blocks(O[0] * O[1] * O[2])
    part = _nan((N, blocks, C, 2), torch.float32)
    _c('rsuper_upsample_fwd', ops._DT[R.DTYPES[mode]], ops._ptr(xd, xoff), ldx, ops._ptr(y, yoff), ldy, ops._ptr(part), blocks, N, *I, *O, C)
    torch.cuda.synchronize()
    return part


@pytest.mark.parametrize('case', R.UP_FWD_CASES, ids=[c[0] for c in R.UP_FWD_CASES])
def test_trilinear_forward(case):
    from rsuper_amd.hip import ops
    name, mode, N, I, O, C, kernel, z = case
    p = R.glue_plan('up_fwd', mode, N, I + O, C)
    assert (p['kernel'], p['bz']) == (kernel, z), p
    dt = R.DTYPES[mode]
    x = R.stored(31, (N,) + I + (C,), mode)
    xd = x.to(DEV)
    y = _nan((N,) + O + (C,), dt)
    part = _up_fwd(mode, xd, C, 0, y, C, 0, N, I, O, C)
    ref, mag = R.trilinear_fwd(x, O)
    r = {'y': R.up_fwd_ratio(y.cpu(), ref, mag, I, mode)}
    rows, fin = _rows_ratios(part, O[0] * O[1] * O[2], y.cpu().double(), exact=False)      # against the STORED output
    r.update(rows)
    if x.numel() < 1 << 16:
        yw, mrw = ops.UpsampleFn.apply(xd.clone().requires_grad_(True), O)
        torch.cuda.synchronize()
        r['wrapper'] = 0.0 if torch.equal(yw, y) and torch.equal(mrw, fin) else float('inf')
    _report(f'up_fwd {name} {mode} {N}x{I}->{O}x{C}', r, f"{p['kernel']} z={p['bz']} rows {p['rows']} c={R.up_fwd_c(I)}")


def test_trilinear_forward_strided_views():
    """Input a channel slice of a wider tensor (ld 96 at channel 32), output one half of the concatenated decoder input (ld 128 at channel 64)."""
    name, mode, N, I, O, C, kernel = R.UP_FWD_STRIDED
    p = R.glue_plan('up_fwd', mode, N, I + O, C, ld=96)
    assert p['kernel'] == kernel, p
    x = R.stored(32, (N,) + I + (96,), mode)
    y = _nan((N,) + O + (128,), R.DTYPES[mode])
    y[..., :64] = 0
    part = _up_fwd(mode, x.to(DEV), 96, 32, y, 128, 64, N, I, O, C)
    ref, mag = R.trilinear_fwd(x[..., 32:], O)
    assert not bool(y[..., :64].any())
    r = {'y': R.up_fwd_ratio(y[..., 64:].cpu(), ref, mag, I, mode)}
    r.update(_rows_ratios(part, O[0] * O[1] * O[2], y[..., 64:].cpu().double(), exact=False)[0])
    _report(f'up_fwd {name} {mode} {N}x{I}->{O}x{C}', r, f"{p['kernel']} z={p['bz']}")


# ================================================================================================ trilinear backward
@pytest.mark.parametrize('case', R.UP_BWD_CASES, ids=[c[0] for c in R.UP_BWD_CASES])
def test_trilinear_backward(case):
    from rsuper_amd.hip import ops
    name, mode, N, I, O, C, kernel, nt = case
    p = R.glue_plan('up_bwd', mode, N, I + O, C)
    assert (p['kernel'], p['sel']) == (kernel, nt), p
    dt = R.DTYPES[mode]
    dy = R.stored(33, (N,) + O + (C,), mode)
    dyd = dy.to(DEV)
    dx = _nan((N,) + I + (C,), dt)
    _c('rsuper_upsample_bwd', ops._DT[dt], ops._ptr(dyd), C, ops._ptr(dx), C, N, *I, *O, C)
    torch.cuda.synchronize()
    ref, mw, ms, K = R.trilinear_bwd(dy, I)
    r = {'dx': R.up_bwd_ratio(dx.cpu(), ref, mw, ms, K, I, mode)}
    xw = torch.zeros((N,) + I + (C,), device=DEV, dtype=dt).requires_grad_(True)
    yw, _ = ops.UpsampleFn.apply(xw, O)
    yw.backward(dyd)
    torch.cuda.synchronize()
    r['wrapper'] = 0.0 if torch.equal(xw.grad, dx) else float('inf')
    _report(f'up_bwd {name} {mode} {N}x{O}->{I}x{C}', r, f"{p['kernel']} NT={p['sel']} K={K}")


def test_trilinear_backward_reaches_both_tile_widths_and_the_gather_kernel():
    assert {(c[6], c[7]) for c in R.UP_BWD_CASES if c[1] == 'bf16'} == {('upsample_bwd4_kernel', 4), ('upsample_bwd4_kernel', 6), ('upsample_bwd2_kernel', 0)}


# ================================================================================================ loss plane sums
@pytest.mark.parametrize('case', R.PLANE_CASES, ids=[c[0] for c in R.PLANE_CASES])
def test_plane_sums(case):
    from rsuper_amd.hip import ops
    name, planes, V, labels, with_k, with_w2 = case
    g = np.random.default_rng(41)
    x = (g.standard_normal((planes, V)) * 3).astype(np.float32)
    t = tpk = None
    tP = tC = 0
    if labels == 'bits':                                          # np.packbits along the class axis, as the dataset stores the labels
        tC = 26 if planes % 26 == 0 else planes
        tP = (tC + 7) // 8
        tpk = g.integers(0, 256, (planes // tC, tP, V), dtype=np.uint8)
        tref = R.unpack_labels(tpk, tC)
        used = np.packbits(np.ones((1, tC, 1), dtype=np.uint8), axis=1)      # the random bytes also set bits past class tC - 1, which belong to no plane
        assert np.array_equal(np.packbits(tref.reshape(planes // tC, tC, V), axis=1), tpk & used)
    else:
        t = (g.random((planes, V)) < 0.3).astype(np.uint8)
        tref = t
    k = (g.random((planes, V)) < 0.8).astype(np.uint8) if with_k else None
    w2 = (g.random((planes, V)) < 0.5).astype(np.uint8) if with_w2 else None
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)      # noqa: E731
    xd, td, tpkd, kd, w2d = dev(x), dev(t), dev(tpk), dev(k), dev(w2)
    nb = ops._L().rsuper_plane_partials_blocks(V)
    assert nb == min(64, -(-V // 4096))
    pblk = torch.full((planes, nb, 6), float('nan'), device=DEV, dtype=torch.float64)
    sums = _nan((planes, 6), torch.float32)
    _c('rsuper_plane_partials_fwd3', ops._ptr(xd), V, ops._ptr(td), ops._ptr(tpkd), tP, tC, ops._ptr(kd), None, None, ops._ptr(w2d), ops._ptr(pblk), 0, planes, V)
    _c('rsuper_plane_sums_reduce', ops._ptr(pblk), planes, nb, ops._ptr(sums))
    torch.cuda.synchronize()
    ref, bound = R.plane_sums(x, tref, k, w2, chain=R.plane_chain(V, nb))
    r = {'pblk': R.plane_ratio(pblk.cpu().sum(1), ref, bound), 'sums': R.plane_ratio(sums.cpu(), ref, bound, reduced=True)}
    _report(f'plane sums {name} {planes}x{V} {labels} k={with_k} w2={with_w2}', r, f'{nb} blocks per plane')
