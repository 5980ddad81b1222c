"""tests/glue_ref.py against itself, on the CPU, before any kernel is judged by it:

  * every reference equals torch float64 autograd of the operation it restates (F.max_pool3d, strided slicing, F.interpolate(align_corners=True), an
    explicit instance norm, F.binary_cross_entropy_with_logits) on ragged shapes, the pool ones also on inputs full of ties;
  * a CORRECT float32 evaluation of the trilinear kernels' arithmetic (lin_coord of csrc/up_coord.hpp restated in NumPy float32, no fused multiply-add,
    every operation rounded once) stays inside the trilinear bounds of the exact-rational reference at every shape tests/test_gpu_glue_ref.py runs -- the
    derivation of the bound is what this tests: were it violated, the derivation would be wrong, not the cases;
  * every bound rejects a subtly wrong kernel: mutants of the reference output made on the CPU must give a ratio > 1 or an inequality;
  * the case tables name the kernel, selector and channel split rsuper_glue_plan answers for their shapes (host code: no GPU needed).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ref as R  # noqa: E402


def _nc(t):
    """channels-last (N, D, H, W, C) -> (N, C, D, H, W)"""
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1.0)


def _rn(t, mode):
    """float64 -> the stored value (round to nearest even), as float64"""
    return t.float().to(R.DTYPES[mode]).double()


def _truncate_bf16(t):
    """float64 -> bf16 by dropping the low 16 bits of the f32 value: the mutant that does not round"""
    return (t.float().view(torch.int32) & -65536).view(torch.float32).double()


# ================================================================================================ the references are right
RAGGED = [(2, (7, 9, 11), 3), (1, (6, 10, 14), 2), (2, (2, 3, 5), 4), (1, (12, 12, 12), 2)]


@pytest.mark.parametrize('N,dims,C', RAGGED)
@pytest.mark.parametrize('kind', ['gauss', 'levels', 'ints'])
def test_maxpool_reference_equals_float64_autograd(N, dims, C, kind):
    x = R.stored(1, (N,) + dims + (C,), 'f32', kind).double()
    xn = _nc(x).requires_grad_(True)
    y = F.max_pool3d(xn, 2)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y.backward(dy)
    add = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    assert torch.equal(R.maxpool_fwd(x), _cl(y.detach()))
    dx, mag = R.maxpool_bwd(x, _cl(dy))
    assert torch.equal(dx, _cl(xn.grad))                         # ATen routes to the first maximum too, ties or not
    dx2, mag2 = R.maxpool_bwd(x, _cl(dy), add)
    assert torch.equal(dx2, _cl(xn.grad) + add) and torch.equal(mag2, mag + add.abs()) and bool((mag >= dx.abs()).all())
    if any(d & 1 for d in dims):                                 # the trailing planes of odd sizes get no gradient
        D, H, W = dims
        tail = torch.ones(dims, dtype=torch.bool)
        tail[:D // 2 * 2, :H // 2 * 2, :W // 2 * 2] = False
        assert not bool(dx[:, tail].any())


@pytest.mark.parametrize('N,dims,C', RAGGED)
def test_subsample_reference_equals_float64_autograd(N, dims, C):
    x = R.stored(4, (N,) + dims + (C,), 'f32').double().requires_grad_(True)
    y = x[:, ::2, ::2, ::2]
    assert tuple(y.shape[1:4]) == tuple((d + 1) // 2 for d in dims)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    y.backward(dy)
    assert torch.equal(R.subsample_fwd(x.detach()), y.detach()) and torch.equal(R.subsample_bwd(dy, dims), x.grad)


UP_SHAPES = [(2, (3, 5, 4), (7, 9, 11), 3), (1, (5, 1, 7), (5, 4, 7), 2), (1, (6, 6, 6), (12, 12, 12), 2), (1, (3, 3, 4), (8, 9, 10), 2), (1, (5, 4, 3), (5, 4, 3), 2),
             (1, (1, 1, 40), (1, 1, 79), 2), (1, (4, 4, 4), (1, 6, 4), 2)]


@pytest.mark.parametrize('N,I,O,C', UP_SHAPES)
def test_trilinear_reference_equals_float64_autograd(N, I, O, C):
    x = R.stored(6, (N,) + I + (C,), 'f32').double()
    xn = _nc(x).requires_grad_(True)
    y = F.interpolate(xn, size=O, mode='trilinear', align_corners=True)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    y.backward(dy)
    ref, mag = R.trilinear_fwd(x, O)
    assert _close(ref, _cl(y.detach())) and bool((mag * (1 + 1e-12) >= ref.abs()).all())
    dx, mw, ms, K = R.trilinear_bwd(_cl(dy), I)
    assert _close(dx, _cl(xn.grad)) and bool((mw * (1 + 1e-12) >= dx.abs()).all()) and bool((ms * (1 + 1e-12) >= mw).all()) and K >= 1


@pytest.mark.parametrize('N,vox,C,nadd', [(2, 693, 8, 0), (1, 100, 24, 1), (3, 37, 4, 2)])
def test_norm_tail_reference_equals_float64_autograd(N, vox, C, nadd):
    gen = torch.Generator().manual_seed(8)
    x = (torch.randn((N, vox, C), dtype=torch.float64, generator=gen) * 1.7 + 0.4).requires_grad_(True)
    g = torch.randn((N, vox, C), dtype=torch.float64, generator=gen)
    adds = [torch.randn((N, vox, C), dtype=torch.float64, generator=gen) for _ in range(nadd)]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    xn = (x - mean) / torch.sqrt(var + R.EPS)                    # nn.InstanceNorm3d(eps=1e-4, affine=False): biased variance
    xn.backward(g)
    mr = torch.stack([mean[:, 0].detach(), 1.0 / torch.sqrt(var[:, 0].detach() + R.EPS)], -1)
    gm = torch.stack([g.mean(1), (g * xn.detach()).mean(1)], -1)
    ref, mag = R.in_bwd_tail(g, x.detach(), mr, gm, adds)
    assert _close(ref, x.grad + sum(adds), 1e-11) and bool((mag * (1 + 1e-12) >= ref.abs()).all())


def _plane_inputs(planes, V, labels, with_k, with_w2, seed=41):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((planes, V)) * 3).astype(np.float32)
    tpk, tC = None, 0
    if labels == 'bits':
        tC = 26 if planes % 26 == 0 else planes
        lab = (g.random((planes // tC, tC, V)) < 0.3).astype(np.uint8)
        tpk = np.packbits(lab, axis=1)                           # the dataset's form: np.packbits along the class axis
        t = lab.reshape(planes, V)
    else:
        t = (g.random((planes, V)) < 0.3).astype(np.uint8)
    k = (g.random((planes, V)) < 0.8).astype(np.uint8) if with_k else None
    w2 = (g.random((planes, V)) < 0.5).astype(np.uint8) if with_w2 else None
    return x, t, tpk, tC, k, w2


@pytest.mark.parametrize('case', R.PLANE_CASES, ids=[c[0] for c in R.PLANE_CASES])
def test_plane_sums_reference_equals_float64_torch(case):
    _, planes, V, labels, with_k, with_w2 = case
    x, t, tpk, tC, k, w2 = _plane_inputs(planes, V, labels, with_k, with_w2)
    if tpk is not None:
        assert tpk.shape == (planes // tC, (tC + 7) // 8, V) and np.array_equal(R.unpack_labels(tpk, tC), t)
    w1 = np.random.default_rng(1).random((planes, V))
    from rsuper_amd.hip import lib
    ref, bound = R.plane_sums(x, t, k, w2, w1, chain=R.plane_chain(V, lib.lib().rsuper_plane_partials_blocks(V)))
    xd, tf = torch.from_numpy(x).double(), torch.from_numpy(t).double()
    kf = torch.ones_like(xd) if k is None else torch.from_numpy(k).double()
    bgf = torch.ones_like(xd) if w2 is None else 1 - torch.from_numpy(w2).double()
    bce = F.binary_cross_entropy_with_logits(xd, tf, reduction='none') * kf
    sg = torch.sigmoid(xd)
    want = torch.stack([bce.sum(1), (sg * kf).sum(1), (sg * tf * kf).sum(1), (tf * kf).sum(1), (bce * torch.from_numpy(w1)).sum(1), (bce * bgf).sum(1)], -1)
    assert _close(ref, want, 1e-12)
    # the bound beats check_plane_partials' 2e-5 -- of each ENTRY, not of the largest sum -- and leaves the count exact
    assert bool((bound[:, 3] == 0).all()) and bool((bound[:, [0, 1, 2, 4, 5]] < 2e-5 * ref[:, [0, 1, 2, 4, 5]].abs()).all())
    print(f'plane sums {case[0]}: bound / |ref| at most {(bound[:, [0, 1, 2, 4, 5]] / ref[:, [0, 1, 2, 4, 5]].abs()).max().item():.2e}')


def test_stat_sums_and_the_exactness_cap():
    y = R.stored(9, (2, 5, 6, 7, 8), 'bf16', 'ints')
    s = R.stat_sums_exact(y)
    yd = y.double()
    assert torch.equal(s[..., 0], yd.sum((1, 2, 3))) and torch.equal(s[..., 1], (yd * yd).sum((1, 2, 3)))
    # any order of f32 partial sums is exact below the cap: a shuffled float32 accumulation gives the same integers
    flat = y.float().reshape(2, -1, 8)
    perm = torch.randperm(flat.shape[1], generator=torch.Generator().manual_seed(1))
    acc = torch.zeros((2, 8), dtype=torch.float32)
    for i in perm.tolist():
        acc = acc + flat[:, i] * flat[:, i]
    assert torch.equal(acc.double(), s[..., 1])
    with pytest.raises(AssertionError):
        R.stat_sums_exact(torch.full((1, 64, 64, 64, 8), 8.0))   # 2^18 voxels x 64 = 2^24
    with pytest.raises(AssertionError):
        R.stat_sums_exact(torch.full((1, 2, 2, 2, 8), 0.5))


# ================================================================================================ a correct f32 evaluation stays inside the trilinear bounds
def _up_fwd_all():
    return [c[:6] for c in R.UP_FWD_CASES] + [R.UP_FWD_STRIDED[:6]]


@pytest.mark.parametrize('case', _up_fwd_all(), ids=[c[0] for c in _up_fwd_all()])
def test_f32_restatement_within_the_trilinear_forward_bound(case):
    name, mode, N, I, O, C = case
    x = R.stored(31, (N,) + I + (C,), mode)
    ref, mag = R.trilinear_fwd(x, O)
    got = torch.from_numpy(R.trilinear_fwd_f32(x.float().numpy(), O))
    q32 = R.up_fwd_ratio(got, ref, mag, I, 'f32')                # the unrounded f32 result against the f32 form of the bound: the stricter one
    q = R.up_fwd_ratio(_rn(got.double(), mode), ref, mag, I, mode)
    print(f'up_fwd {name}: f32 restatement uses {q32:.3f} of the bound (c = {R.up_fwd_c(I)}), {q:.3f} after the storage rounding')
    assert q32 <= 1.0 and q <= 1.0


def test_f32_coordinate_error_within_the_derived_figure():
    """|src_f32 - src| <= 2 (I - 1) 2^-24 on every axis of every case, and the sixteen 1-D pairs up to 1536 -> 3071"""
    pairs = {(i, o) for c in _up_fwd_all() + [c[:6] for c in R.UP_BWD_CASES] for i, o in zip(c[3], c[4])}
    pairs |= {(2, 3), (3, 7), (6, 12), (12, 24), (24, 48), (48, 96), (96, 192), (5, 17), (100, 333), (257, 1000), (768, 1535), (1024, 2047), (1536, 3070),
              (1536, 3071), (1000, 1001), (1535, 1536)}
    worst = 0.0
    for I, O in sorted(pairs):
        if I == 1 or O == 1:
            continue
        scale = np.float32(np.float32(I - 1) / np.float32(O - 1))
        src = (scale * np.arange(O, dtype=np.float32)).astype(np.float32).astype(np.float64)
        exact = np.array([float(R.src_coord(o, I, O)) for o in range(O)])
        e = np.abs(src - exact).max() / ((I - 1) * R.U)
        worst = max(worst, e)
        assert e <= 2.0, (I, O, e)
    print(f'worst |d src| = {worst:.3f} (I - 1) 2^-24')


@pytest.mark.parametrize('case', R.UP_BWD_CASES, ids=[c[0] for c in R.UP_BWD_CASES])
def test_f32_restatement_within_the_trilinear_backward_bound(case):
    name, mode, N, I, O, C = case[:6]
    dy = R.stored(33, (N,) + O + (C,), mode)
    ref, mw, ms, K = R.trilinear_bwd(dy, I)
    got = torch.from_numpy(R.trilinear_bwd_f32(dy.float().numpy(), I))
    q32 = R.up_bwd_ratio(got, ref, mw, ms, K, I, 'f32')
    q = R.up_bwd_ratio(_rn(got.double(), mode), ref, mw, ms, K, I, mode)
    print(f'up_bwd {name}: f32 restatement uses {q32:.3f} of the bound (K = {K}), {q:.3f} after the storage rounding')
    assert q32 <= 1.0 and q <= 1.0


# ================================================================================================ the bounds bite
def test_mutant_truncation_instead_of_rounding():
    """bf16 by truncation errs by up to 2^-7 relative: over the half ulp every stored result is allowed"""
    gen = torch.Generator().manual_seed(11)
    N, vox, C = 2, 693, 8
    g, x = R.stored(1, (N, vox, C), 'bf16'), R.stored(2, (N, vox, C), 'bf16')
    mr = torch.stack([torch.randn((N, C), generator=gen), torch.randn((N, C), generator=gen).abs() + 0.5], -1)
    gm = torch.randn((N, C, 2), generator=gen) * 0.1
    ref, mag = R.in_bwd_tail(g, x, mr, gm, [R.stored(3, (N, vox, C), 'bf16')])
    assert R.tail_ratio(_rn(ref, 'bf16'), ref, mag, 'bf16') <= 1.0 < R.tail_ratio(_truncate_bf16(ref), ref, mag, 'bf16')
    xp, dy, add = R.stored(4, (1, 6, 10, 14, 8), 'bf16'), R.stored(5, (1, 3, 5, 7, 8), 'bf16'), R.stored(6, (1, 6, 10, 14, 8), 'bf16')
    ref, mag = R.maxpool_bwd(xp, dy, add)
    assert R.rounded_sum_ratio(_rn(ref, 'bf16'), ref, mag, 'bf16') <= 1.0 < R.rounded_sum_ratio(_truncate_bf16(ref), ref, mag, 'bf16')
    ref, mag = R.trilinear_fwd(R.stored(7, (1, 3, 5, 4, 8), 'bf16'), (7, 9, 11))
    assert R.up_fwd_ratio(_rn(ref, 'bf16'), ref, mag, (3, 5, 4), 'bf16') <= 1.0 < R.up_fwd_ratio(_truncate_bf16(ref), ref, mag, (3, 5, 4), 'bf16')
    ref, mw, ms, K = R.trilinear_bwd(R.stored(8, (1, 7, 9, 11, 8), 'bf16'), (3, 5, 4))
    assert R.up_bwd_ratio(_rn(ref, 'bf16'), ref, mw, ms, K, (3, 5, 4), 'bf16') <= 1.0 < R.up_bwd_ratio(_truncate_bf16(ref), ref, mw, ms, K, (3, 5, 4), 'bf16')


def test_mutant_last_maximum_routing():
    x, dy = R.stored(12, (1, 6, 10, 14, 8), 'bf16', 'levels'), R.stored(13, (1, 3, 5, 7, 8), 'bf16')
    first, _ = R.maxpool_bwd(x, dy)
    last, _ = R.maxpool_bwd(x, dy, last=True)
    assert not torch.equal(first, last) and torch.equal(first.sum((1, 2, 3)), last.sum((1, 2, 3)))
    xg = R.stored(12, (1, 6, 10, 14, 8), 'f32')                  # without ties the two agree: the tied input is what tells them apart
    assert torch.equal(R.maxpool_bwd(xg, dy)[0], R.maxpool_bwd(xg, dy, last=True)[0])


def _drop_tap(Wm, lo=2.0 ** -10):
    """the matrix with its smallest weight >= 2^-10 zeroed, and that weight"""
    cand = np.where(Wm >= lo, Wm, np.inf)
    o, i = np.unravel_index(np.argmin(cand), Wm.shape)
    out = Wm.copy()
    out[o, i] = 0.0
    return out, Wm[o, i]


@pytest.mark.parametrize('mode,I,O', [('bf16', (3, 5, 4), (7, 9, 11)), ('f32', (3, 5, 4), (7, 9, 11)), ('bf16', (12, 12, 12), (24, 24, 24)),
                                      ('f32', (1, 1, 1536), (1, 1, 3070))])
def test_mutant_dropped_trilinear_tap(mode, I, O, monkeypatch):
    """One tap of one output coordinate of the w axis, the lightest one of weight >= 2^-10, is left out -- forward and backward.  (At 1536 -> 3070 that
    weight is 1 / 1023 and c u = 3.7e-4: the f32 bound still sees it; behind a bf16 rounding of 2^-8 |ref| it is visible only where |ref| is small.)"""
    C = 8
    x, dy = R.stored(14, (1,) + I + (C,), mode), R.stored(15, (1,) + O + (C,), mode)
    ref, mag = R.trilinear_fwd(x, O)
    dref, mw, ms, K = R.trilinear_bwd(dy, I)
    real = R.axis_tables

    def mutant(i, o):
        Wm, S, lo, hi = real(i, o)
        if (i, o) == (I[2], O[2]):
            Wm, w = _drop_tap(Wm)
            assert 2.0 ** -10 <= w < 0.11
        return Wm, S, lo, hi
    monkeypatch.setattr(R, 'axis_tables', mutant)
    bad, _ = R.trilinear_fwd(x, O)
    dbad = R.trilinear_bwd(dy, I)[0]
    monkeypatch.setattr(R, 'axis_tables', real)
    assert R.up_fwd_ratio(_rn(ref, mode), ref, mag, I, mode) <= 1.0 < R.up_fwd_ratio(_rn(bad, mode), ref, mag, I, mode)
    assert R.up_bwd_ratio(_rn(dref, mode), dref, mw, ms, K, I, mode) <= 1.0 < R.up_bwd_ratio(_rn(dbad, mode), dref, mw, ms, K, I, mode)


def test_mutant_voxel_left_out_of_a_statistics_row():
    y = R.stored(16, (2, 3, 4, 5, 8), 'bf16', 'ints')
    s = R.stat_sums_exact(y)
    v = y.double()[:, 1, 2, 3]                                   # one voxel per sample
    assert bool((v != 0).any())
    assert not torch.equal(s - torch.stack([v, v * v], -1), s) and not torch.equal(s + torch.stack([v, v * v], -1), s)
    # general inputs: the finalised (mean, rstd) of 60 voxels with one left out is far outside 1e-4
    yg = R.stored(17, (2, 3, 4, 5, 8), 'bf16').double()
    cnt = 60
    s = R.stat_sums(yg)

    def fin(s):
        m = s[..., 0] / cnt
        return torch.stack([m, 1 / torch.sqrt((s[..., 1] / cnt - m * m).clamp_min(0) + R.EPS)], -1)
    assert max(R.stats_ratio(fin(s), yg)) <= 1.0
    v = yg[:, 1, 2, 3]
    assert min(R.stats_ratio(fin(s - torch.stack([v, v * v], -1)), yg)) > 1.0


def test_mutant_m2_applied_to_x_instead_of_x_n():
    gen = torch.Generator().manual_seed(18)
    N, vox, C = 2, 693, 8
    g, x = R.stored(1, (N, vox, C), 'bf16'), R.stored(2, (N, vox, C), 'bf16')
    mr = torch.stack([torch.randn((N, C), generator=gen), torch.randn((N, C), generator=gen).abs() + 0.5], -1)
    gm = torch.randn((N, C, 2), generator=gen) * 0.1
    ref, mag = R.in_bwd_tail(g, x, mr, gm)
    rs, m1, m2 = (t.double()[:, None, :] for t in (mr[..., 1], gm[..., 0], gm[..., 1]))
    bad = rs * (g.double() - m1 - x.double() * m2)
    assert R.tail_ratio(_rn(ref, 'bf16'), ref, mag, 'bf16') <= 1.0 < R.tail_ratio(_rn(bad, 'bf16'), ref, mag, 'bf16')


def test_mutant_bit_order_of_packed_labels():
    x, t, tpk, tC, k, _ = _plane_inputs(26, 640, 'bits', True, False)
    ref, bound = R.plane_sums(x, t, k, chain=R.plane_chain(640, 1))
    B, tP, V = tpk.shape
    wrong = np.stack([(tpk[:, c >> 3] >> (c & 7)) & 1 for c in range(tC)], 1).reshape(B * tC, V)
    bad, _ = R.plane_sums(x, wrong, k, chain=R.plane_chain(640, 1))
    assert R.plane_ratio(ref, ref, bound) == 0.0 and R.plane_ratio(bad, ref, bound) == float('inf')      # the count column is an inequality
    assert R.plane_ratio(bad[:, [0, 2]], ref[:, [0, 2]], bound[:, [0, 2]]) > 1.0                          # and the sums that read t are far off
    assert R.plane_ratio(ref + 0.5 * bound, ref, bound) <= 1.0 < R.plane_ratio(ref + 2 * bound, ref, bound)


# ================================================================================================ the case tables name what the plan answers
def test_case_tables_name_the_planned_kernels():
    """rsuper_glue_plan is host code: the rungs the GPU cases claim are checked here as well, so a dispatch change shows without a GPU."""
    from rsuper_amd.hip import lib
    assert lib.lib().rsuper_glue_variant(-1) == 1
    for name, mode, N, vox, C, nadd, kernel, sel in R.TAIL_CASES:
        p = R.glue_plan('in_bwd', mode, N, [vox], C)
        assert (p['kernel'], p['sel']) == (kernel, sel), (name, p)
    assert {(c[6], c[7]) for c in R.TAIL_CASES} == {('in_bwd_finalize_kernel', 0), ('in_bwd_finalize2_kernel', 2), ('in_bwd_finalize2_kernel', 4)}
    for name, mode, N, dims, C, kernel, z, bthreads in R.POOL_CASES:
        p, q = R.glue_plan('pool_fwd', mode, N, dims, C), R.glue_plan('pool_bwd', mode, N, dims, C)
        assert (p['kernel'], p['bz'], q['kernel'], q['threads']) == (kernel, z, 'maxpool_bwd_kernel', bthreads), (name, p, q)
    assert {c[6] for c in R.POOL_CASES} == {1, 2, 4} and {c[7] for c in R.POOL_CASES} == {64, 256} and len({c[5] for c in R.POOL_CASES}) == 2
    for name, mode, N, dims, C, z in R.SUB_CASES:
        p = R.glue_plan('sub_fwd', mode, N, dims, C)
        assert (p['kernel'], p['bz']) == ('subsample_fwd_kernel', z), (name, p)
    for name, mode, N, I, O, C, kernel, z in R.UP_FWD_CASES:
        p = R.glue_plan('up_fwd', mode, N, I + O, C)
        assert (p['kernel'], p['bz']) == (kernel, z), (name, p)
    name, mode, N, I, O, C, kernel = R.UP_FWD_STRIDED
    assert R.glue_plan('up_fwd', mode, N, I + O, C, ld=96)['kernel'] == kernel
    for name, mode, N, I, O, C, kernel, nt in R.UP_BWD_CASES:
        p = R.glue_plan('up_bwd', mode, N, I + O, C)
        assert (p['kernel'], p['sel']) == (kernel, nt), (name, p)
    assert {c[7] for c in R.UP_BWD_CASES} == {0, 4, 6}
    blocks = {c[0]: lib.lib().rsuper_plane_partials_blocks(c[2]) for c in R.PLANE_CASES}
    assert (blocks['V4096'], blocks['V4097']) == (1, 2), blocks
