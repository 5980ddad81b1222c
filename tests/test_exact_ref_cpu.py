"""The instrument of tests/test_gpu_exact_int.py checked without a GPU (tests/exact_ref.py): every GPU case is exact in f32, the integer x_hat survives the
kernels' bf16 prologue unchanged, the order of an f32 accumulation really cannot matter on these operands, one zeroed voxel / reduction row changes the
reference at exactly the elements it feeds (so `mismatch` would name it), and every stride-1 case names the kernel the dispatch gives it."""
import ctypes

import numpy as np
import pytest
import torch

import exact_ref as er
from gpu_checks import WGRAD_KERNEL_NAMES, _xhat_bf16
from test_gpu_mf_kernels import POINTWISE                                   # the list the GPU file runs, not a copy


def _wgrad_keys():
    keys = [er.wgrad_int_key(c) for c in er.WGRAD_INT] + [(N, S, Ca, 0, Ya, Yb, 'both', 2, False) for _, N, S, Ca, Ya, Yb in er.WGRAD_S2_INT]
    return sorted(set(keys), key=keys.index)


@pytest.mark.parametrize('key', _wgrad_keys(), ids=lambda k: f"N{k[0]}_{'x'.join(map(str, k[1]))}_{k[2]}+{k[3]}to{k[4]}+{k[5]}_{k[6]}_s{k[7]}")
def test_every_weight_gradient_case_is_exact(key):
    mag = er.wgrad_mag(*key)
    assert er.exact_ok(mag), float(mag.max())
    assert float(mag.max()) > 0


@pytest.mark.parametrize('R,K,N', sorted({c[1:] for c in POINTWISE} | {c[1:] for c in er.POINTWISE_SLICED}))
def test_every_pointwise_case_is_exact(R, K, N):
    for name, (ref, mag) in er.pointwise_ref(er.pointwise_operands(R, K, N)).items():
        assert er.exact_ok(mag), (name, float(mag.max()))
        assert bool((ref.abs() <= mag).all())


def test_exact_ok_is_the_2_to_24_condition_on_halves():
    assert er.exact_ok(torch.tensor([2.0 ** 23 - 0.5])) and not er.exact_ok(torch.tensor([1.0, 2.0 ** 23]))


@pytest.mark.parametrize('case', er.WGRAD_INT, ids=lambda c: f"{c[0]}{c[1]}mt{c[2]}_{c[3]}_N{c[4]}_{'x'.join(map(str, c[5]))}_{c[6]}+{c[7]}to{c[8]}+{c[9]}_thr{c[11]}_tr{c[12]}")
def test_every_stride_1_case_names_the_kernel_of_the_plan(case):
    """rsuper_conv3_wgrad_plan is answered on the host: what check_wgrad_int asserts before its launch, here without one."""
    from rsuper_amd.hip import lib
    L = lib.lib()
    kernel, cfg, mt, mode, N, S, Ca, Cb, Ya, Yb, norm, thr, tr = case[:13]
    old = L.rsuper_conv3_wgrad2_min_tiles(-1)
    try:
        if thr is not None:
            L.rsuper_conv3_wgrad2_min_tiles(thr)
        plan = (ctypes.c_int * 4)()
        assert L.rsuper_conv3_wgrad_plan(lib.BF16 if mode == 'bf16' else lib.F32, tr, Ca, Cb, Ya, Yb, N, *S, int(norm == 'mixed'), 0, plan) == 0
    finally:
        L.rsuper_conv3_wgrad2_min_tiles(old)
    assert (WGRAD_KERNEL_NAMES[plan[0]], plan[2], plan[3]) == (kernel, cfg, mt), tuple(plan)


def test_the_case_list_reaches_every_kernel_and_configuration_of_the_plan():
    ran = {c[:3] for c in er.WGRAD_INT}
    assert {('tile', 0, 1), ('tile', 1, 2), ('tile', 2, 2), ('wgrad2', 0, 1), ('wgrad2', 2, 2), ('wgrad2', 2, 1), ('sv', 1, 1)} <= ran


@pytest.mark.parametrize('narrow', [False, True])
def test_integer_xhat_is_the_bf16_prologue_of_the_kernels(narrow):
    g = np.random.default_rng(5)
    x = er._ints(g, (2, 7, 3, 4, 5), er.X_NARROW if narrow else er.X_RANGE)
    mr = er.stats_int(g, 2, 7, narrow)
    assert not bool((mr[0] == mr[1]).all()) and not bool((mr[:, 0] == mr[:, 1]).all())        # samples and neighbouring channels differ
    xh = er.xhat_int(x, mr)
    assert torch.equal(xh, _xhat_bf16(x, mr))                                                    # f32 fma + bf16 rounding: nothing to round
    assert torch.equal(xh.float().bfloat16().double(), xh) and torch.equal(x.bfloat16().float(), x)
    assert torch.equal(xh * 2, (xh * 2).round()) and float(xh.max()) <= (10.0 if not narrow else 6.0) and float(xh.min()) >= 0.0
    assert torch.equal(er.xhat_int(x, None), x.double())


# ---------------------------------------------------------------------------------------------- order independence
def _taps(xh, stride, So):
    """(R, C, 27) float64: x_hat at the 27 taps of every dY voxel (zero padding), R = N x dY grid in row-major order."""
    N, C = xh.shape[:2]
    xp = torch.nn.functional.pad(xh, (1, 1, 1, 1, 1, 1))
    cols = [xp[:, :, kd:kd + stride * So[0]:stride, kh:kh + stride * So[1]:stride, kw:kw + stride * So[2]:stride] for kd in range(3) for kh in range(3) for kw in range(3)]
    return torch.stack(cols, -1).permute(0, 2, 3, 4, 1, 5).reshape(-1, C, 27)


def _f32_orders(a, b, ref):
    """a (R, P), b (R, Q) float64 terms of ref (P, Q) = a^T b: accumulate the R outer products in f32 one at a time in a shuffled order, and in 7 unequal
    slabs (each summed on its own, in its own shuffled order) added afterwards; both must equal ref exactly."""
    a32, b32 = a.float(), b.float()
    R = a.shape[0]
    g = np.random.default_rng(R)
    acc = torch.zeros(ref.shape, dtype=torch.float32)
    for r in g.permutation(R):
        acc += a32[r][:, None] * b32[r][None, :]
    cuts = [0] + sorted(g.choice(np.arange(1, R), size=6, replace=False).tolist()) + [R]
    assert len(set(np.diff(cuts).tolist())) > 1
    tot = torch.zeros(ref.shape, dtype=torch.float32)
    for lo, hi in reversed(list(zip(cuts[:-1], cuts[1:]))):
        part = torch.zeros(ref.shape, dtype=torch.float32)
        for r in lo + g.permutation(hi - lo):
            part += a32[r][:, None] * b32[r][None, :]
        tot += part
    assert er.mismatch(acc, ref)[0] == 0 and er.mismatch(tot, ref)[0] == 0


@pytest.mark.parametrize('key', [(1, (5, 6, 7), 8, 16, 8, 8, 'both', 1, False), (1, (7, 9, 35), 8, 0, 16, 16, 'both', 2, False)], ids=['stride1', 'stride2'])
def test_f32_accumulation_order_cannot_matter_for_the_weight_gradient(key):
    o, (ref, mag) = er.wgrad_operands(*key), er.wgrad_ref(*key)
    assert er.exact_ok(mag)
    dy = o['dy']
    Y, C = dy.shape[1], o['xh'].shape[1]
    taps = _taps(o['xh'], key[7], tuple(dy.shape[2:]))
    _f32_orders(dy.permute(0, 2, 3, 4, 1).reshape(-1, Y).double(), taps.reshape(-1, C * 27), ref.reshape(Y, C * 27))


def test_f32_accumulation_order_cannot_matter_for_the_pointwise_products():
    o = er.pointwise_operands(200, 116, 64)
    refs = er.pointwise_ref(o)
    _f32_orders(o['dy'].double(), o['x'].double(), refs['dw'][0])                                # reduction over the rows
    _f32_orders(o['x'].double().t().contiguous(), o['w'].double().t().contiguous(), refs['y'][0] - o['b'].double())      # reduction over K


# ---------------------------------------------------------------------------------------------- sensitivity
def _nonzero_case():
    """One x source, raw, every operand non-zero: zeros of x and dY replaced by 1, so that the count of a lost voxel is known."""
    N, S, Ca, Ya = 2, (5, 6, 7), 3, 4
    o = er.wgrad_operands(N, S, Ca, 0, Ya, 0, 'raw')
    x, dy = o['xa'].clone(), o['dy'].clone()
    x[x == 0] = 1.0
    dy[dy == 0] = 1.0
    return x, dy, Ca, Ya


@pytest.mark.parametrize('where,vox,taps', [('corner', (0, 0, 0), 8), ('face', (0, 2, 3), 18), ('edge', (4, 5, 3), 12), ('interior', (2, 3, 4), 27)])
def test_one_lost_voxel_shows_at_every_element_it_feeds(where, vox, taps):
    x, dy, Ca, Ya = _nonzero_case()
    ref = er.wgrad_f64(x, dy)
    lost = x.clone()
    lost[1, :, vox[0], vox[1], vox[2]] = 0.0                          # sample 1: every channel of the voxel
    n, first = er.mismatch(er.wgrad_f64(lost, dy), ref)
    assert n == taps * Ya * Ca and first is not None, (where, n)
    one = x.clone()
    one[1, 2, vox[0], vox[1], vox[2]] = 0.0                           # one channel: 27 Ya elements for an interior voxel
    n, first = er.mismatch(er.wgrad_f64(one, dy), ref)
    assert n == taps * Ya and first[0][1] == 2, (where, n, first)


def test_one_lost_voxel_shows_with_the_cases_own_operands_and_statistics():
    key = (1, (5, 6, 7), 8, 16, 8, 8, 'both', 1, False)
    o, (ref, _) = er.wgrad_operands(*key), er.wgrad_ref(*key)
    for vox in ((0, 0, 0), (4, 2, 3), (2, 3, 4)):
        xh = o['xh'].clone()
        xh[0, :, vox[0], vox[1], vox[2]] = 0.0
        assert er.mismatch(er.wgrad_f64(xh, o['dy']), ref)[0] >= 1, vox


def test_one_lost_reduction_row_shows_in_the_pointwise_products():
    o = er.pointwise_operands(65, 64, 64)
    refs = er.pointwise_ref(o)
    lost = dict(o)
    lost['x'] = o['x'].clone()
    lost['x'][64] = 0.0                                                # the last row: the second slab of the weight gradient at R = 65
    lost['dy'] = o['dy'].clone()
    lost['dy'][64] = 0.0
    got = er.pointwise_ref(lost)
    n_dw = int(torch.count_nonzero(o['dy'][64])) * int(torch.count_nonzero(o['x'][64]))
    assert er.mismatch(got['dw'][0], refs['dw'][0])[0] == n_dw > 0
    assert er.mismatch(got['db'][0], refs['db'][0])[0] == int(torch.count_nonzero(o['dy'][64])) > 0
    lost['w'] = o['w'].clone()
    lost['w'][:, 63] = 0.0                                             # one step of the forward's reduction
    assert er.mismatch(er.pointwise_ref(lost)['y'][0], refs['y'][0])[0] >= 1


def test_mismatch_compares_by_value_and_names_the_first_element():
    ref = torch.tensor([[0.0, 1.5], [-2.0, 3.0]], dtype=torch.float64)
    assert er.mismatch(torch.tensor([[-0.0, 1.5], [-2.0, 3.0]]), ref) == (0, None)               # -0 equals +0
    n, first = er.mismatch(torch.tensor([[0.0, 1.5], [float('nan'), 3.5]]), ref)
    assert n == 2 and first[0] == (1, 0) and np.isnan(first[1]) and first[2] == -2.0
    assert er.mismatch(torch.tensor([[0.0, float('inf')], [-2.0, 3.0]]), torch.tensor([[0.0, float('inf')], [-2.0, 3.0]], dtype=torch.float64))[0] == 1
    assert '1 of 4 differ, first at (0, 1)' in er.mismatch_note('dW', torch.tensor([[0.0, 1.0], [-2.0, 3.0]]), ref)
    assert er.mismatch_note('dW', ref.float(), ref) == ''
