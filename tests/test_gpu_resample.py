"""GPU tests of the whole-CT preprocessing (csrc/resample.hip rsuper_ct_stats / rsuper_ct_normalize / rsuper_pad_box, inference/preprocess.py) and the
class-stack resampler (rsuper_resample3d, inference/resample.py) against the reference's own outputs in tests/golden/resample.npz and, for shapes
without a fixture, the numpy restatement tests/resample_ref.py (which tests/test_resample_cpu.py pins to that fixture).

Bounds (derived, not tuned): trilinear within 12 * 2^-24 * max|x| of the float64 evaluation with the float32 weights (three nested lerps, at most 4
roundings each); z-score within 4 * 2^-24 * (max|clip(x)| + |mean|) / std (one subtraction, one division, mean and std each rounded once); mean
and std within 1e-6 relative of float64.  Nearest, thresholded and pad / unpad results are bit-exact."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import resample_ref as rr  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N_RS, N_NZ, N_PAD = 10, 5, 8
NPDT = {'u8': np.uint8, 'f32': np.float32, 'i16': np.int16}


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'resample.npz'))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def exact_of(g, key):
    return g[key].astype(np.float64) + g[key + '_delta'].astype(np.float64)


def xyz(size):
    return tuple(int(v) for v in size)[::-1]


def check_stack(x, out, thr, box=None, xbig=None):
    """Every output kind of one stack against the restatement; returns (nearest, trilinear, thresholded) as numpy arrays."""
    from rsuper_amd.inference import resample_image_with_gpu as rs
    t = dev(x if xbig is None else xbig)
    near = host(rs(t, new_size=xyz(out), interp='nearest', box=box))
    tri = host(rs(t, new_size=xyz(out), interp='trilinear', box=box))
    bits = host(rs(t, new_size=xyz(out), interp='trilinear', box=box, threshold=thr))
    exact = rr.resample(x, out, 'trilinear', np.float64)
    assert near.dtype == x.dtype and np.array_equal(near, rr.resample(x, out, 'nearest'))
    err = float(np.abs(tri.astype(np.float64) - exact).max())
    print(f'trilinear {x.shape} -> {out}: max error {err:.3e}, bound {rr.trilinear_bound(x):.3e}')
    assert tri.dtype == np.float32 and err <= rr.trilinear_bound(x)
    assert bits.dtype == np.uint8 and np.array_equal(bits, (tri > np.float32(thr)).astype(np.uint8))
    return near, tri, bits


@pytest.mark.parametrize('i', range(N_RS))
@pytest.mark.parametrize('dt', ['u8', 'f32'])
def test_fixture_resampling(g, i, dt):
    x, out = g[f'rs{i}_{dt}_x'], tuple(int(v) for v in g[f'rs{i}_out'])
    near, tri, bits = check_stack(x, out, rr.THRESHOLD[dt])
    assert np.array_equal(near, g[f'rs{i}_{dt}_nearest'])                                              # the reference, bit for bit
    idx = rr.sample_index(tri.size)
    assert np.abs(tri.reshape(-1)[idx].astype(np.float64) - exact_of(g, f'rs{i}_{dt}_tri')).max() <= rr.trilinear_bound(x)
    assert np.array_equal(np.packbits(bits.reshape(-1).astype(bool)), g[f'rs{i}_{dt}_thr'])            # every voxel, bit for bit


def test_box_equals_slicing_first_and_the_fixture(g):
    from rsuper_amd.inference import resample_image_with_gpu as rs, unpad_img
    i = int(g['box_case'][0])
    off, big_shape = g['box_offset'].tolist(), tuple(g['box_pad_shape'].tolist())
    out = tuple(int(v) for v in g[f'rs{i}_out'])
    for dt in ('u8', 'f32'):
        x = g[f'rs{i}_{dt}_x']
        big = rr.stack(big_shape, x.shape[0], 77, NPDT[dt])                                            # the padding holds other values, not zeros
        idx = [off[0], off[0] + x.shape[1], off[1], off[1] + x.shape[2], off[2], off[2] + x.shape[3]]
        big[:, idx[0]:idx[1], idx[2]:idx[3], idx[4]:idx[5]] = x
        near, tri, bits = check_stack(x, out, rr.THRESHOLD[dt], box=idx, xbig=big)
        assert np.array_equal(near, g[f'rs{i}_{dt}_nearest'])
        assert np.array_equal(np.packbits(bits.reshape(-1).astype(bool)), g[f'rs{i}_{dt}_thr'])
        t = dev(big)
        a3 = argparse.Namespace(dimension='3d')
        for interp in ('nearest', 'trilinear'):
            cut = torch.stack([unpad_img(p, idx, a3) for p in t])
            assert torch.equal(rs(t, new_size=xyz(out), interp=interp, box=idx), rs(cut, new_size=xyz(out), interp=interp))
            assert torch.equal(rs(t[1], new_size=xyz(out), interp=interp, box=idx), rs(cut[1], new_size=xyz(out), interp=interp))


# output rows of whole 16-byte / 4-byte vectors (no fixture case has Wo % 4 == 0), more than one x tile, more than one (z, y) tile; then the
# trilinear kernel's two paths: a tile of 4 x 8 output rows 256 wide stages its x-lerped source rows in LDS when they number at most 48 --
# 6 planes x 8 rows is the last that fits, 7 x 7 the first that does not, and 40 x 60 (a 10 : 1 reduction) is far beyond
@pytest.mark.parametrize('sin,sout', [((6, 7, 9), (9, 10, 16)), ((3, 3, 50), (5, 3, 260)), ((5, 20, 6), (9, 17, 8)), ((3, 4, 700), (2, 9, 1028)),
                                      ((6, 8, 140), (4, 8, 132)), ((7, 7, 140), (4, 8, 132)), ((40, 60, 300), (4, 8, 260))])
@pytest.mark.parametrize('dt', ['u8', 'f32'])
def test_vector_store_rows_match_the_restatement(sin, sout, dt):
    check_stack(rr.stack(sin, 2, 31, NPDT[dt]), sout, rr.THRESHOLD[dt])


def test_stack_equals_per_plane_calls_and_two_runs_agree(g):
    from rsuper_amd.inference import resample_image_with_gpu as rs
    x = dev(g['rs4_f32_x'])
    u = dev(g['rs4_u8_x'])
    out = xyz(g['rs4_out'])
    for t, interp, thr in ((x, 'trilinear', None), (x, 'trilinear', 0.5), (x, 'nearest', None), (u, 'nearest', None), (u, 'trilinear', None)):
        a = rs(t, new_size=out, interp=interp, threshold=thr)
        assert a.dim() == 4 and torch.equal(a, rs(t, new_size=out, interp=interp, threshold=thr))
        planes = [rs(p, new_size=out, interp=interp, threshold=thr) for p in t]
        assert all(p.dim() == 3 for p in planes) and torch.equal(a, torch.stack(planes))
    # new_size=None: the reference's rounding
    r = rs(x, old_spacing=(0.8, 0.8, 2.5), old_size=(22, 20, 12), new_spacing=(1., 1., 1.))
    assert tuple(r.shape[1:]) == tuple(rr.new_size((0.8, 0.8, 2.5), (22, 20, 12), (1., 1., 1.))) == (30, 16, 18)
    assert rs(x.view(torch.float32)[0] > 0.5, new_size=out, interp='nearest').dtype == torch.uint8      # a bool mask goes in as bytes


def test_poisoned_resample_output_changes_nothing():
    """The kernel writes every output voxel: the ABI called on a NaN-filled / 0xFF-filled buffer gives the entry's result."""
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import resample_image_with_gpu as rs
    x = dev(rr.stack((5, 9, 11), 2, 5, np.float32))
    out = (7, 6, 13)
    for interp, thr, odt in (('trilinear', None, torch.float32), ('trilinear', 0.5, torch.uint8), ('nearest', None, torch.float32)):
        want = rs(x, new_size=xyz(out), interp=interp, threshold=thr)
        buf = torch.full((2,) + out, float('nan'), device=DEV) if odt == torch.float32 else torch.full((2,) + out, 255, device=DEV, dtype=torch.uint8)
        rc = lib.lib().rsuper_resample3d(x.data_ptr(), 1, 2, 5, 9, 11, 0, 0, 0, 5, 9, 11, buf.data_ptr(), 1 if odt == torch.float32 else 0,
                                         out[0], out[1], out[2], 1 if interp == 'trilinear' else 0, 0 if thr is None else 1, thr or 0.0,
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and torch.equal(buf, want)


def test_ct_like_stack_against_the_restatement():
    """(40, 96, 100) padded prediction, 5 planes, unpadded by the box and brought to (63, 123, 131)."""
    box = [2, 38, 0, 96, 3, 99]
    out = (63, 123, 131)
    for dt in ('u8', 'f32'):
        big = rr.stack((40, 96, 100), 5, 123, NPDT[dt])
        x = np.ascontiguousarray(big[:, box[0]:box[1], box[2]:box[3], box[4]:box[5]])
        check_stack(x, out, rr.THRESHOLD[dt], box=box, xbig=big)


# ---- z-score
def run_abi_zscore(x, out, off, ws, ms):
    from rsuper_amd.hip import lib
    L, s = lib.lib(), torch.cuda.current_stream().cuda_stream
    dt = 2 if x.dtype == torch.int16 else 1
    D, H, W = x.shape
    n = ws.numel() * ws.element_size()
    assert L.rsuper_ct_stats(x.data_ptr(), dt, D, H, W, rr.CLIP[0], rr.CLIP[1], ws.data_ptr(), n, s) == 0
    assert L.rsuper_ct_normalize(x.data_ptr(), dt, D, H, W, rr.CLIP[0], rr.CLIP[1], ws.data_ptr(), n, out.data_ptr(), out.shape[0], out.shape[1],
                                 out.shape[2], off[0], off[1], off[2], ms.data_ptr(), s) == 0


def check_zscore(x, got, mean, std):
    exact, m, s = rr.zscore(x)
    bound = rr.zscore_bound(x, m, s)
    err = float(np.abs(got.astype(np.float64) - exact).max())
    print(f'z-score {x.shape} {x.dtype}: max error {err:.3e}, bound {bound:.3e}; mean {mean!r} vs {m!r}, std {std!r} vs {s!r}')
    assert got.dtype == np.float32 and err <= bound
    assert abs(mean - m) <= 1e-6 * abs(m) and abs(std - s) <= 1e-6 * abs(s)
    return exact, bound


@pytest.mark.parametrize('i', range(N_NZ))
@pytest.mark.parametrize('dt', ['i16', 'f32'])
def test_fixture_zscore(g, i, dt):
    from rsuper_amd.inference import normalize_ct
    shape = tuple(int(v) for v in g[f'nz{i}_shape'])
    mean, sigma, seed = g[f'nz{i}_params']
    x = rr.ct_volume(shape, mean, sigma, int(seed), NPDT[dt])
    out, m, s = normalize_ct(dev(x))
    assert m.is_cuda and m.dim() == 0 and s.dim() == 0
    exact, bound = check_zscore(x, host(out), float(m), float(s))
    np.testing.assert_allclose([float(m), float(s)], g[f'nz{i}_{dt}_stats'], rtol=1e-6)
    k = rr.sample_index(exact.size, 512, 512)
    assert np.abs(host(out).reshape(-1)[k].astype(np.float64) - exact_of(g, f'nz{i}_{dt}_ref')).max() <= bound


def test_single_voxel_and_constant_volumes_give_nan_like_the_reference():
    from rsuper_amd.inference import normalize_ct
    out, m, s = normalize_ct(torch.full((1, 1, 1), 40, dtype=torch.int16, device=DEV))                  # N = 1: 0 / 0
    assert bool(torch.isnan(out).all()) and float(m) == 40.0 and bool(torch.isnan(s))
    for x in (torch.full((6, 10, 11), -300, dtype=torch.int16, device=DEV), torch.full((6, 10, 11), 2000.0, device=DEV)):
        out, m, s = normalize_ct(x, pad=((9, 10, 16), (2, 0, 3)))
        box = out[2:8, :, 3:14]
        assert bool(torch.isnan(box).all()) and float(s) == 0.0 and float(m) == float(x.clamp(-991, 500)[0, 0, 0])
        out[2:8, :, 3:14] = 0
        assert tuple(out.shape) == (9, 10, 16) and int(torch.count_nonzero(out)) == 0 and not bool(torch.isnan(out).any())   # the padding stays zero


@pytest.mark.parametrize('dt', ['i16', 'f32'])
def test_zscore_ragged_shapes_offsets_poison_and_repeat(dt):
    """Odd shapes at an unaligned base address into an unaligned, padded output; a NaN-filled workspace and output; two runs."""
    from rsuper_amd.inference import normalize_ct
    for shape, pad_shape, off, skip in (((3, 5, 7), (4, 9, 10), (1, 2, 3), 1), ((9, 33, 67), (12, 35, 70), (2, 1, 1), 3),
                                        ((20, 40, 64), (20, 40, 64), (0, 0, 0), 0), ((130, 129, 130), (130, 129, 130), (0, 0, 0), 5)):     # the last: several vectors per lane
        x = rr.ct_volume(shape, -300.0, 500.0, 42, NPDT[dt])
        n = int(np.prod(shape))
        store = torch.zeros(n + 16, dtype=torch.int16 if dt == 'i16' else torch.float32, device=DEV)
        t = store[skip:skip + n].view(shape)
        t.copy_(dev(x))
        assert t.is_contiguous() and (t.data_ptr() - store.data_ptr()) == skip * store.element_size()
        nout = int(np.prod(pad_shape))
        obuf = torch.full((nout + 8,), float('nan'), device=DEV)
        out = obuf[1:1 + nout].view(pad_shape)                                                          # 4 bytes past a 16-byte boundary
        ws = torch.full((rr_ws_bytes() // 4,), float('nan'), device=DEV)
        ms = torch.full((2,), float('nan'), device=DEV)
        run_abi_zscore(t, out, off, ws, ms)
        want, m, s = rr.zscore(x)
        exact = np.zeros(pad_shape)
        exact[off[0]:off[0] + shape[0], off[1]:off[1] + shape[1], off[2]:off[2] + shape[2]] = want
        got = host(out)
        assert np.abs(got.astype(np.float64) - exact).max() <= rr.zscore_bound(x, m, s)
        assert np.array_equal(got == 0, exact == 0) and bool(torch.isnan(obuf[0])) and bool(torch.isnan(obuf[1 + nout:]).all())
        # the entry (fresh, unpoisoned buffers) gives the same bits, twice
        a, m1, s1 = normalize_ct(t, pad=(pad_shape, off))
        b, m2, s2 = normalize_ct(t, pad=(pad_shape, off))
        assert torch.equal(a, out) and torch.equal(a, b) and torch.equal(ms, torch.stack([m1, s1])) and torch.equal(ms, torch.stack([m2, s2]))


def rr_ws_bytes():
    from rsuper_amd.hip import lib
    return lib.lib().rsuper_ct_stats_workspace_bytes()


def test_preprocess_array_pads_in_the_second_launch(g):
    from rsuper_amd.inference import preprocess_array
    mean, sigma, seed = g['nz0_params']
    x = rr.ct_volume(tuple(int(v) for v in g['nz0_shape']), mean, sigma, int(seed), np.int16)
    args = argparse.Namespace(dimension='3d', training_size=g['pp_training_size'].tolist())
    for inp in (x, dev(x), dev(x.astype(np.float32)), x.astype(np.int32)):
        out, idx = preprocess_array(inp, args)
        _, m, s = rr.zscore(x)
        assert out.is_cuda and tuple(out.shape) == g['pp_out'].shape and idx == g['pp_idx'].tolist()
        assert np.abs(host(out).astype(np.float64) - g['pp_out'].astype(np.float64)).max() <= 2 * rr.zscore_bound(x, m, s)   # both sides carry the bound
        assert np.abs(host(out).astype(np.float64) - rr.pad(rr.zscore(x)[0], args.training_size)[0]).max() <= rr.zscore_bound(x, m, s)
        assert np.array_equal(host(out) == 0, g['pp_out'] == 0)


@pytest.mark.parametrize('i', range(N_PAD))
def test_fixture_pad_and_unpad(g, i):
    from rsuper_amd.inference import pad_to_training_size, unpad_img
    x = g[f'pad{i}_x']
    args = argparse.Namespace(dimension='3d', training_size=g['pad_training_size'].tolist())
    t = dev(x)
    out, idx = pad_to_training_size(t, args)
    assert idx == g[f'pad{i}_idx'].tolist() and tuple(out.shape) == g[f'pad{i}_out'].shape
    assert np.array_equal(host(out), g[f'pad{i}_out'])
    assert np.array_equal(host(unpad_img(out, idx, args)), g[f'pad{i}_unpad'])
    if tuple(out.shape) == x.shape:
        assert out is t                                                                                 # nothing short: the reference returns its argument
    with pytest.raises(NotImplementedError):
        pad_to_training_size(t, argparse.Namespace(dimension='2d', training_size=[16, 16]))


def test_cpu_tensors_raise():
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.inference import normalize_ct, pad_to_training_size, resample_image_with_gpu, postprocess_npz  # noqa: F401
    a = argparse.Namespace(dimension='3d', training_size=[8, 8, 8])
    with pytest.raises(RSuperHipError):
        normalize_ct(torch.zeros(4, 4, 4))
    with pytest.raises(RSuperHipError):
        pad_to_training_size(torch.zeros(4, 4, 4), a)
    with pytest.raises(RSuperHipError):
        resample_image_with_gpu(torch.zeros(2, 4, 4, 4), new_size=(5, 5, 5))
    with pytest.raises(NotImplementedError):
        resample_image_with_gpu(torch.zeros(4, 4, 4, device=DEV), new_size=(5, 5, 5), interp='area')
    with pytest.raises(NotImplementedError):
        torch.ops.rsuper.ct_normalize(torch.zeros(4, 4, 4), -991.0, 500.0, [4, 4, 4], [0, 0, 0], None)
    with pytest.raises(ValueError):
        resample_image_with_gpu(torch.zeros(4, 4, 4, device=DEV), new_size=(5, 5, 5), box=[4, 9, 0, 4, 0, 4])


# ---- the whole case
@pytest.fixture(scope='module')
def nets():
    from oracle import unet_oracle as uo
    from rsuper_amd.model.dim3.unet import UNet
    classes = synth.TINY_CLASSES
    net = UNet(1, 8, num_classes=len(classes), block='BasicBlock', norm='in', compute_dtype='f32')
    sd = synth.fill_state_dict(uo.unet_param_shapes(1, 8, len(classes)), 3)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return [net.to(DEV)]


def case_args(**kw):
    return argparse.Namespace(dimension='3d', training_size=[32, 32, 32], window_size=[32, 32, 32], classes=len(synth.TINY_CLASSES), **kw)


def test_predict_case_equals_the_hand_composition(nets):
    from rsuper_amd.inference import predict_case, preprocess_array, prediction, resample_image_with_gpu, postprocess_npz
    from rsuper_amd.inference.resample import resample_launches
    classes = synth.TINY_CLASSES
    assert any('lesion' in c for c in classes) and len(classes) == 5
    hu = rr.ct_volume((40, 28, 36), -200.0, 400.0, 8, np.int16)                                          # y is short: padded to 34
    args = case_args(organ_mask_on_lesion=True)
    orig_size = (45, 37, 52)                                                                            # x, y, z
    n0 = resample_launches()
    out, raw = predict_case(nets, hu, args, classes, orig_size=orig_size)
    assert resample_launches() == n0 + 2                                                                # one per output kind
    img, idx = preprocess_array(hu, args)
    assert tuple(img.shape) == (40, 34, 36) and idx == [0, 40, 3, 31, 0, 36]
    label, raw0 = prediction(nets, img, args, to_cpu=False)
    lab2 = resample_image_with_gpu(label, new_size=orig_size, interp='nearest', box=idx)
    raw2 = resample_image_with_gpu(raw0, new_size=orig_size, interp='trilinear', box=idx)
    want = postprocess_npz(lab2, classes, args)
    assert list(out) == list(want) and all(torch.equal(out[c], want[c]) for c in want)
    assert raw.dtype == torch.float32 and tuple(raw.shape) == (5, 52, 37, 45) and torch.equal(raw, raw2)
    # the label planes are raw > 0.5, resampled nearest
    lab3 = resample_image_with_gpu((raw0 > 0.5).to(torch.uint8), new_size=orig_size, interp='nearest', box=idx)
    plain, _ = predict_case(nets, hu, case_args(), classes, orig_size=orig_size)
    assert all(plain[c].dtype == torch.uint8 and torch.equal(plain[c], lab3[i]) for i, c in enumerate(classes))
    assert 0 < int(lab3.sum()) < lab3.numel()
    # the spacing form of the same grid: round(size * target / orig)
    by_spacing, _ = predict_case(nets, hu, case_args(), classes, orig_spacing=(0.8, 28.0 / 37.0, 40.0 / 52.0), target_spacing=(1., 1., 1.))
    assert all(torch.equal(by_spacing[c], plain[c]) for c in classes)


def test_predict_case_on_the_same_grid_launches_no_resample(nets):
    from rsuper_amd.inference import predict_case, preprocess_array, prediction
    from rsuper_amd.inference.resample import resample_launches
    classes = synth.TINY_CLASSES
    hu = dev(rr.ct_volume((34, 32, 40), -200.0, 400.0, 9, np.float32))
    n0 = resample_launches()
    out, raw = predict_case(nets, hu, case_args(), classes)
    assert resample_launches() == n0
    label, raw0 = prediction(nets, preprocess_array(hu, case_args())[0], case_args(), to_cpu=False)
    assert torch.equal(raw, raw0) and all(torch.equal(out[c], label[i]) for i, c in enumerate(classes))
    # padding alone (no other grid) still needs the unpad: one launch per output kind
    out2, raw2 = predict_case(nets, hu[:, 2:30], case_args(), classes)
    assert resample_launches() == n0 + 2 and tuple(raw2.shape) == (5, 34, 28, 40) and tuple(out2[classes[0]].shape) == (34, 28, 40)
