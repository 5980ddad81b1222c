"""Writes tests/golden/resample.npz by IMPORTING the unmodified reference's predict_abdomenatlas.py (SimpleITK, nibabel, pandas, matplotlib and
its own sibling packages stubbed, as SURVEY.md section 8c does for the other generators) and calling its pad_to_training_size, unpad_img,
resample_image_with_gpu and preprocess on CPU tensors.  Nothing is restated here: preprocess runs as written, on a stand-in image object whose
array is the test volume and whose spacing already equals the target spacing (so the SimpleITK resample branch is not taken), with
Tensor.cuda() mapped to the identity.

    rs{i}_*    class stacks (uint8 labels and float32 probabilities, 2-3 planes) through resample_image_with_gpu plane by plane:
               'nearest' in full; 'trilinear' (a uint8 plane goes in as .float()) at the voxels resample_ref.sample_index names -- all of them
               for the small cases -- as the reference's float32 values and exact = float64(values) + float64(delta): the float64 evaluation of
               the same formula with the float32 weights (resample_ref.resample), stored as a float32 difference (its own rounding, 2^-24 of
               1e-7, is far below every bound); sums of the whole exact output; `trilinear > threshold` of every voxel, bit-packed.
               A case is redrawn until no float64 value lies within 1e-6 of the threshold, so that comparison is exact with nothing left out.
    box_*      the sub-box case: which case, the padded shape and the odd offsets; its outputs are that case's outputs
    ns_*       new_size=None: (old_spacing, old_size, new_spacing) rows in x, y, z order -> the output shape the reference produced
    nz{i}_*    preprocess from the clip onward for int16 and float32 volumes drawn by resample_ref.ct_volume (recorded: parameters and a checksum
               of the input, float64 mean / std, the reference's float32 output and the float64 z-score at sampled voxels)
    pp_*       preprocess of the smallest volume with a training size that pads it (z short: the axis quirk), in full
    pad{i}_*   every subset of short axes for training size (16, 16, 16): input, padded array, original_idx, unpad_img of the padded array

The generator asserts what the tests rely on: the reference's float32 results lie inside 12 * 2^-24 * max|x| (trilinear) and
4 * 2^-24 * (max|clip(x)| + |mean|) / std (z-score) of the float64 evaluation.
Run from the repository root: python tests/golden/gen_golden_resample.py
"""
import argparse
import importlib
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402
import resample_ref as rr  # noqa: E402

# in -> out, z, y, x
RS_CASES = [((7, 9, 8), (11, 5, 13)), ((5, 6, 7), (5, 6, 7)), ((1, 4, 3), (3, 1, 7)), ((2, 2, 2), (1, 1, 1)), ((12, 20, 22), (30, 16, 18)),
            ((16, 17, 19), (7, 33, 10)), ((9, 1, 5), (4, 3, 2)), ((4, 4, 300), (4, 4, 77)), ((5, 3, 100), (5, 3, 333)), ((97, 5, 3), (291, 5, 3))]
BOX_CASE, BOX_PAD_SHAPE, BOX_OFFSET = 4, (17, 25, 29), (3, 1, 5)
# shape, target mean, target sigma
NZ_CASES = [((5, 7, 9), 0.0, 2000.0), ((1, 1, 2), 0.0, 2000.0), ((33, 65, 130), -200.0, 400.0), ((40, 50, 60), -900.0, 150.0),
            ((64, 128, 128), 450.0, 30.0)]
NS_CASES = [((2., 2., 2.), (6, 5, 4), (1., 1., 1.)), ((1., 1., 1.), (5, 7, 9), (2., 2., 2.)), ((0.8, 0.8, 2.5), (10, 11, 4), (1., 1., 1.)),
            ((1., 1., 1.), (13, 9, 7), (0.75, 1.5, 3.)), ((1.5, 1.5, 1.5), (3, 5, 7), (1., 1., 1.))]
PAD_TS = (16, 16, 16)


def planes_of(out):
    return 3 if int(np.prod(out)) < 1000 else 2


def import_reference():
    stubs = ['SimpleITK', 'nibabel', 'nibabel.orientations', 'pandas', 'matplotlib', 'matplotlib.pyplot', 'model', 'model.utils', 'training',
             'training.dataset', 'training.dataset.utils', 'inference', 'inference.utils', 'dataset_conversion', 'dataset_conversion.utils', 'utils']
    for name in stubs:
        sys.modules[name] = mock.MagicMock()
    sys.path.insert(0, gg.REF)
    return importlib.import_module('predict_abdomenatlas')


def ref_resample(pa, x, out, interp):
    """The reference, plane by plane; sizes travel in x, y, z order."""
    planes = []
    for p in x:
        t = torch.from_numpy(np.ascontiguousarray(p))
        if interp == 'trilinear':
            t = t.float()
        planes.append(pa.resample_image_with_gpu(t, new_size=tuple(out[::-1]), interp=interp).numpy())
    return np.stack(planes)


class _Image:
    def __init__(self, arr):
        self.arr = arr

    def GetDirection(self):
        return (1., 0., 0., 0., 1., 0., 0., 0., 1.)

    def GetSpacing(self):
        return (1., 1., 1.)


def ref_preprocess(pa, arr, training_size):
    args = argparse.Namespace(dimension='3d', training_size=list(training_size))
    with mock.patch.object(pa, 'reorient_image', lambda img, o: img), mock.patch.object(pa.sitk, 'GetArrayFromImage', lambda img: img.arr), \
            mock.patch.object(torch.Tensor, 'cuda', lambda self, *a, **k: self):
        t, idx, _, _ = pa.preprocess(_Image(arr), [1., 1., 1.], args)
    return t.numpy(), [int(v) for v in idx]


def main():
    pa = import_reference()
    out = {}
    worst_tri, worst_z = 0.0, 0.0
    for i, (sin, sout) in enumerate(RS_CASES):
        C = planes_of(sout)
        out[f'rs{i}_in'] = np.array(sin, np.int64)
        out[f'rs{i}_out'] = np.array(sout, np.int64)
        for dt, npdt in (('u8', np.uint8), ('f32', np.float32)):
            seed = 7000 + 10 * i + (npdt == np.float32)
            for _ in range(200):
                x = rr.stack(sin, C, seed, npdt)
                exact = rr.resample(x, sout, 'trilinear', np.float64)
                if np.abs(exact - rr.THRESHOLD[dt]).min() > 1e-6:
                    break
                seed += 1000
            else:
                raise RuntimeError(f'case {i} {dt}: no draw clears the threshold')
            near = ref_resample(pa, x, sout, 'nearest')
            tri = ref_resample(pa, x, sout, 'trilinear')
            assert near.dtype == npdt and tri.dtype == np.float32 and near.shape == tri.shape == (C,) + tuple(sout)
            assert np.array_equal(near, rr.resample(x, sout, 'nearest')), (i, dt)
            err = float(np.abs(tri.astype(np.float64) - exact).max())
            assert err <= rr.trilinear_bound(x), (i, dt, err)
            worst_tri = max(worst_tri, err / float(x.max()))
            assert np.array_equal(tri > np.float32(rr.THRESHOLD[dt]), exact > rr.THRESHOLD[dt])
            idx = rr.sample_index(tri.size)
            out[f'rs{i}_{dt}_x'] = x
            out[f'rs{i}_{dt}_nearest'] = near
            out[f'rs{i}_{dt}_tri'] = tri.reshape(-1)[idx]
            out[f'rs{i}_{dt}_tri_delta'] = (exact.reshape(-1)[idx] - tri.reshape(-1)[idx].astype(np.float64)).astype(np.float32)
            out[f'rs{i}_{dt}_tri_sums'] = np.array([exact.sum(), (exact * exact).sum(), np.abs(exact).max(), exact.size], np.float64)
            out[f'rs{i}_{dt}_thr'] = np.packbits((tri > np.float32(rr.THRESHOLD[dt])).reshape(-1))
    out['box_case'] = np.array([BOX_CASE], np.int64)
    out['box_pad_shape'] = np.array(BOX_PAD_SHAPE, np.int64)
    out['box_offset'] = np.array(BOX_OFFSET, np.int64)
    # the reference's unpad_img then resample equals the case's own outputs: checked here on the float32 stack, not recorded twice
    sin, sout = RS_CASES[BOX_CASE]
    x = out[f'rs{BOX_CASE}_f32_x']
    big = np.full((x.shape[0],) + BOX_PAD_SHAPE, 0.75, np.float32)
    o = BOX_OFFSET
    big[:, o[0]:o[0] + sin[0], o[1]:o[1] + sin[1], o[2]:o[2] + sin[2]] = x
    idx3 = [o[0], o[0] + sin[0], o[1], o[1] + sin[1], o[2], o[2] + sin[2]]
    a3 = argparse.Namespace(dimension='3d')
    cut = np.stack([pa.unpad_img(torch.from_numpy(p), idx3, a3).numpy() for p in big])
    assert np.array_equal(ref_resample(pa, cut, sout, 'nearest'), out[f'rs{BOX_CASE}_f32_nearest'])

    out['ns_in'] = np.array([list(a) + list(b) + list(c) for a, b, c in NS_CASES], np.float64)
    ns_out = []
    for osp, osz, nsp in NS_CASES:
        r = pa.resample_image_with_gpu(torch.zeros(tuple(osz[::-1])), old_spacing=osp, old_size=osz, new_spacing=nsp, interp='nearest')
        ns_out.append(list(r.shape))
    out['ns_out'] = np.array(ns_out, np.int64)

    for i, (shape, mean, sigma) in enumerate(NZ_CASES):
        out[f'nz{i}_shape'] = np.array(shape, np.int64)
        out[f'nz{i}_params'] = np.array([mean, sigma, 9100 + i], np.float64)
        for dt, npdt in (('i16', np.int16), ('f32', np.float32)):
            x = rr.ct_volume(shape, mean, sigma, 9100 + i, npdt)
            assert x.min() < rr.CLIP[0] and x.max() > rr.CLIP[1]
            ref, idx = ref_preprocess(pa, x, (1, 1, 1))
            assert ref.shape == tuple(shape) and idx == [0, shape[0], 0, shape[1], 0, shape[2]]
            exact, m, s = rr.zscore(x)
            err = float(np.abs(ref.astype(np.float64) - exact).max())
            assert err <= rr.zscore_bound(x, m, s), (i, dt, err, rr.zscore_bound(x, m, s))
            worst_z = max(worst_z, err)
            k = rr.sample_index(ref.size, 512, 512)
            out[f'nz{i}_{dt}_checksum'] = np.array([x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum()], np.float64)
            out[f'nz{i}_{dt}_stats'] = np.array([m, s], np.float64)
            out[f'nz{i}_{dt}_ref'] = ref.reshape(-1)[k]
            out[f'nz{i}_{dt}_ref_delta'] = (exact.reshape(-1)[k] - ref.reshape(-1)[k].astype(np.float64)).astype(np.float32)
    x = rr.ct_volume(NZ_CASES[0][0], NZ_CASES[0][1], NZ_CASES[0][2], 9100, np.int16)
    ref, idx = ref_preprocess(pa, x, (8, 8, 8))
    out['pp_training_size'] = np.array([8, 8, 8], np.int64)
    out['pp_out'] = ref
    out['pp_idx'] = np.array(idx, np.int64)

    n = 0
    for zs in (10, 20):
        for ys in (11, 20):
            for xs in (12, 18):
                x = rr.stack((zs, ys, xs), 1, 9500 + n, np.float32, levels=4)[0]
                a = argparse.Namespace(dimension='3d', training_size=list(PAD_TS))
                p, idx = pa.pad_to_training_size(torch.from_numpy(x), a)
                out[f'pad{n}_x'] = x
                out[f'pad{n}_out'] = p.numpy()
                out[f'pad{n}_idx'] = np.array(idx, np.int64)
                out[f'pad{n}_unpad'] = pa.unpad_img(p, idx, a).numpy()
                n += 1
    out['pad_training_size'] = np.array(PAD_TS, np.int64)
    path = os.path.join(HERE, 'resample.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays; worst trilinear error / max|x| {worst_tri:.3e}, worst z-score error {worst_z:.3e}')


if __name__ == '__main__':
    main()
