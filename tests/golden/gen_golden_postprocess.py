"""Writes tests/golden/postprocess.npz with scipy's literal forms of the prediction post-processing (predict_abdomenatlas.py postprocess_npz /
keep_largest_component, eval_AUC.detection):

    det_*   smooth random probability volumes -> ndimage.zoom(order=1), then per threshold binary_erosion(box3) ->
            binary_dilation(box3, iterations=2) -> AND -> count (erode) or the plain count; plus the maximum resampled value
    cc_*    masks -> ndimage.label (default, face-connected structure) -> first label of the largest size; empty -> all ones
    om_*    class stacks (5- and 42-class lists, uint8 labels and float32 probabilities) -> organ > 0.5 -> binary_dilation(box3) -> * lesion

A detection case whose resampled values lie within 1e-9 of a threshold is redrawn, so float64 summation order cannot flip a voxel.
Run from the repository root: python tests/golden/gen_golden_postprocess.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402

THRESHOLDS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
BOX = np.ones((3, 3, 3))

# (name, input shape, spacing): odd sides, sides < 3 (erosion removes everything), 1-voxel slabs, half-to-even output sides
# (5 * 0.5 -> 2, 7 * 0.5 -> 4), an n_out == 1 axis (2 * 0.5 -> 1), CT-like anisotropic spacing, and (down_big, y: 26 -> 23) a last
# output plane whose coordinate 22 * (25 / 22) rounds above 24 in f64, which ndimage's 'constant' mode sets to 0
DET_CASES = [
    ('iso_odd', (9, 11, 13), (1, 1, 1)),
    ('iso_big', (25, 31, 37), (1, 1, 1)),
    ('thin2', (2, 5, 7), (1, 1, 1)),
    ('slab_z', (1, 12, 14), (1, 1, 1)),
    ('slab_y', (10, 1, 9), (1, 1, 1)),
    ('half_even', (5, 7, 9), (0.5, 0.5, 1.0)),
    ('nout1', (2, 9, 11), (0.5, 1.0, 1.0)),
    ('ct_like', (12, 20, 22), (2.5, 0.8, 0.8)),
    ('up', (7, 9, 8), (1.5, 1.25, 2.0)),
    ('down_big', (20, 26, 30), (0.7, 0.9, 0.55)),
]


def smooth_volume(shape, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal(shape)
    x = ndimage.gaussian_filter(x, sigma=1.5, mode='nearest')
    x = (x - x.mean()) / (x.std() + 1e-12)
    return (1.0 / (1.0 + np.exp(-2.0 * x))).astype(np.float32)


def detection_literal(array, spacing, thresholds, erode):
    array = ndimage.zoom(array.astype(np.float64), np.array(spacing, np.float64) / np.ones(3), order=1)
    vols = []
    for th in thresholds:
        b = array > th
        if erode:
            a = ndimage.binary_erosion(b, structure=BOX, iterations=1)
            a = ndimage.binary_dilation(a, structure=BOX, iterations=2)
            a &= b
            vols.append(int(a.sum()))
        else:
            vols.append(int(b.sum()))
    return array, np.array(vols, np.int64), float(np.max(array))


def largest_literal(mask):
    cc, n = ndimage.label(mask > 0)
    best, best_size = 0, 0
    for i in range(1, n + 1):
        s = int((cc == i).sum())
        if s > best_size:
            best, best_size = i, s
    return (cc == best).astype(np.uint8)


def organ_literal(pred, classes):
    organs = {c: pred[i] for i, c in enumerate(classes) if 'lesion' not in c}
    out = []
    for i, c in enumerate(classes):
        if 'lesion' not in c:
            continue
        name = c.split('_')[0].replace('pancreatic', 'pancreas')
        if name == 'kidney':
            o = organs['kidney_right'] + organs['kidney_left']
        elif name == 'adrenal':
            o = organs['adrenal_gland_right'] + organs['adrenal_gland_left']
        elif name == 'lung':
            o = organs['lung_right'] + organs['lung_left']
        elif name == 'uterus':
            o = organs['prostate']
        elif name == 'gallbladder':
            o = organs['gall_bladder']
        elif name in ('bone', 'breast'):
            o = np.ones_like(organs['prostate'], dtype=np.uint8)
        else:
            o = organs[name]
        o = ndimage.binary_dilation((o > 0.5).astype(np.uint8), structure=BOX).astype(pred.dtype)
        out.append(o * pred[i])
    return np.stack(out)


def blobs(shape, n_blobs, seed):
    """Organ-like blobs: thresholded smooth noise."""
    r = np.random.default_rng(seed)
    x = ndimage.gaussian_filter(r.standard_normal(shape), sigma=2.0)
    return x > np.quantile(x, 1.0 - 0.15 * n_blobs)


def main():
    out = {}
    for k, (name, shape, spacing) in enumerate(DET_CASES):
        seed = 100 + k
        while True:
            x = smooth_volume(shape, seed)
            rs, v_e, m = detection_literal(x, spacing, THRESHOLDS, True)
            if min(np.abs(rs - t).min() for t in THRESHOLDS) > 1e-9:
                break
            seed += 1000
        _, v_n, m_n = detection_literal(x, spacing, THRESHOLDS, False)
        assert m == m_n
        out[f'det_{name}_x'] = x
        out[f'det_{name}_spacing'] = np.array(spacing, np.float64)
        out[f'det_{name}_vol_erode'] = v_e
        out[f'det_{name}_vol_plain'] = v_n
        out[f'det_{name}_max'] = np.float64(m)
    # largest component: densities around the face-connectivity percolation point, multi-tile shapes, a tie, the empty mask
    cc_cases = [('d20', (20, 24, 70), 0.2), ('d31', (24, 40, 72), 0.31), ('d50', (17, 19, 45), 0.5), ('d31_small', (5, 6, 7), 0.31)]
    for k, (name, shape, dens) in enumerate(cc_cases):
        r = np.random.default_rng(500 + k)
        m = (r.random(shape) < dens).astype(np.uint8)
        out[f'cc_{name}_mask'] = np.packbits(m.ravel())
        out[f'cc_{name}_shape'] = np.array(shape, np.int64)
        out[f'cc_{name}_out'] = np.packbits(largest_literal(m).ravel())
    tie = np.zeros((6, 10, 40), np.uint8)
    tie[1:3, 6:8, 30:33] = 1          # 12 voxels, first voxel (1, 6, 30)
    tie[0, 0, 36:40] = 1              # 4 voxels, first in C order but smaller
    tie[1:3, 2:4, 10:13] = 1          # 12 voxels, first voxel (1, 2, 10): the tie goes to this one
    for name, m in (('tie', tie), ('empty', np.zeros((4, 9, 33), np.uint8))):
        out[f'cc_{name}_mask'] = np.packbits(m.ravel())
        out[f'cc_{name}_shape'] = np.array(m.shape, np.int64)
        out[f'cc_{name}_out'] = np.packbits(largest_literal(m).ravel())
    # organ masking
    for lname, classes in (('tiny', synth.TINY_CLASSES), ('m42', synth.MASK42_CLASSES)):
        shape = (len(classes), 8, 11, 13) if lname == 'm42' else (len(classes), 13, 17, 21)
        r = np.random.default_rng(900 + len(classes))
        lab = np.stack([blobs(shape[1:], 1 + (c % 3), 1000 + c) for c in range(shape[0])]).astype(np.uint8)
        prob = np.stack([smooth_volume(shape[1:], 2000 + c) for c in range(shape[0])]) * r.random(shape).astype(np.float32)
        prob = prob.astype(np.float32)
        out[f'om_{lname}_u8'] = lab
        out[f'om_{lname}_u8_out'] = organ_literal(lab, classes)
        out[f'om_{lname}_f32'] = prob
        out[f'om_{lname}_f32_out'] = organ_literal(prob, classes)
    path = os.path.join(HERE, 'postprocess.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
