"""Writes tests/golden/pseudo_labels.npz and pseudo_labels.json by IMPORTING the unmodified reference's
baselines/pseudo_labels/pseudo_label_report_refinement.py (nibabel and tqdm stubbed in sys.modules; neither is called by what runs here, except the
nib.load / nib.save stub over .npy files that process_bdmap goes through in a temporary tree):

    calls    extract_lesion_candidates on synthetic volumes (tests/pseudo_labels_ref.py builds them): the thirteen neighbour directions, ties, rejected
             components, the float32 threshold, min_peak, two plateaus, a serpentine through every labelling tile, smooth volumes, speckle.  Per call:
             the mask (bit-packed), kept, and the number of ndimage.label passes (P.label is wrapped with a counter).
    cases    process_bdmap on seven folders of one three-class case: included, a missing id, a missing column, a NaN count, a zero count, found < n,
             a 4-D probability.  Per folder: included and the masks it wrote.
    helpers  slice_indices for every (n, parts, part) up to (7, 3); dump_yaml / load_yaml round trip.

The smooth volumes come from this project's own generator (pseudo_labels_ref.smooth_volume), not from the one behind the issue's illustrative
figures (about 250 iterations for n = 60, kept = 45 on the first volume): here n = 60 takes 198 / 85 / 89 iterations and the first volume ends with
kept = 49.  The recorded numbers are the reference's on these volumes.

The generator asserts what the issue states about these cases and that the restatement (pseudo_labels_ref.candidates) equals the reference on every
call.  Run from the repository root: python tests/golden/gen_golden_pseudo_labels.py
"""
import importlib
import json
import os
import sys
import tempfile
import types
from pathlib import Path
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402
import pseudo_labels_ref as pr  # noqa: E402

CASE_CLASSES = ['liver_lesion', 'kidney_lesion', 'pancreatic_lesion']
CASE_SHAPE = (12, 20, 24)
NAN = 'NaN'                                                  # how a NaN count is written in the JSON rows


class _Image:
    def __init__(self, data, affine=None, header=None):
        self.data, self.affine, self.header = np.asarray(data), affine, header

    def get_fdata(self, dtype=np.float64):
        return self.data.astype(dtype)


def _nib_stub():
    nib = types.ModuleType('nibabel')

    def load(path):
        with open(path, 'rb') as f:
            return _Image(np.load(f), affine=np.eye(4), header=None)

    def save(img, path):
        with open(path, 'wb') as f:
            np.save(f, img.data)

    nib.load, nib.save, nib.Nifti1Image, nib.Nifti1Header = load, save, _Image, object
    return nib


def import_reference():
    sys.modules['nibabel'] = _nib_stub()
    sys.modules['tqdm'] = mock.MagicMock()
    sys.path.insert(0, os.path.join(gg.REF, 'baselines', 'pseudo_labels'))
    P = importlib.import_module('pseudo_label_report_refinement')
    passes = [0]
    label = P.label

    def counted(*a, **k):
        passes[0] += 1
        return label(*a, **k)

    P.label = counted
    return P, passes


def blob(shape, centre, sigma, height):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    r2 = (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2
    return height * np.exp(-r2 / (2.0 * sigma ** 2))


def case_volume():
    liver = blob(CASE_SHAPE, (3, 5, 6), 1.6, 0.9) + blob(CASE_SHAPE, (8, 14, 17), 1.8, 0.7)
    kidney = blob(CASE_SHAPE, (6, 10, 12), 2.0, 0.8)
    pancreas = blob(CASE_SHAPE, (5, 6, 18), 1.5, 0.6)
    return np.stack([liver, kidney, pancreas]).astype(np.float32)


def case_rows():
    col = {c: 'number of %s lesion instances' % c.split('_')[0] for c in CASE_CLASSES}
    full = {col['liver_lesion']: 2, col['kidney_lesion']: 1, col['pancreatic_lesion']: 1, 'sex': 'F'}
    rows = {
        'BDMAP_00000001': dict(full),
        'BDMAP_00000002': None,                              # the id is missing from the metadata
        'BDMAP_00000003': {k: v for k, v in full.items() if k != col['pancreatic_lesion']},
        'BDMAP_00000004': dict(full, **{col['kidney_lesion']: NAN}),
        'BDMAP_00000005': dict(full, **{col['kidney_lesion']: 0}),
        'BDMAP_00000006': dict(full, **{col['pancreatic_lesion']: 9}),           # more than the volume yields
        'BDMAP_00000007': dict(full),                        # stored as (D, H, W, 2): the reference takes [..., 0]
    }
    return rows


def main():
    P, passes = import_reference()
    arrays, calls = {}, []

    def call(name, key, x, n, peak_cut=0.40, min_voxels=11, min_peak=0.01):
        if key + '_x' not in arrays:
            arrays[key + '_x'] = x
        before = x.copy()
        passes[0] = 0
        mask, kept = P.extract_lesion_candidates(x, n, peak_cut, min_voxels, min_peak)
        its = passes[0]
        assert np.array_equal(x, before) and mask.dtype == np.uint8
        rm, rk, ri = pr.candidates(x, n, peak_cut, min_voxels, min_peak)
        assert np.array_equal(rm, mask) and (rk, ri) == (kept, its), name
        arrays[name + '_mask'] = np.packbits(mask.reshape(-1))
        calls.append({'name': name, 'input': key, 'n_lesions': n, 'peak_cut': peak_cut, 'min_voxels': min_voxels, 'min_peak': min_peak,
                      'kept': int(kept), 'iterations': int(its), 'voxels': int(mask.sum())})
        return mask, kept, its

    for i, d in enumerate(pr.DIRECTIONS):
        x = pr.direction_volume(d)
        m, k, it = call('dir_%d' % i, 'dir_%d' % i, x, 1)
        assert k == 1 and it == 1 and m.sum() == 12 and np.array_equal(m > 0, x > 0), d
    assert len(pr.DIRECTIONS) == 13

    x = pr.ties_volume()
    m, k, it = call('ties', 'ties', x, 1)
    assert k == 1 and it == 1 and m.sum() == 12 and m[0:2, 0:3, 0:2].all()

    x = pr.reject_volume()
    want = {(1, 11): (1, 11, 2), (2, 11): (2, 51, 3), (3, 11): (2, 51, 3), (2, 10): (2, 21, 2)}
    for n, mv in pr.REJECT_CALLS:
        m, k, it = call('reject_n%d_v%d' % (n, mv), 'reject', x, n, min_voxels=mv)
        assert (k, int(m.sum()), it) == want[(n, mv)], (n, mv, k, m.sum(), it)

    x = pr.bridge_volume()
    m, k, it = call('bridge32', 'bridge32', x, 1, min_voxels=7)
    assert k == 1 and m.sum() == 7

    m, k, it = call('minpeak_eq', 'minpeak_eq', pr.minpeak_volume(False), 1)
    assert k == 1 and it == 1 and m.sum() == 12
    m, k, it = call('minpeak_lt', 'minpeak_lt', pr.minpeak_volume(True), 1)
    assert k == 0 and it == 0 and m.sum() == 0

    m, k, it = call('zero', 'ties', pr.ties_volume(), 0)
    assert k == 0 and it == 0 and m.sum() == 0

    x = pr.plateau_volume()
    m, k, it = call('plateau', 'plateau', x, 2)
    xs = np.nonzero(m)[2]
    assert k == 2 and m.sum() == 64 and xs.min() == 2 and xs.max() == 65
    m1 = P.extract_lesion_candidates(x, 1)[0]
    assert m1.sum() == 32 and np.nonzero(m1)[2].max() == 33                     # the first peak alone stops at the valley

    x = pr.snake_volume()
    m, k, it = call('snake', 'snake', x, 1)
    assert k == 1 and it == 1 and m.sum() == 5759 and np.array_equal(m > 0, pr.snake_support())

    long_runs = 0
    for i, shape in enumerate(pr.SMOOTH_SHAPES):
        x = pr.smooth_volume(shape, 100 + i)
        for j, (n, pc, mv, mp) in enumerate(pr.SMOOTH_PARAMS):
            m, k, it = call('smooth_%d_%d' % (i, j), 'smooth_%d' % i, x, n, pc, mv, mp)
            assert it <= 400, (i, j, it)
            long_runs += it >= 60
            if j == 2:
                print('smooth', shape, 'n = 60: kept', k, 'iterations', it)
    assert long_runs >= 2
    assert [c for c in calls if c['name'] == 'smooth_0_2'][0]['kept'] < 60        # the small volume runs dry before the count is reached

    x = pr.speckle_volume()
    m, k, it = call('speckle', 'speckle', x, 5, peak_cut=0.6)
    print('speckle: kept', k, 'iterations', it, 'voxels', int(m.sum()))
    assert (k, it, int(m.sum())) == (5, 49, 69)

    # ---- process_bdmap on a temporary tree ---------------------------------------------------------------------------------------------------
    raw = case_volume()
    arrays['case_raw'] = raw
    rows = case_rows()
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        root, out_nii, out_npz = Path(tmp) / 'in', Path(tmp) / 'nii', Path(tmp) / 'npz'
        meta = {}
        for bid, row in rows.items():
            d = root / (bid + '.npz') / 'predictions_raw'
            d.mkdir(parents=True)
            for c, cname in enumerate(CASE_CLASSES):
                vol = raw[c]
                if bid == 'BDMAP_00000007':
                    vol = np.stack([vol, 1.0 - vol], axis=-1)
                with open(d / (cname + '.nii.gz'), 'wb') as f:
                    np.save(f, vol)
            if row is not None:
                meta[bid] = {k: (float('nan') if v == NAN else v) for k, v in row.items()}
        for bid, row in rows.items():
            got_id, included = P.process_bdmap(str(root / (bid + '.npz')), meta, str(out_nii), str(out_npz), str(root))
            assert got_id == bid
            written = {}
            if (out_npz / bid).exists():
                for f in sorted((out_npz / bid).iterdir()):
                    written[f.name[:-len('.npz')]] = np.load(f)['mask']
            assert included or not written
            for cname, mask in written.items():
                assert mask.dtype == np.uint8 and mask.shape == CASE_SHAPE
                arrays['case_%s_%s' % (bid, cname)] = np.packbits(mask.reshape(-1))
            cases.append({'id': bid, 'row': row, 'included': bool(included), 'masks': sorted(written), 'four_d': bid == 'BDMAP_00000007'})
    by_id = {c['id']: c for c in cases}
    assert [c['included'] for c in cases] == [True, False, False, False, True, False, True], cases
    assert by_id['BDMAP_00000001']['masks'] == sorted(CASE_CLASSES) and by_id['BDMAP_00000005']['masks'] == ['liver_lesion', 'pancreatic_lesion']
    for cname in CASE_CLASSES:
        assert np.array_equal(arrays['case_BDMAP_00000001_' + cname], arrays['case_BDMAP_00000007_' + cname])

    # ---- helpers -----------------------------------------------------------------------------------------------------------------------------
    slices = []
    for n in range(0, 8):
        for parts in range(1, 4):
            for part in range(parts):
                s = P.slice_indices(n, parts, part)
                slices.append([n, parts, part, s.start, s.stop])
    names = ['BDMAP_00000012', 'BDMAP_A0000003', 'BDMAP_00000001']
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / 'list' / 'dataset.yaml'
        P.dump_yaml(path, names)
        text = path.read_text()
        assert P.load_yaml(path) == set(names) and P.load_yaml(Path(tmp) / 'none.yaml') == set()

    np.savez_compressed(os.path.join(HERE, 'pseudo_labels.npz'), **arrays)
    with open(os.path.join(HERE, 'pseudo_labels.json'), 'w') as f:
        json.dump({'numpy': np.__version__, 'scipy': importlib.import_module('scipy').__version__, 'calls': calls,
                   'case': {'classes': CASE_CLASSES, 'shape': list(CASE_SHAPE), 'folders': cases},
                   'slices': slices, 'yaml': {'names': names, 'text': text}}, f, indent=1)
    size = os.path.getsize(os.path.join(HERE, 'pseudo_labels.npz'))
    print('%d calls, %d folders, pseudo_labels.npz %d bytes' % (len(calls), len(cases), size))
    assert size <= 1 << 20


if __name__ == '__main__':
    main()
