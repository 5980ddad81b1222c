#!/usr/bin/env python3
"""Golden vectors for the report-annotated crop, produced by the UNMODIFIED reference `AbdomenAtlasDataset` (training/dataset/dim3/
dataset_abdomenatlas_UFO.py: crop :836, get_tumor_segment_labels :647, assign_labels :1154, get_chosen_segment_mask :808, estimate_tumor_volume
:1335) and `training/augmentation.py` (crop_foreground_3d :790, denoise_mask :746, pad_volume_pair :1023) under seeded `random`, numpy and torch
generators.  Run in the authoring container only (it needs the reference, pandas and scipy):

    RSUPER_REFERENCE=<checkout of the reference>/rsuper_train python tests/golden/gen_golden_report_crop.py

Import shims as in gen_golden_crop.py / gen_golden_loader.py; the dataset object is created without __init__ and `read_report` returns a DataFrame
of the case's rows.  Writes tests/golden/report_crop.npz.  Inputs are NOT stored: `case_inputs` regenerates them (the tests import it).  The image
is 1 + the voxel's linear index, so a crop gives its own corner.

The reference builds its option lists through list(set(...)), whose order is the hash order of the process; this repository sorts them
(dataset/reports.py).  The generator asserts that, for its cases, the reference's lists came out in sorted order and asks for another
PYTHONHASHSEED otherwise.

npz: `cases` = JSON list, one record per CASES entry: entered (functions entered, in order), draws (every random.choice / random.randint /
np.random.random up to the end of crop(), with arguments and result), next (the next draw of the three generators after crop()), selected (the
chosen segment, or 'random'), fg ([count, bbox] of the foreground of every crop_foreground_3d call, padded coordinates), opened (the same after
every denoise_mask), outcomes (what every crop_foreground_3d call returned: 'crop' or its string), corner, unk_channels, sums / sha (per-class voxel
sums and SHA-256 of np.packbits(axis=0) for label / unk / mask), sums_ufo / sha_ufo (the same of the cropped classes_UFO label), volumes, diameters,
error (the exception type of a step that raised), affine (the fallback resampled the crop).  The fallback cases' seeds are chosen so that the plain
crop is taken (check_branch asserts it): their corners and volumes are pinned like the others'.  `segments` = JSON: get_tumor_segment_labels' dict
for SEGMENT_ROWS."""
import contextlib
import hashlib
import importlib
import io
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float('nan')

_ORGANS = ['spleen', 'aorta', 'stomach']
_MORE = ['gall_bladder', 'postcava', 'adrenal_gland_left', 'adrenal_gland_right', 'esophagus', 'duodenum', 'colon', 'bladder', 'prostate',
         'lung_left', 'lung_right']
_LIVER = ['liver_segment_%d' % i for i in range(1, 9)]
_PANCREAS = ['pancreas_head', 'pancreas_body', 'pancreas_tail']
_KIDNEY = ['kidney_left', 'kidney_right']
_LESIONS = ['liver_lesion', 'pancreatic_lesion', 'kidney_lesion']
_UNKNOWN = ['femur_left', 'femur_right', 'hepatic_vessel', 'portal_vein_and_splenic_vein', 'celiac_trunk', 'superior_mesenteric_artery', 'veins',
            'intestine', 'rectum']
CLASSES_UFO = {9: ['background'] + _PANCREAS + _KIDNEY + _ORGANS,
               17: ['background'] + _LIVER[:7] + _PANCREAS + _KIDNEY + _ORGANS + _LIVER[7:],     # the liver's set spans byte planes 0 and 2
               28: ['background'] + _LIVER + _PANCREAS + _KIDNEY + _ORGANS + _MORE}
CLASSES = {9: CLASSES_UFO[9] + ['pancreatic_lesion'],
           17: CLASSES_UFO[17] + ['liver', 'pancreas'] + _LESIONS + _UNKNOWN[:4],
           28: CLASSES_UFO[28] + ['liver', 'pancreas'] + _LESIONS + _UNKNOWN}
TUMOR_CLASS_NAMES = ['kidney_lesion', 'spleen']             # the fallbacks' foreground: kidney_right, kidney_left, spleen (in every class list)
assert [len(CLASSES[k]) for k in (9, 17, 28)] == [10, 26, 42] and [len(CLASSES_UFO[k]) for k in (9, 17, 28)] == [9, 17, 28]
ARGS = dict(scale=0.3, rotate=45, translate=0.1)

SIZE, CROP = (40, 48, 56), (20, 24, 28)                      # padded to (40, 64, 68): two axes
ROOMY, SMALL_CROP = (40, 56, 60), (12, 14, 16)               # no padding: (32, 54, 56) fits
ONE_AXIS, THREE_AXES = (44, 70, 60), (30, 48, 56)


def ell(c, r):
    return ('ell', tuple(c), tuple(r))


def box(lo, hi):
    return ('box', tuple(lo), tuple(hi))


def R(organ, loc, size):
    return {'Standardized Organ': organ, 'Standardized Location': loc, 'Tumor Size (mm)': size}


def K(name, seed, ufo, rows, shapes, size=SIZE, crop=CROP, expect=None):
    return dict(name=name, seed=seed, ufo=ufo, rows=rows, shapes=shapes, size=size, crop=crop, expect=expect)


_BLOB = [ell((18, 22, 30), (6, 7, 8)), box((35, 3, 50), (37, 5, 52)), box((18, 22, 30), (19, 23, 55))]    # ellipsoid + 2^3 speck + one-voxel spur
_STR_LIVER = [R('pancreas', 'head', 'u'), R('liver', 'head', '15')]
_TWO_KIDNEYS = [R('kidney', 'left', '10'), R('kidney', 'right', '12 x 8')]
CASES = [
    K('no_rows', 0, 9, None, {'pancreas_head': [ell((10, 20, 20), (3, 4, 5))]}, expect='random_crop_on_tumor'),
    K('gate', 7, 9, [R('pancreas', 'head', '12')], {'pancreas_head': [ell((10, 20, 20), (3, 4, 5))]}, expect='random_crop'),
    K('one_name', 1, 9, [R('pancreas', 'head', '12')], {'pancreas_head': [ell((10, 20, 20), (3, 4, 5))], 'spleen': [ell((30, 30, 30), (5, 6, 7))]},
      expect='fits'),
    K('pair', 2, 17, [R('pancreas', 'head / body', '10 x 12'), R('pancreas', 'body', '7 x 8 x 9')],
      {'pancreas_head': [ell((12, 20, 20), (3, 4, 5))], 'pancreas_body': [ell((14, 26, 27), (3, 4, 5))], 'pancreas_tail': [ell((30, 30, 40), (3, 3, 3))]},
      expect='fits'),
    K('pancreas_list', 3, 28, [R('pancreas', 'pancreas', '22')],
      {'pancreas_head': [ell((12, 20, 20), (3, 4, 5))], 'pancreas_body': [ell((14, 26, 27), (3, 4, 5))], 'pancreas_tail': [ell((16, 30, 34), (3, 3, 4))],
       'liver_segment_8': [ell((30, 12, 12), (4, 5, 6))]}, expect='fits'),
    K('liver_str_open', 4, 17, _STR_LIVER,
      {'liver_segment_1': _BLOB[:1], 'liver_segment_8': _BLOB[1:2], 'liver_segment_3': _BLOB[2:], 'pancreas_head': [ell((30, 40, 12), (3, 4, 5))]},
      expect='opened'),
    K('pancreas_str', 5, 28, [R('liver', 'segment 1', 'u'), R('pancreas', 'segment 1', '12')],
      {'pancreas_head': [ell((12, 20, 20), (2, 3, 3))], 'pancreas_tail': [ell((14, 24, 24), (2, 2, 3))]}, size=ROOMY, crop=SMALL_CROP, expect='fits'),
    K('empty_then_second', 6, 17, _TWO_KIDNEYS, {'kidney_%s': [ell((20, 20, 20), (4, 5, 6))]}, expect='second_mask'),
    K('empty_no_option', 0, 9, [R('kidney', 'left', '10')], {'kidney_right': [ell((20, 20, 20), (4, 5, 6))]}, expect='empty'),
    K('no_fit_then_second', 8, 17, _TWO_KIDNEYS, {'kidney_%s': [box((4, 4, 4), (34, 44, 52))], 'kidney_%s2': [ell((20, 20, 20), (4, 5, 6))]},
      expect='retry'),
    K('zero_after_open', 0, 9, [R('kidney', 'right', '10')], {'kidney_right': [box((5, 5, 5), (6, 45, 50))]}, expect='zero'),
    K('tie', 10, 28, [R('kidney', 'left', '9')], {'kidney_left': [box((4, 30, 40), (11, 37, 47)), box((12, 6, 8), (19, 13, 15)),
                                                                 box((4, 30, 48), (5, 31, 54))]}, expect='tie'),
    K('pad_one_axis', 11, 17, [R('liver', 'segment 2 / segment 8', '30'), R('kidney', 'u', '5')],
      {'liver_segment_2': [ell((20, 30, 30), (5, 6, 7))], 'liver_segment_8': [ell((24, 36, 36), (4, 5, 6))], 'kidney_left': [ell((8, 10, 10), (3, 3, 3))]},
      size=ONE_AXIS, expect='fits'),
    K('pad_three_axes', 0, 28, [R('pancreas', 'tail', 'multiple'), R('liver', 'segment 5', '14 x 9'), R('liver', 'segment 5', NAN)],
      {'liver_segment_5': [ell((15, 24, 28), (5, 6, 7))], 'pancreas_tail': [ell((8, 10, 10), (3, 3, 3))]}, size=THREE_AXES, expect='random_crop_on_tumor'),
    K('pad_three_axes_fit', 13, 28, [R('liver', 'segment 5', '14 x 9'), R('pancreas', 'tail', '11')],
      {'liver_segment_5': [ell((15, 24, 28), (5, 6, 7))], 'pancreas_tail': [ell((8, 10, 10), (3, 3, 3))]}, size=THREE_AXES, expect='fits'),
]
SEGMENT_ROWS = [c['rows'] for c in CASES] + [
    [R('liver', 'segment 1 / segment 2', '10'), R('liver', 'segment 2 / segment 3', 'u'), R('liver', 'segment 7', '5')],
    [R('pancreas', 'head', '12'), R('pancreas', 'u', '10'), R('kidney', 'left', '8')],
    [R('kidney', 'left', 'multiple'), R('kidney', 'right', '10'), R('liver', NAN, '10'), R('u', 'segment 4', '3')],
    [R('pancreas', 'head / body', NAN), R('pancreas', 'tail', '4 x 5')],
]


def _draw_case_choice(case):
    """The index random.choice(2 options) gives first under the case's seed, after the gate's np draw (which random does not see)."""
    return random.Random(case['seed']).choice([0, 1])


def case_inputs(case):
    """-> (image (D, H, W) f32 = 1 + linear index, label (C_ufo, D, H, W) bool, rows).  A class name with '%s' is kidney_left / kidney_right: '%s' is the
    side random.choice draws first under the case's seed, '%s2' the other one."""
    D, H, W = case['size']
    names = CLASSES_UFO[case['ufo']]
    img = (1 + np.arange(D * H * W, dtype=np.float32)).reshape(D, H, W)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    lab = np.zeros((len(names), D, H, W), bool)
    first = ('left', 'right')[_draw_case_choice(case)]
    other = 'right' if first == 'left' else 'left'
    for name, shapes in case['shapes'].items():
        name = name.replace('%s2', other).replace('%s', first)
        for kind, a, b in shapes:
            if kind == 'ell':
                lab[names.index(name)] |= ((z - a[0]) / b[0]) ** 2 + ((y - a[1]) / b[1]) ** 2 + ((x - a[2]) / b[2]) ** 2 < 1.0
            else:
                lab[names.index(name), a[0]:b[0], a[1]:b[1], a[2]:b[2]] = True
    if case['name'] in ('empty_then_second',):                    # the side drawn first is empty, the other one is there
        lab[names.index('kidney_' + other)] = lab[names.index('kidney_' + first)]
        lab[names.index('kidney_' + first)] = False
    return img, lab, case['rows']


def count_bbox(m):
    m = np.asarray(m) != 0
    if not m.any():
        return [0, list(m.shape) + [-1, -1, -1]]
    idx = np.nonzero(m)
    return [int(m.sum()), [int(i.min()) for i in idx] + [int(i.max()) for i in idx]]


def sha(vol):
    return hashlib.sha256(np.packbits(np.asarray(vol) != 0, axis=0).tobytes()).hexdigest()


def import_reference():
    ref = os.environ.get('RSUPER_REFERENCE')
    if not ref or not os.path.isdir(ref):
        raise SystemExit('set RSUPER_REFERENCE to the reference checkout\'s rsuper_train directory')
    for name in ('SimpleITK', 'nibabel', 'torchvision', 'torchvision.transforms'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.path.insert(0, ref)
    return importlib.import_module('training.dataset.dim3.dataset_abdomenatlas_UFO'), importlib.import_module('training.augmentation')


def run_case(refds, aug, case):
    import pandas as pd
    sys.path.insert(0, HERE)
    import gen_golden_crop as GC
    img, lab, rows = case_inputs(case)
    d, h, w = case['crop']
    ds = object.__new__(refds.AbdomenAtlasDataset)
    ds.classes, ds.classes_UFO, ds.num_classes = CLASSES[case['ufo']], CLASSES_UFO[case['ufo']], len(CLASSES[case['ufo']])
    ds.tumor_class_names, ds.lesion_classes = TUMOR_CLASS_NAMES, []
    ds.args = types.SimpleNamespace(no_pancreas_subseg=False, pancreas_only=False, aug_device='cpu', training_size=[d, h, w], proc_idx=0, **ARGS)
    ds.img_list, ds.tumor_annotated_seg, ds.UFO_paths = ['case.npy'], {'case.npy': False}, ['case.npy']
    ds.current_sample, ds.zero_masks, ds.crop_on_tumor = 'case.npy', {}, True
    ds.read_report = lambda idx: None if rows is None else pd.DataFrame(rows)
    rec = dict(name=case['name'], entered=[], draws=[], fg=[], opened=[], outcomes=[], error={})
    size = case['size']
    full = [max(s, c + m) for s, c, m in zip(size, (d, h, w), (20, 40, 40))]

    def spy(owner, name, after=None):
        orig = getattr(owner, name)

        def f(*a, **kw):
            rec['entered'].append(name)
            r = orig(*a, **kw)
            if after:
                after(r, a, kw)
            return r
        setattr(owner, name, f)
        return orig

    saved = [(ds, n, spy(ds, n)) for n in ('random_crop_on_tumor', 'random_crop', 'get_random_tumor_seg_mask')]
    saved.append((aug, 'crop_foreground_3d', spy(aug, 'crop_foreground_3d', lambda r, a, kw: (
        rec['fg'].append(count_bbox(kw['foreground'].reshape(full))), rec['outcomes'].append('crop' if isinstance(r, tuple) else r)))))
    saved.append((aug, 'denoise_mask', spy(aug, 'denoise_mask', lambda r, a, kw: rec['opened'].append(count_bbox(r)))))
    o_affine = aug.random_scale_rotate_translate_3d
    rec['affine'] = False

    def affine(*a, **kw):
        rec['affine'] = True
        return o_affine(*a, **kw)
    aug.random_scale_rotate_translate_3d = affine
    saved.append((aug, 'random_scale_rotate_translate_3d', o_affine))
    o_choice, o_randint, o_nprandom = random.choice, random.randint, np.random.random
    armed = [True]

    def choice(seq):
        r = o_choice(seq)
        if armed[0]:
            rec['draws'].append(['choice', len(seq), list(seq).index(r)])
            ordered = sorted(seq, key=lambda s: s if isinstance(s, str) else sorted(s))
            assert [sorted(s) if isinstance(s, list) else s for s in seq] == [sorted(s) if isinstance(s, list) else s for s in ordered], \
                'the reference listed %s: rerun with another PYTHONHASHSEED' % (seq,)
        return r

    def randint(a, b):
        r = o_randint(a, b)
        if armed[0]:
            rec['draws'].append(['randint', a, b, r])
        return r

    def nprandom(*a):
        r = o_nprandom(*a)
        if armed[0] and not a:
            rec['draws'].append(['np.random', float(r)])
        return r
    random.choice, random.randint, np.random.random = choice, randint, nprandom
    random.seed(case['seed'])
    np.random.seed(case['seed'])
    torch.manual_seed(case['seed'])
    cwd = os.getcwd()
    try:
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
            os.chdir(tmp)                                          # crop() writes zero_masks.yaml where it stands
            timg = torch.from_numpy(img)[None, None]
            tlab = torch.from_numpy(lab.astype(np.uint8))[None]
            timg, tlab = aug.pad_volume_pair(timg, tlab, d + 20, h + 40, w + 40)
            assert list(timg.shape[2:]) == full
            segments, _ = ds.get_tumor_segment_labels(0)
            timg, tlab, _, selected = ds.crop(timg, tlab, 0, d, h, w)
            armed[0] = False
            rec['next'] = {'np': float(o_nprandom()), 'random': random.random(), 'torch': float(torch.rand(1))}
            rec['selected'] = selected
            if not rec['affine']:                                  # a resampled crop is crop.npz's business; a plain one is pinned here, fallbacks included
                rec['corner'] = GC.corner_of(timg.numpy(), full, size)
                lo = [(f - s) // 2 for f, s in zip(full, size)]
                padded = np.zeros(full, np.float32)
                padded[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = img
                c = rec['corner']
                assert np.array_equal(timg.numpy()[0, 0], padded[c[0]:c[0] + d, c[1]:c[1] + h, c[2]:c[2] + w])
                tlab = tlab.squeeze(0)
                rec['sums_ufo'], rec['sha_ufo'] = [int(v) for v in tlab.sum((1, 2, 3))], sha(tlab.numpy())
                try:
                    label, unk, unk_t = ds.assign_labels(tlab, 0)
                    rec['unk_channels'] = unk
                    rec['sums'] = {'label': [int(v) for v in label.sum((1, 2, 3))], 'unk': [int(v) for v in unk_t.sum((1, 2, 3))]}
                    rec['sha'] = {'label': sha(label.numpy()), 'unk': sha(unk_t.numpy())}
                except Exception as e:                             # noqa: BLE001
                    rec['error']['assign_labels'] = type(e).__name__
            if selected != 'random':
                assert not rec['affine']
                v, dm = ds.estimate_tumor_volume(0, selected)
                rec['volumes'], rec['diameters'] = [float(x) for x in torch.tensor(v).float()], dm.float().numpy().tolist()
                if 'assign_labels' not in rec['error']:
                    try:
                        mask = ds.get_chosen_segment_mask(label, selected)
                        rec['sums']['mask'], rec['sha']['mask'] = [int(x) for x in mask.sum((1, 2, 3))], sha(mask.numpy())
                    except Exception as e:                         # noqa: BLE001
                        rec['error']['get_chosen_segment_mask'] = type(e).__name__
    finally:
        os.chdir(cwd)
        random.choice, random.randint, np.random.random = o_choice, o_randint, o_nprandom
        for owner, n, orig in saved:
            if owner is ds:
                continue
            setattr(owner, n, orig)
    rec['segments'] = segments
    return rec


def check_branch(case, rec):
    """Every case must reach the branch it was written for; a fallback case must take the plain (not the affine) crop, so that its volumes are pinned."""
    e, ent, out, name = case['expect'], rec['entered'], rec['outcomes'], case['name']
    choices = [d for d in rec['draws'] if d[0] == 'choice']
    if e in ('random_crop_on_tumor', 'random_crop'):
        ok = rec['selected'] == 'random' and ent == [e] and not rec['affine'] and (e != 'random_crop' or rec['draws'][0][1] < 0.1)
        if name == 'no_rows':
            ok = ok and case['rows'] is None and not choices
    elif e == 'fits':
        ok = out == ['crop'] and not rec['opened'] and len(choices) == 1
    elif e == 'opened':
        ok = out == ['crop'] and len(rec['opened']) == 1 and rec['opened'][0][0] > 0
    elif e == 'second_mask':
        ok = ent[:3] == ['get_random_tumor_seg_mask'] * 2 + ['crop_foreground_3d'] and out == ['crop'] and len(choices) == 2
    elif e == 'empty':
        ok = ent == ['get_random_tumor_seg_mask', 'random_crop_on_tumor'] and rec['selected'] == 'random' and not rec['affine'] and len(choices) == 1
    elif e == 'retry':
        ok = out == ['mask does not fit crop size', 'crop'] and len(rec['opened']) == 1 and rec['opened'][0][0] > 0 and len(choices) == 2
    elif e == 'zero':
        ok = (out == ['zero mask'] and rec['opened'] == [[0, list(rec_full(case)) + [-1, -1, -1]]] and ent[-1] == 'random_crop_on_tumor'
              and not rec['affine'])
    elif e == 'tie':
        # two 7^3 boxes: the opening leaves 2 x 63 voxels, the component step 63, and the box at z = 4 comes first in C order
        img, lab, _ = case_inputs(case)
        from scipy.ndimage import binary_dilation, binary_erosion, label
        m = lab[CLASSES_UFO[case['ufo']].index('kidney_left')]
        _, n = label(binary_dilation(binary_erosion(m, iterations=3), iterations=3) & m)
        counts = np.bincount(label(binary_dilation(binary_erosion(m, iterations=3), iterations=3) & m)[0].ravel())[1:]
        ok = out == ['crop'] and n == 2 and counts[0] == counts[1] == rec['opened'][0][0] and rec['opened'][0][1][0] == 4
    else:
        raise AssertionError('unknown expectation %r' % (e,))
    if name == 'pancreas_list':
        ok = ok and rec['selected'] == ['pancreas'] and len([v for v in rec['sums_ufo'] if v]) >= 3 and rec['error'] == {'assign_labels': 'KeyError'}
    if name in ('liver_str_open', 'pancreas_str'):                  # an organ name as a plain string: expanded for the mask, iterated by character later
        ok = ok and rec['selected'] == name.split('_')[0] and rec['error'] == {'get_chosen_segment_mask': 'AssertionError'}
        ok = ok and len([v for v in rec['sums_ufo'] if v]) >= 2
    if name == 'pair':
        ok = ok and sorted(rec['selected']) == ['body', 'head']
    if name == 'one_name':
        ok = ok and rec['selected'] == ['head']
    assert ok, (name, {k: v for k, v in rec.items() if k != 'segments'})


def rec_full(case):
    return [max(s, c + m) for s, c, m in zip(case['size'], case['crop'], (20, 40, 40))]


def main():
    refds, aug = import_reference()
    import pandas as pd
    recs = []
    for case in CASES:
        rec = run_case(refds, aug, case)
        check_branch(case, rec)
        recs.append(rec)
        print(case['name'], rec['entered'], rec['outcomes'], rec['selected'], rec.get('corner'), rec['error'])
    names = {c['name'] for c in CASES}
    assert {c['ufo'] for c in CASES} == {9, 17, 28}
    assert any(isinstance(r['selected'], list) and len(r['selected']) == 1 for r in recs) and any(isinstance(r['selected'], list) and len(r['selected']) == 2 for r in recs)
    pads = [sum(s < f for s, f in zip(c['size'], rec_full(c))) for c in CASES]
    assert {0, 1, 2, 3} <= set(pads), pads
    ds = object.__new__(refds.AbdomenAtlasDataset)
    ds.args = types.SimpleNamespace(no_pancreas_subseg=False)
    segs = []
    for rows in SEGMENT_ROWS:
        ds.read_report = lambda idx, rows=rows: None if rows is None else pd.DataFrame(rows)
        segs.append(ds.get_tumor_segment_labels(0)[0])
    path = os.path.join(HERE, 'report_crop.npz')
    np.savez_compressed(path, cases=np.array(json.dumps(recs)), segments=np.array(json.dumps(segs)))
    print('wrote', path, os.path.getsize(path), 'bytes', len(names), 'cases')


if __name__ == '__main__':
    main()
