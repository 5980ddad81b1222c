#!/usr/bin/env python3
"""Golden vectors for crop-on-tumour, produced by the UNMODIFIED reference `training/augmentation.py` (random_crop_on_tumor :600, negative_crop
:662, organ_crop :675, tumor_crop :716, crop_around_coordinate_3d :498, pad_volume_pair :1023, crop_3d :446) under seeded numpy and torch
generators.  Run in the authoring container only:

    RSUPER_REFERENCE=<checkout of the reference>/rsuper_train python tests/golden/gen_golden_crop.py

Import shims as in gen_golden_augment.py.  Writes tests/golden/crop.npz.  Inputs are NOT stored: `case_inputs` below regenerates them (the tests
import it).  The image holds 1 + the voxel's own linear index as float32 (exact below 2^24; the padding pad_volume_pair adds is 0), so any
non-zero voxel of a returned crop gives the crop's corner; the generator asserts that every reference crop equals the (padded) input sliced there.

Per case k (CASES[k]):
  seed_k, args_k   the seed of both generators and the case's arguments (the CASES entry as JSON)
  calls_k    the reference functions entered, in order, joined by '>' ('tumor_crop', 'negative_crop', 'organ_crop', then 'crop_3d' on a fallback)
  organ_k    crop_organ as return_crop_organ gives it (-1 = 'random'); -2 where the function does not return one
  center_k   the coordinate handed to crop_around_coordinate_3d (padded coordinates), (-1, -1, -1) on a fallback
  rank_k, count_k   the centre's position in torch.nonzero of the chosen mask and that mask's voxel count (-1 on a fallback)
  tdraws_k   (n, 2): high and result of every torch.randint;  ndraws_k  (n, 3): low, high and result of every np.random.randint
  origin_k   the crop's corner in padded coordinates;  padded_k  the shape pad_volume_pair returned
  next_np_k, next_torch_k   the next np.random.random() / torch.rand(1) after the call: pin the draws consumed
wrap_*: the dataset wrapper (dataset_abdomenatlas_UFO.py:580-631) restated with the reference functions for WRAP_LEN consecutive samples under one
seed: the 0.4 branch, the corner of the (large or direct) crop and, for the large branch, the theta drawn after it.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SIZE, CROP = (41, 53, 67), (24, 28, 32)
FOREGROUND = [0, 1, 2]
SMALL_ONE, SMALL_ALL = (49, 20, 79), (18, 20, 25)        # smaller than the large crop (44, 68, 72) of CROP in one axis / in all three


def lesion_of(classes):
    return [classes - 2, classes - 1]


def C(fn, seed, classes=10, size=SIZE, crop=CROP, variant='default', tumor_case=True, pad=None, probs=None):
    return dict(fn=fn, seed=seed, classes=classes, size=size, crop=crop, variant=variant, tumor_case=tumor_case, pad=pad, probs=probs)


LARGE = (CROP[0] + 20, CROP[1] + 40, CROP[2] + 40)
CASES = (
    # seeds 0 .. 39 of random_crop_on_tumor reach all three branches: organ at 4 and 24, background at 37, tumour otherwise
    [C('random_crop_on_tumor', s) for s in (0, 1, 2, 3, 4, 24, 37)]
    + [C('random_crop_on_tumor', s, tumor_case=False) for s in (0, 1, 5)]                            # probabilities 0 / 0.9 / 0.1
    + [C('random_crop_on_tumor', 2, probs=(0.3, 0.3, 0.4)), C('random_crop_on_tumor', 6, probs=(0.3, 0.3, 0.4))]
    + [C(fn, s) for fn in ('tumor_crop', 'organ_crop', 'negative_crop') for s in (0, 1)]
    + [C('tumor_crop', 3, variant='no_lesion'), C('organ_crop', 3, variant='no_foreground'), C('negative_crop', 3, variant='no_background'),
       C('random_crop_on_tumor', 0, variant='no_lesion'), C('random_crop_on_tumor', 37, variant='no_background')]
    + [C(fn, 7, classes=c) for c in (5, 8, 26, 42) for fn in ('tumor_crop', 'organ_crop', 'negative_crop')]
    + [C(fn, 8, size=SMALL_ONE, crop=LARGE, pad=LARGE) for fn in ('tumor_crop', 'organ_crop', 'negative_crop', 'random_crop_on_tumor')]
    + [C(fn, 9, size=SMALL_ALL, crop=LARGE, pad=LARGE) for fn in ('tumor_crop', 'organ_crop', 'negative_crop', 'random_crop_on_tumor')]
    + [C(fn, 10, size=SMALL_ALL, crop=CROP, pad=LARGE) for fn in ('negative_crop', 'tumor_crop', 'organ_crop')]
    + [C('tumor_crop', 10, size=SIZE, crop=CROP, pad=(44, 93, 107))]
)
WRAP_SEED, WRAP_LEN, WRAP_CROP, WRAP_ARGS = 11, 10, (16, 12, 16), dict(scale=0.3, rotate=45, translate=0.1)
WRAP_TUMOR_NAMES = ['pancreatic_lesion', 'kidney_lesion', 'liver']
WRAP_CLASSES = ['pancreas', 'kidney_right', 'kidney_left', 'liver', 'spleen', 'aorta', 'stomach', 'gall_bladder', 'pancreatic_lesion', 'kidney_lesion']


def case_inputs(seed, classes, size, variant='default'):
    """Image (1, 1, D, H, W) f32: 1 + the voxel's linear index.  Label (1, classes, D, H, W) u8 0/1: two ellipsoids per class, small ones for the two
    lesion classes (the last two), class 3 left empty.  variant: 'no_lesion' / 'no_foreground' clear those classes, 'no_background' fills class 4."""
    rs = np.random.RandomState(2000 + seed)
    D, H, W = size
    img = (1 + np.arange(D * H * W, dtype=np.float32)).reshape(1, 1, D, H, W)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')

    def ellipsoid(rmin, rmax):
        c = rs.uniform(0.15, 0.85, 3) * np.array(size)
        r = rs.uniform(rmin, rmax, 3) * np.array(size)
        return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < 1.0

    lab = np.zeros((1, classes, D, H, W), np.uint8)
    lesion = lesion_of(classes)
    for c in range(classes):
        lab[0, c] = ellipsoid(0.04, 0.1) | ellipsoid(0.03, 0.08) if c in lesion else ellipsoid(0.08, 0.3) | ellipsoid(0.05, 0.2)
    lab[0, 3] = 0
    if variant == 'no_lesion':
        lab[0, lesion] = 0
    elif variant == 'no_foreground':
        lab[0, FOREGROUND] = 0
    elif variant == 'no_background':
        lab[0, 4] = 1
    else:
        assert variant == 'default'
    return torch.from_numpy(img), torch.from_numpy(lab)


def corner_of(crop, padded, size):
    """The corner (padded coordinates) of a crop of the padded index image: from its first non-zero voxel."""
    a = np.asarray(crop).reshape(crop.shape[-3:])
    i = np.flatnonzero(a)[0]
    pos = np.unravel_index(i, a.shape)
    src = np.unravel_index(int(a.reshape(-1)[i]) - 1, size)
    lo = [(p - s) // 2 for p, s in zip(padded, size)]
    return [int(s + l - p) for s, l, p in zip(src, lo, pos)]


def import_reference():
    ref = os.environ.get('RSUPER_REFERENCE')
    if not ref or not os.path.isdir(ref):
        raise SystemExit('set RSUPER_REFERENCE to the reference checkout\'s rsuper_train directory')
    for name in ('SimpleITK', 'nibabel', 'torchvision', 'torchvision.transforms'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.path.insert(0, ref)
    return importlib.import_module('training.augmentation')


class Spy:
    """While active: records which reference functions are entered, the coordinate crop_around_coordinate_3d receives and every torch.randint /
    np.random.randint with its result.  Everything passes through unchanged."""
    NAMES = ('tumor_crop', 'negative_crop', 'organ_crop', 'crop_3d', 'crop_around_coordinate_3d')

    def __init__(self, aug):
        self.aug = aug

    def __enter__(self):
        self.calls, self.center, self.tdraws, self.ndraws = [], None, [], []
        self._orig = {n: getattr(self.aug, n) for n in self.NAMES}
        self._trand, self._nrand = torch.randint, np.random.randint
        for n in self.NAMES:
            setattr(self.aug, n, self._wrap(n))

        def trand(low, high, size, **kw):
            r = self._trand(low, high, size, **kw)
            self.tdraws.append((int(high), int(r)))
            return r

        def nrand(low, high=None, *a, **kw):
            r = self._nrand(low, high, *a, **kw)
            self.ndraws.append((int(low), int(high), int(r)))
            return r
        torch.randint, np.random.randint = trand, nrand
        return self

    def _wrap(self, name):
        def f(*a, **kw):
            if name == 'crop_around_coordinate_3d':
                self.center = [int(v) for v in kw['coordinate']]
            else:
                self.calls.append(name)
            return self._orig[name](*a, **kw)
        return f

    def __exit__(self, *exc):
        for n, f in self._orig.items():
            setattr(self.aug, n, f)
        torch.randint, np.random.randint = self._trand, self._nrand


def run_reference(aug, case):
    """One case through the unmodified reference -> the record dict (without the case's index)."""
    img, lab = case_inputs(case['seed'], case['classes'], case['size'], case['variant'])
    lesion = lesion_of(case['classes'])
    d, h, w = case['crop']
    if case['pad'] is not None:
        pimg, plab = aug.pad_volume_pair(img, lab, *case['pad'])
    else:
        pimg, plab = img, lab
    padded = tuple(pimg.shape[2:])
    np.random.seed(case['seed'])
    torch.manual_seed(case['seed'])
    organ = -2
    with Spy(aug) as spy, contextlib.redirect_stdout(io.StringIO()):
        if case['fn'] == 'random_crop_on_tumor':
            tp, fp, bp = case['probs'] if case['probs'] else (None, None, None)
            ci, cl, co = aug.random_crop_on_tumor(pimg, plab, lesion, d, h, w, case['tumor_case'], tumor_prob=tp, foreground_prob=fp,
                                                  background_prob=bp, return_crop_organ=True, class_names=list(range(case['classes'])),
                                                  foreground_classes=FOREGROUND)
            organ = -1 if co == 'random' else int(co)
        elif case['fn'] == 'tumor_crop':
            ci, cl, co = aug.tumor_crop(pimg, plab, lesion, d, h, w, return_crop_organ=True)
            organ = -1 if co == 'random' else int(co)
        elif case['fn'] == 'organ_crop':
            ci, cl, co = aug.organ_crop(pimg, plab, lesion, d, h, w, return_crop_organ=True, foreground_classes=FOREGROUND)
            organ = -1 if co == 'random' else int(co)
        else:
            ci, cl = aug.negative_crop(pimg, plab, lesion, d, h, w)
    nxt_np, nxt_t = np.random.random(), float(torch.rand(1))
    org = corner_of(ci.numpy(), padded, case['size'])
    z, y, x = org
    assert tuple(ci.shape[2:]) == (d, h, w)
    assert torch.equal(ci, pimg[:, :, z:z + d, y:y + h, x:x + w]) and torch.equal(cl, plab[:, :, z:z + d, y:y + h, x:x + w])
    rank = count = -1
    if spy.center is not None:
        if spy.calls[-1] == 'negative_crop':
            mask = plab[0].sum(0) == 0
        else:
            mask = plab[0, organ] != 0
        vox = torch.nonzero(mask)
        count = len(vox)
        rank = int(torch.nonzero((vox == torch.tensor(spy.center)).all(1))[0])
        assert spy.tdraws[-1] == (count, rank)
    return {'calls': np.array('>'.join(spy.calls)), 'organ': np.array(organ), 'center': np.array(spy.center if spy.center else [-1, -1, -1]),
            'rank': np.array(rank), 'count': np.array(count), 'tdraws': np.array(spy.tdraws, np.int64).reshape(-1, 2),
            'ndraws': np.array(spy.ndraws, np.int64).reshape(-1, 3), 'origin': np.array(org), 'padded': np.array(padded),
            'next_np': np.array(nxt_np), 'next_torch': np.array(nxt_t, np.float32)}


def run_wrapper(aug):
    """dataset_abdomenatlas_UFO.py:580-631 restated with the reference functions, WRAP_LEN samples under one seed."""
    import torch.nn.functional as F
    img, lab = case_inputs(WRAP_SEED, len(WRAP_CLASSES), SIZE)
    lesion = lesion_of(len(WRAP_CLASSES))
    forg = []
    for c in WRAP_TUMOR_NAMES:
        if 'pancrea' in c:
            forg.append('pancreas')
        elif 'kidney' in c:
            forg.append('kidney_right')
            forg.append('kidney_left')
        elif 'gall' in c:
            forg.append('gall_bladder')
        else:
            forg.append(c)
    forg = [WRAP_CLASSES.index(c) for c in list(set(forg))]
    d, h, w = WRAP_CROP
    np.random.seed(WRAP_SEED)
    torch.manual_seed(WRAP_SEED)
    large, origins, thetas = [], [], []
    orig_grid = F.affine_grid
    for _ in range(WRAP_LEN):
        tumor_case = lab[:, lesion].sum() > 0
        with contextlib.redirect_stdout(io.StringIO()):
            if np.random.random() < 0.4:
                ci, cl = aug.random_crop_on_tumor(img, lab, lesion, d + 20, h + 40, w + 40, tumor_case, foreground_classes=forg)
                seen = []
                F.affine_grid = lambda theta, size, align_corners=None: (seen.append(theta.detach().clone()), orig_grid(theta, size, align_corners=align_corners))[1]
                try:
                    aug.random_scale_rotate_translate_3d(ci, cl.long(), WRAP_ARGS['scale'], WRAP_ARGS['rotate'], WRAP_ARGS['translate'])
                finally:
                    F.affine_grid = orig_grid
                large.append(1)
                thetas.append(seen[0][0].numpy())
            else:
                ci, cl = aug.random_crop_on_tumor(img, lab, lesion, d, h, w, tumor_case, foreground_classes=forg)
                large.append(0)
                thetas.append(np.eye(4, dtype=np.float32)[:3])
        origins.append(corner_of(ci.numpy(), SIZE, SIZE))
    assert 0 < sum(large) < WRAP_LEN
    return {'wrap_forg': np.array(sorted(forg)), 'wrap_large': np.array(large), 'wrap_origins': np.array(origins), 'wrap_thetas': np.stack(thetas),
            'wrap_next_np': np.array(np.random.random()), 'wrap_next_torch': np.array(float(torch.rand(1)), np.float32)}


def main():
    aug = import_reference()
    out = {'n_cases': np.array(len(CASES))}
    seen = set()
    for k, case in enumerate(CASES):
        rec = run_reference(aug, case)
        rec['seed'], rec['args'] = np.array(case['seed']), np.array(json.dumps(case, sort_keys=True))
        for name, v in rec.items():
            out['%s_%d' % (name, k)] = v
        seen.add(str(rec['calls']))
        print('case %2d %-22s seed %2d C %2d %-14s -> %-22s organ %2d origin %s' % (k, case['fn'], case['seed'], case['classes'], case['variant'],
                                                                                    rec['calls'], rec['organ'], rec['origin'].tolist()))
    need = {'tumor_crop', 'organ_crop', 'negative_crop', 'tumor_crop>crop_3d', 'organ_crop>crop_3d', 'negative_crop>crop_3d'}
    assert need <= seen, need - seen
    out.update(run_wrapper(aug))
    path = os.path.join(HERE, 'crop.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'kB')


if __name__ == '__main__':
    main()
