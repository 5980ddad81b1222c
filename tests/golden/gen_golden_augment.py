#!/usr/bin/env python3
"""Golden vectors for the spatial augmentation, produced by the UNMODIFIED reference `training/augmentation.py`
(random_scale_rotate_translate_3d :228-319, crop_3d :446-469) under seeded numpy generators.  Run in the authoring container only:

    RSUPER_REFERENCE=<checkout of the reference>/rsuper_train python tests/golden/gen_golden_augment.py

Import shims as in gen_golden_loader.py: `SimpleITK`, `nibabel`, `torchvision` are only touched by code outside this path, so empty
modules are registered for them.  theta is captured by wrapping F.affine_grid for the duration of a call.

Writes tests/golden/augment.npz.  Inputs are NOT stored: `case_inputs` below regenerates them from the case's seed (the tests import it).
Per case k:  theta_k (3, 4) f32, next_k (the next np.random.random() after the reference call: pins the draws consumed),
  img_k (1, 1, d, h, w) f32 and lab_k (1, P, d, h, w) packed u8 [, fg_k (1, 1, d, h, w) u8]: the reference's transform + centre crop,
  tie_k: np.packbits of the (d, h, w) mask of voxels whose float64 source coordinate lies within TIE_BAND of a half-integer on any axis
  (there the reference's f32 coordinate may round to either neighbour), e_ref_k: the reference image's maximum distance from the float64
  trilinear value on the crop.
crop_seed_s: the (z, y, x) corner crop_3d(mode='random') cuts under seed s; branch_*: `random_crop`'s branch (dataset_abdomenatlas_UFO.py:573-577)
restated with the reference functions for SEQ_LEN consecutive samples under one seed.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))

SIZE, CROP = (40, 48, 44), (24, 28, 24)
TIE_BAND = 2e-4
TIE_MAX_FRACTION = 0.005
# seed, classes, keyword arguments of random_scale_rotate_translate_3d, with a foreground mask
CASES = [
    (0, 26, dict(scale=0.3, rotate=45, translate=0.1), False),                       # the function's defaults
    (1, 26, dict(scale=0.3, rotate=45, translate=0.1), False),
    (2, 26, dict(scale=0, rotate=30, translate=0), False),                           # the shipped MedFormer YAML
    (3, 26, dict(scale=[0.1, 0.2, 0.3], rotate=[10, 20, 30], translate=[0.05, 0.1, 0.0], shear=[0.02, 0.05, 0.0]), False),
    (4, 26, dict(scale=0.3, rotate=45, translate=0.1), True),
    (5, 3, dict(scale=0.3, rotate=45, translate=0.1), False),
]
CROP_SEEDS = (0, 1, 2, 3)
SEQ_SEED, SEQ_LEN, SEQ_ARGS = 7, 12, dict(scale=0.3, rotate=45, translate=0.1)


def case_inputs(seed, classes, size=SIZE):
    """Image: unit-variance white noise (1, 1, D, H, W) f32.  Label: (1, classes, D, H, W) u8 0/1, two random ellipsoids per class.
    Foreground: (D, H, W) bool, one large ellipsoid."""
    rs = np.random.RandomState(1000 + seed)
    D, H, W = size
    img = rs.standard_normal((1, 1, D, H, W)).astype(np.float32)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')

    def ellipsoid(rmin, rmax):
        c = rs.uniform(0.15, 0.85, 3) * np.array(size)
        r = rs.uniform(rmin, rmax, 3) * np.array(size)
        return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < 1.0

    lab = np.zeros((1, classes, D, H, W), np.uint8)
    for c in range(classes):
        lab[0, c] = ellipsoid(0.08, 0.3) | ellipsoid(0.05, 0.2)
    fg = ellipsoid(0.3, 0.45)
    return torch.from_numpy(img), torch.from_numpy(lab), torch.from_numpy(fg)


def source_coords(theta, size):
    """float64 source coordinates (3, D, H, W) in x, y, z order of the full grid: affine_grid(align_corners=True) + grid_sample's un-normalisation."""
    D, H, W = size
    t = np.asarray(theta, np.float64).reshape(3, 4)
    z, y, x = np.meshgrid(-1 + 2 * np.arange(D) / (D - 1), -1 + 2 * np.arange(H) / (H - 1), -1 + 2 * np.arange(W) / (W - 1), indexing='ij')
    n = (W, H, D)
    return np.stack([((t[r, 0] * x + t[r, 1] * y + t[r, 2] * z + t[r, 3]) + 1) / 2 * (n[r] - 1) for r in range(3)])


def tie_mask(coords):
    """Voxels whose coordinate lies within TIE_BAND of a half-integer on any axis."""
    return (np.abs(coords - np.floor(coords) - 0.5) < TIE_BAND).any(0)


def center(a, crop=CROP):
    off = [(s - c) // 2 for s, c in zip(a.shape[-3:], crop)]
    return a[..., off[0]:off[0] + crop[0], off[1]:off[1] + crop[1], off[2]:off[2] + crop[2]]


def trilinear_f64(img, theta):
    """The float64 trilinear value on the full grid, by torch's own CPU operators in double."""
    t = torch.as_tensor(np.asarray(theta), dtype=torch.float64).reshape(-1, 3, 4)
    grid = F.affine_grid(t, list(img.shape), align_corners=True)
    return F.grid_sample(img.double(), grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def import_reference():
    ref = os.environ.get('RSUPER_REFERENCE')
    if not ref or not os.path.isdir(ref):
        raise SystemExit('set RSUPER_REFERENCE to the reference checkout\'s rsuper_train directory')
    for name in ('SimpleITK', 'nibabel', 'torchvision', 'torchvision.transforms'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.path.insert(0, ref)
    return importlib.import_module('training.augmentation')


class CaptureTheta:
    """Wraps F.affine_grid while active and keeps the theta of every call."""

    def __enter__(self):
        self.thetas, self._orig = [], F.affine_grid

        def wrapped(theta, size, align_corners=None):
            self.thetas.append(theta.detach().clone())
            return self._orig(theta, size, align_corners=align_corners)
        F.affine_grid = wrapped
        return self

    def __exit__(self, *exc):
        F.affine_grid = self._orig


def main():
    aug = import_reference()
    out = {'size': np.array(SIZE), 'crop': np.array(CROP), 'n_cases': np.array(len(CASES))}
    for k, (seed, classes, kw, with_fg) in enumerate(CASES):
        img, lab, fg = case_inputs(seed, classes)
        np.random.seed(seed)
        with CaptureTheta() as cap:
            r = aug.random_scale_rotate_translate_3d(img, lab.long(), foreground=fg if with_fg else None, **kw)
        out['next_%d' % k] = np.array(np.random.random())
        assert len(cap.thetas) == 1 and cap.thetas[0].dtype == torch.float32
        theta = cap.thetas[0][0].numpy()
        assert r[1].dtype == torch.int64 and r[0].shape == img.shape and r[1].shape == lab.shape
        ci, cl = aug.crop_3d(r[0], r[1], list(CROP), mode='center')
        out['theta_%d' % k] = theta
        out['img_%d' % k] = ci.numpy()
        out['lab_%d' % k] = np.packbits(cl.numpy().astype(np.bool_), axis=1)
        if with_fg:
            assert r[2].dtype == torch.bool and r[2].shape == fg.shape
            out['fg_%d' % k] = center(r[2].numpy()).astype(np.uint8)[None, None]
        tie = center(tie_mask(source_coords(theta, SIZE)))
        frac = tie.mean()
        assert frac <= TIE_MAX_FRACTION, 'case %d: %.3f %% of the voxels lie in the tie band' % (k, 100 * frac)
        out['tie_%d' % k] = np.packbits(tie)
        e_ref = np.abs(ci.numpy().astype(np.float64) - center(trilinear_f64(img, theta).numpy())).max()
        out['e_ref_%d' % k] = np.array(e_ref)
        print('case %d seed %d classes %d: tie band %.3f %%, e_ref %.3g' % (k, seed, classes, 100 * frac, e_ref))

    # crop_3d 'random': the corner is read back from an image that holds its own linear index
    idx = torch.arange(SIZE[0] * SIZE[1] * SIZE[2], dtype=torch.float32).reshape((1, 1) + SIZE)
    for s in CROP_SEEDS:
        np.random.seed(s)
        c, _ = aug.crop_3d(idx, idx, list(CROP), mode='random')
        first = int(c[0, 0, 0, 0, 0])
        out['crop_seed_%d' % s] = np.array([first // (SIZE[1] * SIZE[2]), first // SIZE[2] % SIZE[1], first % SIZE[2]])
    c, _ = aug.crop_3d(idx, idx, list(CROP), mode='center')
    first = int(c[0, 0, 0, 0, 0])
    out['crop_center'] = np.array([first // (SIZE[1] * SIZE[2]), first // SIZE[2] % SIZE[1], first % SIZE[2]])

    # the branch of random_crop for consecutive samples under one seed
    np.random.seed(SEQ_SEED)
    branch, offs, thetas = [], [], []
    for _ in range(SEQ_LEN):
        if np.random.random() < 0.4:
            with CaptureTheta() as cap:
                a, b = aug.random_scale_rotate_translate_3d(idx, idx.long(), SEQ_ARGS['scale'], SEQ_ARGS['rotate'], SEQ_ARGS['translate'])
            c, _ = aug.crop_3d(idx, idx, list(CROP), mode='center')
            branch.append(1)
            thetas.append(cap.thetas[0][0].numpy())
        else:
            c, _ = aug.crop_3d(idx, idx, list(CROP), mode='random')
            branch.append(0)
            thetas.append(np.eye(4, dtype=np.float32)[:3])
        first = int(c[0, 0, 0, 0, 0])
        offs.append([first // (SIZE[1] * SIZE[2]), first // SIZE[2] % SIZE[1], first % SIZE[2]])
    out['branch_taken'], out['branch_offsets'], out['branch_thetas'] = np.array(branch), np.array(offs), np.stack(thetas)
    out['branch_next'] = np.array(np.random.random())
    assert 0 < sum(branch) < SEQ_LEN

    path = os.path.join(HERE, 'augment.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'kB')


if __name__ == '__main__':
    main()
