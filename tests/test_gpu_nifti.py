"""MI355X tests of the NIfTI front and back end (csrc/nifti.hip, inference/nifti_device.py) against tests/nifti_ref.py: reorientation bit for
bit against numpy, prefilter + resample within 0.02 HU of scipy's float64 cubic spline (outside voxels exactly), load_nifti_device and
save_nifti_masks on files the test writes, and predict_abdomenatlas --nifti end to end on a tiny seeded UNet.

The 0.02 HU bound: the same recursion in float32 numpy stays within 8e-4 HU of scipy's float64 on the coefficients and 2e-4 on the samples of
such data; 0.02 leaves about 25x for fused multiply-add and ordering and is 50x below the 1 HU quantum, so a wrong tap, mirror or boundary
(several HU) fails by hundreds of times the bound."""
import gzip
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import nifti_ref as R  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BOUND_HU = 0.02
NP_OF = {2: np.uint8, 256: np.int8, 4: np.int16, 512: np.uint16, 8: np.int32, 16: np.float32, 64: np.float64}
CLASSES = ['kidney_left', 'kidney_lesion', 'kidney_right', 'liver', 'liver_lesion', 'pancreas', 'pancreatic_lesion']
LAS = ((0, 1, 2), (False, True, False))
LAS_PIX = (0.8, 0.8, 2.5)
LAS_SHAPE = (40, 36, 14)


def volume_of(arr_ijk, datatype, pixdim, perm, flip, slope=0.0, inter=0.0):
    """The NiftiVolume read_nifti would return for arr_ijk stored with this orientation (built in memory: the file reader has its own CPU tests)."""
    from rsuper_amd.inference.nifti import NiftiVolume
    A = R.affine_for(perm, flip, pixdim)
    data = R.file_order(arr_ijk).astype(np.float32 if datatype == 64 else NP_OF[datatype])
    return NiftiVolume(path='<memory>', data=data, shape=tuple(arr_ijk.shape), pixdim=tuple(float(np.float32(v)) for v in pixdim), qfac=1.0,
                       datatype=datatype, vox_offset=352, scl_slope=slope, scl_inter=inter, qform_code=0, sform_code=1, quatern=(0.0, 0.0, 0.0),
                       qoffset=(0.0, 0.0, 0.0), srow=A[:3].copy())


def test_reorientation_all_48_orientations_int16_bit_exact():
    """5 x 7 x 9 canonical ramp of int16 stored in each of the 48 orientations at the target spacing: one load launch each, no prefilter, no resample."""
    from rsuper_amd.inference import load_nifti_device
    from rsuper_amd.inference.nifti_device import nifti_launches
    rng = np.random.default_rng(3)
    canon = rng.integers(-1024, 3072, size=(9, 7, 5)).astype(np.int16)
    before = nifti_launches()
    for perm, flip in R.ORIENTATIONS:
        arr = R.inverse_reorient(canon, perm, flip)
        hu, geom = load_nifti_device(volume_of(arr, 4, (1.0, 1.0, 1.0), perm, flip))
        assert (geom.perm, geom.flip) == (perm, flip) and geom.size == (5, 7, 9) and geom.shape_ijk == arr.shape
        assert hu.is_cuda and hu.dtype == torch.float32 and tuple(hu.shape) == (9, 7, 5)
        assert np.array_equal(hu.cpu().numpy(), canon.astype(np.float32)), (perm, flip)
    after = nifti_launches()
    assert after['load'] - before['load'] == 48 and after['prefilter'] == before['prefilter'] and after['resample'] == before['resample']


@pytest.mark.parametrize('datatype,orient', [(2, 5), (256, 13), (512, 22), (8, 31), (16, 40), (64, 47)])
def test_reorientation_other_dtypes_with_slope_and_intercept_bit_exact(datatype, orient):
    from rsuper_amd.inference import load_nifti_device
    perm, flip = R.ORIENTATIONS[orient]
    rng = np.random.default_rng(datatype)
    lo, hi = {2: (0, 256), 256: (-128, 128), 512: (0, 65536), 8: (-2 ** 31, 2 ** 31), 16: (-3000, 3000), 64: (-3000, 3000)}[datatype]
    canon = rng.integers(lo, hi, size=(9, 7, 5)).astype(NP_OF[datatype])
    if datatype in (16, 64):
        canon = canon + rng.random(canon.shape).astype(canon.dtype)
    arr = R.inverse_reorient(canon, perm, flip)
    hu, _ = load_nifti_device(volume_of(arr, datatype, (1.0, 1.0, 1.0), perm, flip, slope=2.5, inter=-1024.0))
    want = canon.astype(np.float32) * np.float32(2.5) + np.float32(-1024.0)
    assert np.array_equal(hu.cpu().numpy(), want)
    hu, _ = load_nifti_device(volume_of(arr, datatype, (1.0, 1.0, 1.0), perm, flip))           # slope 0: no scaling
    assert np.array_equal(hu.cpu().numpy(), canon.astype(np.float32))


SHAPES = [(5, 37, 29), (3, 1, 200), (2, 200, 3), (4, 130, 67), (1, 2, 2)]                     # (Z, Y, X)
INPLANE = [(0.8203, 0.8203), (1.5, 1.5), (1.0, 0.8203)]                                      # (x, y) spacing: down, up, one axis 1 -> 1
ZSPACING = [2.5, 0.625]
_PHANTOMS = {}


def _phantom(shape):
    if shape not in _PHANTOMS:
        _PHANTOMS[shape] = R.phantom(shape, 100 + len(_PHANTOMS))
        _PHANTOMS[shape].setflags(write=False)
    return _PHANTOMS[shape]


@pytest.mark.parametrize('zsp', ZSPACING)
@pytest.mark.parametrize('inplane', INPLANE, ids=['down', 'up', 'x_same'])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_prefilter_and_resample_against_scipy(shape, inplane, zsp):
    from rsuper_amd.inference import nifti as N
    vol = _phantom(shape)
    assert vol.min() >= -1024 and vol.max() <= 3071
    spacing = (inplane[0], inplane[1], zsp)
    ref, inside = R.resample(vol, spacing, (1.0, 1.0, 1.0))
    Z, Y, X = shape
    raw = torch.from_numpy(vol.copy().reshape(-1).view(np.uint8)).to(DEV)          # the shared phantom stays read-only
    coef = torch.ops.rsuper.nifti_load_prefilter(raw, 2, [Z, Y, X], [Y * X, X, 1], 0, 1.0, 0.0, True)
    ix, wx = N.resample_axis_table(X, spacing[0], 1.0, 'bspline')
    iy, wy = N.resample_axis_table(Y, spacing[1], 1.0, 'bspline')
    iz = N.resample_axis_table(Z, spacing[2], 1.0, 'nearest')
    got = torch.ops.rsuper.bspline_resample(coef, *[torch.from_numpy(t).to(DEV) for t in (ix, wx, iy, wy, iz)], 0.0).cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    # the coefficients themselves against scipy's prefilter, slice by slice
    from scipy import ndimage
    cref = np.stack([ndimage.spline_filter(vol[z].astype(np.float64), order=3, mode='mirror') for z in range(Z)])
    cerr = float(np.abs(coef.cpu().numpy() - cref).max())
    err = float(np.abs(got[inside] - ref[inside]).max()) if inside.any() else 0.0
    print(f'{shape} spacing {spacing}: out {got.shape}, coefficient error {cerr:.2e} HU, sample error {err:.2e} HU, outside voxels {int((~inside).sum())}')
    assert cerr <= BOUND_HU and err <= BOUND_HU
    assert np.array_equal(got[~inside], ref[~inside]) and (got[~inside] == 0.0).all()            # outside voxels exactly


def test_outside_value_and_flipped_source_through_the_prefilter():
    """The prefilter reads through negative strides too (a flipped, permuted file) and outside voxels take the caller's value."""
    from rsuper_amd.inference import load_nifti_device
    vol = _phantom((5, 37, 29))
    perm, flip = (2, 0, 1), (True, False, True)
    arr = R.inverse_reorient(vol, perm, flip)
    pix_xyz = (1.5, 0.8203, 2.5)
    pix = tuple(pix_xyz[perm[a]] for a in range(3))
    hu, geom = load_nifti_device(volume_of(arr, 4, pix, perm, flip), outside_value=-1024.0)
    sp = tuple(float(np.float32(v)) for v in pix_xyz)
    assert geom.spacing == sp and geom.size == (29, 37, 5)
    ref, inside = R.resample(vol, sp, (1.0, 1.0, 1.0), outside_value=-1024.0)
    got = hu.cpu().numpy()
    assert got.shape == ref.shape and (~inside).any()
    assert np.abs(got[inside] - ref[inside]).max() <= BOUND_HU and (got[~inside] == -1024.0).all()


@pytest.fixture(scope='module')
def las_file(tmp_path_factory):
    """The LAS scan of the issue: 40 x 36 x 14 voxels at 0.8 x 0.8 x 2.5 mm, int16, qform and sform, gzip, written by the tests' own writer."""
    d = tmp_path_factory.mktemp('nifti')
    canon = R.phantom((14, 36, 40), 9)
    canon = np.clip(canon, -1000, 600).astype(np.int16)
    arr = R.inverse_reorient(canon, *LAS)
    A = R.affine_for(*LAS, LAS_PIX, origin=(100.0, -80.0, -300.0))
    b, c, dd, qfac, _ = R.qform_of(A)
    os.makedirs(d / 'img')
    path = d / 'img' / 'BDMAP_00000009.nii.gz'
    R.write_nifti(path, arr, 4, LAS_PIX, sform=A, qform=(b, c, dd, qfac), qoffset=(100.0, -80.0, -300.0))
    return {'dir': str(d), 'path': str(path), 'canon': canon, 'arr': arr, 'affine': A}


def test_load_nifti_device_end_to_end(las_file):
    from rsuper_amd.inference import load_nifti_device, read_nifti
    from rsuper_amd.inference import nifti as N
    from rsuper_amd.inference.nifti_device import nifti_launches
    hu, geom = load_nifti_device(las_file['path'])
    assert (geom.perm, geom.flip) == LAS and geom.shape_ijk == LAS_SHAPE and geom.size == LAS_SHAPE
    sp = tuple(float(np.float32(v)) for v in LAS_PIX)
    assert geom.spacing == sp and geom.pixdim == sp and np.allclose(geom.affine, las_file['affine'], atol=1e-5)
    # the kernel-level result on the canonical array
    canon = las_file['canon']
    Z, Y, X = canon.shape
    raw = torch.from_numpy(canon.reshape(-1).view(np.uint8)).to(DEV)
    coef = torch.ops.rsuper.nifti_load_prefilter(raw, 2, [Z, Y, X], [Y * X, X, 1], 0, 1.0, 0.0, True)
    tabs = [N.resample_axis_table(X, sp[0], 1.0, 'bspline'), N.resample_axis_table(Y, sp[1], 1.0, 'bspline')]
    iz = N.resample_axis_table(Z, sp[2], 1.0, 'nearest')
    want = torch.ops.rsuper.bspline_resample(coef, *[torch.from_numpy(t).to(DEV) for t in (*tabs[0], *tabs[1], iz)], 0.0)
    assert tuple(hu.shape) == (35, 29, 32) == tuple(want.shape) and torch.equal(hu, want)
    ref, inside = R.resample(canon, sp, (1.0, 1.0, 1.0))
    assert np.abs(hu.cpu().numpy()[inside] - ref[inside]).max() <= BOUND_HU and (hu.cpu().numpy()[~inside] == 0).all() and (~inside).any()
    # the same spacing as the target: the reoriented samples, zero prefilter and zero resample launches
    before = nifti_launches()
    hu1, _ = load_nifti_device(read_nifti(las_file['path']), target_spacing=LAS_PIX)
    after = nifti_launches()
    assert after['resample'] == before['resample'] and after['prefilter'] == before['prefilter'] and after['load'] == before['load'] + 1
    assert np.array_equal(hu1.cpu().numpy(), canon.astype(np.float32))
    with pytest.raises(Exception):
        torch.ops.rsuper.bspline_resample(coef.cpu(), *[torch.from_numpy(t) for t in (*tabs[0], *tabs[1], iz)], 0.0)


@pytest.mark.parametrize('orient', [0, 9, 18, 27, 36, 47])
def test_save_nifti_masks_round_trip(tmp_path, orient):
    """3 random uint8 class planes on a 9 x 7 x 5 canonical grid -> .nii.gz in the input's voxel order, read back with gzip and the tests' parser."""
    from rsuper_amd.inference import save_nifti_masks
    from rsuper_amd.inference.nifti_device import geometry_of
    perm, flip = R.ORIENTATIONS[orient]
    rng = np.random.default_rng(orient)
    stack = rng.integers(0, 256, size=(3, 9, 7, 5)).astype(np.uint8)
    pix_xyz = (0.7, 0.8, 2.5)
    pix = tuple(pix_xyz[perm[a]] for a in range(3))
    shape_ijk = tuple((5, 7, 9)[perm[a]] for a in range(3))
    geom = geometry_of(volume_of(np.zeros(shape_ijk, np.int16), 4, pix, perm, flip))
    names = ['liver', 'liver_lesion', 'pancreas']
    save_nifti_masks(str(tmp_path), {n: torch.from_numpy(stack[k]).to(DEV) for k, n in enumerate(names)}, names, geom)
    assert sorted(os.listdir(tmp_path / 'predictions')) == sorted(n + '.nii.gz' for n in names)
    for k, n in enumerate(names):
        h, arr = R.read_nifti_gz(tmp_path / 'predictions' / (n + '.nii.gz'))
        assert h['datatype'] == 2 and h['bitpix'] == 8 and h['dim'][:4] == (3,) + shape_ijk and h['vox_offset'] == 352.0
        assert h['pixdim'][1:4] == tuple(float(np.float32(v)) for v in pix)
        assert np.array_equal(h['srow'], geom.affine[:3].astype(np.float32).astype(np.float64))
        # the qform says the same as far as float32 b, c, d can: near a half turn a = sqrt(1 - b^2 - c^2 - d^2) is known to sqrt(2^-23) = 3.5e-4 only,
        # a rotation error of 7e-4 times the largest spacing (2.5 mm)
        assert np.allclose(R.quaternion_affine(h), geom.affine, atol=2.5 * 7e-4 + 1e-5)
        assert arr.dtype == np.uint8 and np.array_equal(arr, R.inverse_reorient(stack[k], perm, flip))


def test_save_nifti_masks_vector_path_and_wrong_grid(tmp_path):
    """ni a multiple of four takes the 4-byte store path; masks that are not on the scan's canonical grid are refused."""
    from rsuper_amd.inference import save_nifti_masks
    from rsuper_amd.inference.nifti_device import geometry_of
    perm, flip = (1, 0, 2), (True, False, True)
    rng = np.random.default_rng(1)
    stack = (rng.random((2, 6, 8, 10)) < 0.3).astype(np.uint8)                  # canonical (Z, Y, X) = (6, 8, 10); ni = Y = 8
    geom = geometry_of(volume_of(np.zeros((8, 10, 6), np.int16), 4, (1.0, 1.0, 1.0), perm, flip))
    names = ['a', 'b']
    save_nifti_masks(str(tmp_path), {n: torch.from_numpy(stack[k]).to(DEV) for k, n in enumerate(names)}, names, geom)
    for k, n in enumerate(names):
        with gzip.open(tmp_path / 'predictions' / (n + '.nii.gz')) as f:
            assert len(f.read()) == 352 + 480
        assert np.array_equal(R.read_nifti_gz(tmp_path / 'predictions' / (n + '.nii.gz'))[1], R.inverse_reorient(stack[k], perm, flip))
    with pytest.raises(ValueError, match='canonical grid'):
        save_nifti_masks(str(tmp_path), {'a': torch.zeros((6, 8, 9), dtype=torch.uint8, device=DEV)}, ['a'], geom)


def test_predict_abdomenatlas_nifti_end_to_end(las_file):
    """main([... '--nifti']) on the LAS file with a tiny seeded UNet: every written mask is predict_case fed with load_nifti_device's own output,
    put back into the file's voxel order by numpy, bit for bit; the same directory without --nifti still raises the section 3b error."""
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd.inference import load_nifti_device, predict_case
    from rsuper_amd.model.dim3.unet import UNet
    d = las_file['dir']
    os.makedirs(os.path.join(d, 'run3'), exist_ok=True)
    with open(os.path.join(d, 'classes.yaml'), 'w') as f:
        f.write('[' + ', '.join(reversed(CLASSES)) + ']\n')
    with open(os.path.join(d, 'unet8.yaml'), 'w') as f:
        f.write('in_chan: 1\nbase_chan: 8\ndown_scale: [[2,2,2], [2,2,2], [2,2,2], [2,2,2]]\nkernel_size: [[3,3,3], [3,3,3], [3,3,3], [3,3,3], [3,3,3]]\n'
                'block: BasicBlock\nnorm: in\ncompute_dtype: f32\ntraining_size: [32, 32, 32]\n')
    net = UNet(1, 8, num_classes=len(CLASSES), block='BasicBlock', norm='in', compute_dtype='f32')
    sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 7)
    torch.save({'epoch': 1, 'model_state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, os.path.join(d, 'run3', 'latest.pth'))
    argv = ['--load', os.path.join(d, 'run3', 'latest.pth'), '--img_path', os.path.join(d, 'img'), '--class_list', os.path.join(d, 'classes.yaml'),
            '--config', os.path.join(d, 'unet8.yaml'), '--save_path', os.path.join(d, 'res'), '--dataset', 'synthetic', '--score']
    with pytest.raises(ValueError, match='INTEGRATION section 3b'):
        P.main(argv)
    done, _ = P.main(argv + ['--nifti'])
    assert done == ['BDMAP_00000009']
    args = P.get_parser(argv + ['--nifti'])
    args.class_list, args.classes = CLASSES, len(CLASSES)
    models = P.init_model(args, CLASSES)
    hu, geom = load_nifti_device(las_file['path'])
    pred, _ = predict_case(models, hu, args, CLASSES, orig_spacing=geom.spacing, orig_size=geom.size)
    out = os.path.join(args.save_path, 'BDMAP_00000009', 'predictions')
    assert sorted(os.listdir(out)) == sorted(c + '.nii.gz' for c in CLASSES)
    some = 0
    for c in CLASSES:
        h, arr = R.read_nifti_gz(os.path.join(out, c + '.nii.gz'))
        want = pred[c].cpu().numpy()
        assert want.shape == (14, 36, 40) and h['dim'][1:4] == LAS_SHAPE and h['datatype'] == 2
        assert np.array_equal(h['srow'], las_file['affine'][:3].astype(np.float32).astype(np.float64))
        assert np.array_equal(arr, R.inverse_reorient(want.astype(np.uint8), *LAS)), c
        some += int(want.sum())
    assert some > 0, 'the seeded network predicts nothing: the comparison would be empty'
    import csv
    with open(os.path.join(args.save_path, 'tumor_detection_results.csv'), newline='') as f:
        rows = list(csv.DictReader(f))
    assert [r['BDMAP_ID'] for r in rows] == ['BDMAP_00000009']
    assert P.filter_already_predicted(['BDMAP_00000009.nii.gz'], args.save_path, CLASSES, False) == []
