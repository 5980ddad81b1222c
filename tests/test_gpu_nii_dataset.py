"""MI355X tests of the NIfTI -> packed-case conversion (csrc/nii_dataset.hip, dataset_conversion/) against the numpy restatement of the reference chain
(tests/nii_dataset_ref.py, itself pinned to the reference's outputs by tests/test_nii_dataset_cpu.py).  Every label comparison is bit for bit.  The image
bound is the CPU test's: 4 x the distance between the reference's float32 image and the float64 restatement on the golden fixture (1.5e-7 -> 6.0e-7, read
from tests/golden/nii_dataset.json); the test images take the fixture's HU palette, so their z-scores lie in the same range as the fixture's."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import nifti_ref as nr  # noqa: E402
import nii_dataset_ref as ndr  # noqa: E402

pytestmark = pytest.mark.gpu
IDENT = ((0, 1, 2), (False, False, False))
PALETTE = np.array([-1024, -1000, -200, 40, 300, 1200], np.int16)
with open(os.path.join(ROOT, 'tests', 'golden', 'nii_dataset.json')) as _f:
    IMAGE_BOUND = 4.0 * json.load(_f)['ref_vs_float64']


def f32(v):
    return tuple(float(np.float32(x)) for x in v)


def palette_image(shape_zyx, seed):
    return PALETTE[np.random.default_rng(seed).integers(0, len(PALETTE), size=shape_zyx)]


def blobs(shape_zyx, seed, density=0.35, value=1):
    """A mask with structure on every axis: random voxels plus a box, so that a transposed or flipped read cannot reproduce it."""
    rng = np.random.default_rng(seed)
    m = (rng.random(shape_zyx) < density)
    Z, Y, X = shape_zyx
    m[: max(1, Z // 2), : max(1, Y // 3), : max(1, X // 2)] ^= True
    return m.astype(np.int64) * value


def write_volume(path, canon_zyx, orient, spacing_xyz, datatype, bo='<'):
    perm, flip = orient
    arr = nr.inverse_reorient(canon_zyx, perm, flip)
    pix = tuple(spacing_xyz[perm[a]] for a in range(3))
    nr.write_nifti(str(path), arr, datatype, pix, bo=bo, sform=nr.affine_for(perm, flip, pix))
    return arr, perm, flip


def make_case(tmp, ct_canon, ct_orient, spacing_xyz, masks, name='case'):
    """Write <tmp>/<name>/ct.nii.gz and one mask file per entry of masks {class: (canonical array, orientation, NIfTI datatype, byte order) or None}.
    Returns (ct path, {class: path or None}, {class: (arr_ijk, perm, flip) or None} for the restatement)."""
    d = tmp / name
    (d / 'segmentations').mkdir(parents=True, exist_ok=True)
    write_volume(d / 'ct.nii.gz', ct_canon, ct_orient, spacing_xyz, 4)
    paths, ref = {}, {}
    for k, m in masks.items():
        if m is None:
            paths[k], ref[k] = None, None
            continue
        canon, orient, datatype, bo = m
        p = d / 'segmentations' / (k + '.nii.gz')
        ref[k] = write_volume(p, canon, orient, spacing_xyz, datatype, bo)
        paths[k] = str(p)
    return str(d / 'ct.nii.gz'), paths, ref


def convert(ct, paths, names, **kw):
    from rsuper_amd.dataset_conversion.nii_dataset import convert_case
    image, lab, geom = convert_case(ct, paths, names, **kw)
    torch.cuda.synchronize()
    return image, lab, geom


def expect(names, ref, size_xyz, spacing_xyz, min_size):
    return ndr.packed_labels(ndr.label_stack(names, ref, size_xyz, f32(spacing_xyz)), min_size)


def check_labels(tmp, shape_zyx, spacing_xyz, ct_orient, masks, min_size=16, seed=0):
    names = sorted(masks)
    ct, paths, ref = make_case(tmp, palette_image(shape_zyx, seed), ct_orient, spacing_xyz, masks)
    _, lab, geom = convert(ct, paths, names, min_size=min_size)
    want = expect(names, ref, shape_zyx[::-1], spacing_xyz, min_size)
    got = lab.packed[0].cpu().numpy()
    assert got.shape == want.shape == ((len(names) + 7) // 8,) + geom.shape and lab.C == len(names)
    assert np.array_equal(got, want)
    return got, geom


def test_identity_case_equals_packbits_of_the_padded_stack(tmp_path):
    shape = (9, 11, 13)
    stack = np.stack([blobs(shape, 10 + k) for k in range(3)]).astype(np.uint8)
    masks = {n: (stack[k], IDENT, 2, '<') for k, n in enumerate(['kidney', 'liver', 'spleen'])}
    got, geom = check_labels(tmp_path, shape, (1.0, 1.0, 1.0), IDENT, masks)
    assert geom.box == shape and geom.shape == (17, 17, 17) and geom.offset == (4, 3, 2)
    padded = np.pad(stack, [(0, 0), (4, 4), (3, 3), (2, 2)])
    assert np.array_equal(got, np.packbits(padded, axis=0))


def test_ct_and_masks_in_different_orientations_with_resampling(tmp_path):
    """CT 0.8 x 0.7 x 2.5 mm, not in the identity orientation; three masks in three other orientations, one of them a permutation whose unit stride is
    canonical z."""
    shape = (6, 14, 12)
    orients = [((0, 1, 2), (True, False, False)), ((2, 0, 1), (False, True, False)), ((1, 2, 0), (True, True, True))]
    masks = {n: (blobs(shape, 20 + k), orients[k], 2, '<') for k, n in enumerate(['kidney', 'liver', 'spleen'])}
    _, geom = check_labels(tmp_path, shape, (0.8, 0.7, 2.5), ((1, 0, 2), (False, True, True)), masks)
    assert geom.box == (15, 10, 10)


def test_all_48_orientations_of_one_mask(tmp_path):
    """One canonical 7 x 9 x 5 mask stored in each of the 48 orientations, as the 48 classes of one case (six groups): every plane must hold the same
    bits, and they are the canonical mask's."""
    shape = (5, 9, 7)
    canon = blobs(shape, 31)
    masks = {'c%02d' % k: (canon, o, 2, '<') for k, o in enumerate(nr.ORIENTATIONS)}
    got, _ = check_labels(tmp_path, shape, (1.0, 1.0, 1.0), nr.ORIENTATIONS[17], masks)
    bits = np.unpackbits(got, axis=0)
    assert all(np.array_equal(bits[k], bits[0]) for k in range(48)) and bits[0].sum() == canon.sum()


@pytest.mark.parametrize('C', [1, 8, 9, 17])
def test_class_counts_and_group_boundaries(tmp_path, C):
    from rsuper_amd.dataset_conversion.nii_dataset import nii_dataset_launches
    shape = (4, 6, 10)
    masks = {'c%02d' % k: (blobs(shape, 40 + k), nr.ORIENTATIONS[(5 * k) % 48], 2, '<') for k in range(C)}
    before = nii_dataset_launches()
    got, _ = check_labels(tmp_path, shape, (1.0, 1.0, 1.0), IDENT, masks)
    after = nii_dataset_launches()
    assert after['gather'] - before['gather'] == (C + 7) // 8 and after['background'] == before['background']
    tail = np.unpackbits(got, axis=0)[C:]
    assert not tail.any()                                # the padding bits of the last byte plane


@pytest.mark.parametrize('X,Y,Z,min_size', [(1, 5, 3, 1), (15, 4, 3, 1), (16, 3, 2, 1), (17, 3, 3, 1), (63, 2, 3, 1), (65, 3, 2, 1), (130, 2, 2, 1),
                                            (1, 5, 3, 16), (15, 1, 4, 16), (17, 5, 3, 16), (65, 1, 1, 1)])
def test_row_lengths_tails_and_unaligned_planes(tmp_path, X, Y, Z, min_size):
    shape = (Z, Y, X)
    masks = {n: (blobs(shape, 50 + k), nr.ORIENTATIONS[7 * k], 2, '<') for k, n in enumerate(['a', 'b', 'background', 'c'])}
    masks['background'] = None                           # the synthesised background runs over the same rows
    got, geom = check_labels(tmp_path, shape, (1.0, 1.0, 1.0), IDENT, masks, min_size=min_size)
    assert geom.shape[2] == (X if X >= min_size else X + 2 * ((min_size - X + 1) // 2))


def test_writes_stay_inside_the_plane():
    """The ops themselves on an output that lies at an odd address inside a buffer of 0xAA: the bytes in front of and behind it stay; label-map mode
    with V % 16 != 0 puts the later planes at other alignments than plane 0."""
    from rsuper_amd.dataset_conversion import nii_dataset as nd
    Z, Y, X, P = 3, 5, 7, 3
    box, off = (Z, Y, X), (1, 2, 3)
    shape = (Z + 2, Y + 4, X + 6)
    V = int(np.prod(shape))
    assert V % 16 != 0
    src = np.random.default_rng(60).integers(-2, 9, size=(Z, Y, X)).astype(np.int16)
    lut = np.random.default_rng(61).integers(0, 256, size=(6, P)).astype(np.uint8)
    desc = torch.tensor([[0, 2, Y * X, X, 1, 0, src.size, 0]], dtype=torch.int64, device='cuda')
    raw = torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).cuda()
    ix, iy, iz = (torch.arange(n, dtype=torch.int32, device='cuda') for n in (X, Y, Z))
    lut_dev = torch.from_numpy(lut).cuda()
    want = np.zeros((P,) + shape, np.uint8)
    inside = (src >= 0) & (src < 6)
    vals = np.where(inside[..., None], lut[np.clip(src, 0, 5)], 0)                        # (Z, Y, X, P)
    want[:, 1:1 + Z, 2:2 + Y, 3:3 + X] = np.moveaxis(vals, 3, 0)
    for lead in (0, 5, 16, 29):
        buf = torch.full((lead + P * V + 37,), 0xAA, dtype=torch.uint8, device='cuda')
        dst = buf[lead:lead + P * V].view((P,) + shape)
        nd._label_gather_pack_impl(raw, desc, 1, lut_dev, ix, iy, iz, [Z, Y, X], dst, 0, list(off))
        one = buf[lead:lead + V].view((1,) + shape)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:lead] == 0xAA).all() and (host[lead + P * V:] == 0xAA).all(), lead
        assert np.array_equal(host[lead:lead + P * V].reshape(want.shape), want), lead
        # pack mode into plane 0 only: the two planes behind it must keep the label-map result
        nd._label_gather_pack_impl(raw, desc, 1, None, ix, iy, iz, [Z, Y, X], one, 0, list(off))
        nd._label_background_impl(one, 1, list(off), list(box))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        p0 = np.zeros(shape, np.uint8)
        p0[1:1 + Z, 2:2 + Y, 3:3 + X] = np.where(src != 0, 0x80, 0x40)                   # class 0 where set, else the "background" (class 1)
        assert (host[:lead] == 0xAA).all() and (host[lead + P * V:] == 0xAA).all(), lead
        assert np.array_equal(host[lead:lead + V].reshape(shape), p0) and np.array_equal(host[lead + V:lead + P * V].reshape(want[1:].shape), want[1:])


def test_zero_stripe_outside_the_scan(tmp_path):
    """z spacing 2.5 -> 1 with 4 slices: 10 output slices, the last at source position 3.6 >= 3.5 is outside the scan.  Label bits are 0 there, the
    synthesised background is 1 there, and the padding is all zero, background bit included."""
    shape = (4, 6, 9)
    assert nr.nearest_table(4, float(np.float32(2.5)), 1.0)[-1] == -1
    masks = {'background': None, 'liver': (np.ones(shape, np.int64), IDENT, 2, '<'), 'spleen': (blobs(shape, 70), nr.ORIENTATIONS[9], 2, '<')}
    got, geom = check_labels(tmp_path, shape, (1.0, 1.0, 2.5), IDENT, masks)
    assert geom.box == (10, 6, 9) and geom.offset == (3, 5, 4)
    z0, y0, x0 = geom.offset
    stripe = got[0, z0 + 9, y0:y0 + 6, x0:x0 + 9]
    assert (stripe == 0x80).all()
    outside = got[0].copy()
    outside[z0:z0 + 10, y0:y0 + 6, x0:x0 + 9] = 0
    assert not outside.any() and (got[0, z0:z0 + 9, y0:y0 + 6, x0:x0 + 9] & 0x40).all()


def test_mask_dtypes_and_refusals(tmp_path):
    shape = (5, 6, 7)
    masks = {'a_u8': (blobs(shape, 80, value=255), IDENT, 2, '<'), 'b_i8': (blobs(shape, 81, value=-1), nr.ORIENTATIONS[3], 256, '<'),
             'c_i16': (blobs(shape, 82, value=300), nr.ORIENTATIONS[20], 4, '<'), 'd_u16': (blobs(shape, 83, value=40000), nr.ORIENTATIONS[33], 512, '<'),
             'e_i32': (blobs(shape, 84, value=-70000), nr.ORIENTATIONS[41], 8, '<'), 'f_be': (blobs(shape, 85, value=258), nr.ORIENTATIONS[12], 4, '>')}
    check_labels(tmp_path / 'ok', shape, (1.0, 1.0, 1.0), IDENT, masks)
    ct, paths, _ = make_case(tmp_path / 'float', palette_image(shape, 1), IDENT, (1.0, 1.0, 1.0), {'liver': (blobs(shape, 86).astype(np.float32), IDENT, 16, '<')})
    with pytest.raises(ValueError, match='liver.nii.gz'):
        convert(ct, paths, ['liver'], min_size=16)
    ct, paths, _ = make_case(tmp_path / 'size', palette_image(shape, 2), IDENT, (1.0, 1.0, 1.0), {'liver': (blobs(shape, 87), IDENT, 2, '<')})
    write_volume(tmp_path / 'size' / 'case' / 'segmentations' / 'spleen.nii.gz', blobs((5, 6, 8), 88), IDENT, (1.0, 1.0, 1.0), 2)
    paths['spleen'] = str(tmp_path / 'size' / 'case' / 'segmentations' / 'spleen.nii.gz')
    with pytest.raises(ValueError, match='spleen.nii.gz'):
        convert(ct, paths, ['liver', 'spleen'], min_size=16)
    # the same voxels, transposed in the file: the canonical size differs although the voxel count does not
    write_volume(tmp_path / 'size' / 'case' / 'segmentations' / 'spleen.nii.gz', blobs((7, 6, 5), 89), IDENT, (1.0, 1.0, 1.0), 2)
    with pytest.raises(ValueError, match='spleen.nii.gz'):
        convert(ct, paths, ['liver', 'spleen'], min_size=16)


def test_missing_files_and_background(tmp_path):
    from rsuper_amd.dataset_conversion.nii_dataset import nii_dataset_launches
    shape = (5, 7, 9)
    liver = blobs(shape, 90)
    lesion = blobs(shape, 91)                                                # overlaps the liver at random voxels
    masks = {'background': None, 'kidney': None, 'liver': (liver, IDENT, 2, '<'), 'liver_lesion': (lesion, nr.ORIENTATIONS[14], 2, '<')}
    before = nii_dataset_launches()
    got, geom = check_labels(tmp_path / 'a', shape, (1.0, 1.0, 1.0), IDENT, masks)
    after = nii_dataset_launches()
    assert after['gather'] - before['gather'] == 1 and after['background'] - before['background'] == 1
    z0, y0, x0 = geom.offset
    box = got[0, z0:z0 + 5, y0:y0 + 7, x0:x0 + 9]
    assert not (box & 0x40).any()                                            # the missing kidney is a zero plane
    assert np.array_equal((box & 0x80) != 0, (liver != 0).astype(int) + (lesion != 0) != 1) and ((liver != 0) & (lesion != 0)).any()
    masks['background'] = (blobs(shape, 92), nr.ORIENTATIONS[25], 2, '<')     # a present background file is read like any class
    before = nii_dataset_launches()
    check_labels(tmp_path / 'b', shape, (1.0, 1.0, 1.0), IDENT, masks)
    assert nii_dataset_launches()['background'] == before['background']


def test_label_map_mode(tmp_path):
    """12 values in the table, two joint classes, values outside the table (20, 300) and negative values in an int16 map; one gather launch."""
    from rsuper_amd.dataset_conversion.nii_dataset import build_lut, nii_dataset_launches
    shape = (6, 8, 10)
    table = {'c%02d' % v: v for v in range(1, 10)}
    table.update({'joint_a': [2, 3, 10], 'joint_b': [11, 12, 9]})
    names = sorted(table)
    rng = np.random.default_rng(100)
    lm = rng.choice(np.array([-5, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 20, 300]), size=shape)
    d = tmp_path / 'case'
    d.mkdir()
    orient = nr.ORIENTATIONS[29]
    sp = (0.9, 1.0, 1.6)
    write_volume(d / 'ct.nii.gz', palette_image(shape, 3), IDENT, sp, 4)
    write_volume(d / 'labels.nii.gz', lm, orient, sp, 4)
    before = nii_dataset_launches()
    _, lab, geom = convert(str(d / 'ct.nii.gz'), str(d / 'labels.nii.gz'), names, min_size=16, lut=build_lut(names, table))
    after = nii_dataset_launches()
    assert after['gather'] - before['gather'] == 1 and after['background'] == before['background']
    want = ndr.packed_labels(ndr.label_map_stack(names, table, lm, shape[::-1], f32(sp)), 16)
    got = lab.packed[0].cpu().numpy()
    assert got.shape == want.shape == (2,) + geom.shape and np.array_equal(got, want)


def test_image_population_zscore_and_padding(tmp_path):
    shape = (13, 17, 20)
    canon = palette_image(shape, 110)
    ct, paths, _ = make_case(tmp_path, canon, nr.ORIENTATIONS[38], (1.0, 1.0, 1.0), {'liver': (blobs(shape, 111), IDENT, 2, '<')})
    image, _, geom = convert(ct, paths, ['liver'], min_size=16)
    got = image.cpu().numpy().astype(np.float64)
    pop, unb = ndr.zscore(canon, 16, ddof=0), ndr.zscore(canon, 16, ddof=1)
    e0, e1 = np.abs(got - pop).max(), np.abs(got - unb).max()
    print(f'image vs ddof=0: {e0:.3e}, vs ddof=1: {e1:.3e}, bound {IMAGE_BOUND:.3e}')
    assert image.dtype == torch.float32 and got.shape == geom.shape == (17, 17, 20)
    assert e0 <= IMAGE_BOUND and e0 < e1 and e1 > 50 * IMAGE_BOUND         # ddof = 1 is 1.1e-4 relative away at 4420 voxels
    z0, y0, x0 = geom.offset
    pad = got.copy()
    pad[z0:z0 + 13, y0:y0 + 17, x0:x0 + 20] = 0
    assert not pad.any()
    m, s = np.clip(canon.astype(np.float64), -991, 500).mean(), np.clip(canon.astype(np.float64), -991, 500).std()
    ms = geom.mean_std.cpu().numpy()
    assert abs(ms[0] - m) <= 2.0 ** -23 * abs(m) and abs(ms[1] - s) <= 2.0 ** -23 * s


def test_image_default_min_size_pads_127_to_129(tmp_path):
    shape = (3, 127, 5)
    canon = palette_image(shape, 120)
    ct, paths, ref = make_case(tmp_path, canon, IDENT, (1.0, 1.0, 1.0), {'liver': (blobs(shape, 121), nr.ORIENTATIONS[10], 2, '<')})
    image, lab, geom = convert(ct, paths, ['liver'])
    assert geom.shape == (129, 129, 129) and geom.offset == (63, 1, 62) and tuple(image.shape) == geom.shape
    assert np.abs(image.cpu().numpy().astype(np.float64) - ndr.zscore(canon, 128, ddof=0)).max() <= IMAGE_BOUND
    assert np.array_equal(lab.packed[0].cpu().numpy(), expect(['liver'], ref, shape[::-1], (1.0, 1.0, 1.0), 128))


def test_nii2packed_end_to_end(tmp_path):
    import yaml
    from rsuper_amd.dataset_conversion import nii2packed
    from rsuper_amd.training.dataset import whole_ct
    src, tgt = tmp_path / 'src', tmp_path / 'tgt'
    names = ['background', 'kidney', 'liver', 'liver_lesion']
    cases = {}
    for i, (cid, shape, ct_orient) in enumerate((('BDMAP_00000011', (6, 9, 12), IDENT), ('BDMAP_00000012', (7, 10, 8), nr.ORIENTATIONS[21]))):
        canon = palette_image(shape, 130 + i)
        masks = {'background': None, 'kidney': None if i else (blobs(shape, 140 + i), nr.ORIENTATIONS[4], 2, '<'),
                 'liver': (blobs(shape, 150 + i), nr.ORIENTATIONS[30 + i], 2, '<'), 'liver_lesion': (blobs(shape, 160 + i), IDENT, 4, '<')}
        _, _, ref = make_case(src, canon, ct_orient, (1.0, 1.0, 1.0), masks, name=cid)
        cases[cid] = (canon, ref, shape)
    label_yaml = tmp_path / 'labels.yaml'
    label_yaml.write_text(yaml.dump(['liver', 'kidney', 'liver_lesion', 'background']))
    argv = ['--src_path', str(src), '--label_path', str(src), '--tgt_path', str(tgt), '--label_yaml', str(label_yaml), '--min_size', '16', '--workers', '2']
    assert nii2packed.main(argv) == sorted(cases)
    assert whole_ct.scan_root(str(tgt)) == sorted(cases) and whole_ct.read_label_names(str(tgt)) == names
    assert yaml.safe_load((tgt / 'list' / 'dataset.yaml').read_text()) == sorted(cases)
    for cid, (canon, ref, shape) in cases.items():
        img_path, lab_path = whole_ct.case_paths(str(tgt), cid)
        assert img_path.endswith(cid + '.npy') and lab_path.endswith(cid + '_gt.npy')
        img, lab = np.asarray(whole_ct.load_array(img_path)), np.asarray(whole_ct.load_array(lab_path))
        assert img.dtype == np.float32 and lab.dtype == np.uint8
        assert np.abs(img.astype(np.float64) - ndr.zscore(canon, 16, ddof=0)).max() <= IMAGE_BOUND
        assert np.array_equal(lab, expect(names, ref, shape[::-1], (1.0, 1.0, 1.0), 16))
    stamp = {f: os.path.getmtime(tgt / f) for f in os.listdir(tgt) if f.endswith('.npy')}
    assert nii2packed.main(argv) == []                                       # both cases exist: nothing is converted
    assert stamp == {f: os.path.getmtime(tgt / f) for f in stamp}
    assert nii2packed.main(argv + ['--overwrite']) == sorted(cases)
    assert nii2packed.main(argv + ['--overwrite', '--parts', '2', '--current_part', '1']) == [sorted(cases)[1]]
