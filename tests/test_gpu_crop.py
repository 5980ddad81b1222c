"""Crop-on-tumour on the device (csrc/crop.hip, training/augmentation.py, training/dataset/whole_volume.py) on a real MI355X.  Every check is
bit-exact: the kernels against the numpy restatement tests/crop_ref.py (which tests/test_crop_cpu.py pins to the unmodified reference's fixture
tests/golden/crop.npz), the reference-named functions against the fixture itself.

Shapes: (41, 53, 67) = 145591 voxels is 8 whole chunks of 16384 and a partial ninth, all extents odd, not a multiple of 16; (17, 48, 64) is a
multiple of 16 (every plane aligned); bases are shifted by 1, 7 and 15 bytes through slices of a larger buffer."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import crop_ref as R  # noqa: E402
import gen_golden_crop as GC  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'crop.npz'))
ODD, ALIGNED = (41, 53, 67), (17, 48, 64)
_CACHE = {}


def A():
    from rsuper_amd.training import augmentation
    return augmentation


def PB(packed, C):
    from rsuper_amd.training.dataset import PackedBits
    return PackedBits(packed, C)


def label(seed, C, size, variant='default'):
    """(image (1, 1, D, H, W) f32, label (1, C, D, H, W) u8, packed (P, D, H, W) u8) as numpy, computed once."""
    key = (seed, C, tuple(size), variant)
    if key not in _CACHE:
        img, lab = GC.case_inputs(seed, C, size, variant)
        _CACHE[key] = (img.numpy(), lab.numpy(), np.packbits(lab.numpy()[0].astype(bool), axis=0))
    return _CACHE[key]


def shifted(a, off):
    """a on the device with its base `off` bytes past an allocation's start."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() * t.element_size() + 16, dtype=torch.uint8, device=DEV)
    v = buf[off:off + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off % 16
    return v


def counts_of(packed_np, C, off=0, plain=False):
    """class_counts of a (B, P, D, H, W) array -> (totals (B, C + 1), table (B, chunks, C + 1)) as numpy."""
    t = shifted(packed_np, off)
    totals, ws = A()._class_counts(t, C, plain)
    torch.cuda.synchronize()
    B = packed_np.shape[0]
    return totals.cpu().numpy(), ws.cpu().numpy().view(np.int32).reshape(B, -1, C + 1)


# ------------------------------------------------------------------------------------------------------------------ totals
@pytest.mark.parametrize('C', [5, 8, 26, 42])
@pytest.mark.parametrize('B', [1, 3])
def test_totals_and_chunk_table_equal_unpackbits(C, B):
    packed = np.stack([label(20 + b, C, ODD)[2] for b in range(B)])
    totals, table = counts_of(packed, C)
    assert totals.dtype == np.int64 and table.shape[1] == 9
    for b in range(B):
        assert np.array_equal(totals[b], R.totals(packed[b], C)), (C, b)
        assert np.array_equal(table[b], R.chunk_table(packed[b], C)), (C, b)


@pytest.mark.parametrize('size', [ODD, ALIGNED, (3, 5, 7)])
@pytest.mark.parametrize('off', [0, 1, 7, 15])
def test_totals_for_any_base_alignment_and_voxel_count(size, off):
    C = 10
    packed = label(3, C, size)[2][None]
    totals, table = counts_of(packed, C, off)
    assert np.array_equal(totals[0], R.totals(packed[0], C)) and np.array_equal(table[0], R.chunk_table(packed[0], C))


@pytest.mark.parametrize('C', [5, 26])
def test_totals_of_all_zero_and_all_ones_volumes(C):
    V = ODD[0] * ODD[1] * ODD[2]
    zero = np.zeros(((C + 7) // 8,) + ODD, np.uint8)
    ones = np.packbits(np.ones((C,) + ODD, bool), axis=0)
    totals, _ = counts_of(np.stack([zero, ones]), C)
    assert totals[0].tolist() == [0] * C + [V] and totals[1].tolist() == [V] * C + [0]


def test_plain_label_gives_the_packed_label_totals():
    C = 10
    _, lab, packed = label(3, C, ODD)
    a, ta = counts_of(packed[None], C)
    b, tb = counts_of(lab, C, plain=True)
    assert np.array_equal(a, b) and np.array_equal(ta, tb)
    c = A().class_counts(torch.from_numpy(lab).long().to(DEV))
    assert c.plain and c.host(0) == a[0].tolist()


# ------------------------------------------------------------------------------------------------------------------ selection
def crafted():
    """The (41, 53, 67) label of seed 3 with class 1 set exactly at the last voxel of chunk 2, the first of chunk 3 and two more, and class 3 (empty in
    the generator) only inside the last, partial chunk."""
    if 'crafted' not in _CACHE:
        C = 10
        lab = label(3, C, ODD)[1].copy()
        flat = lab.reshape(C, -1)
        flat[1] = 0
        flat[1, [5, 3 * R.CHUNK - 1, 3 * R.CHUNK, 3 * R.CHUNK + 70]] = 1
        flat[3] = 0
        flat[3, [8 * R.CHUNK + 1, 8 * R.CHUNK + 200, flat.shape[1] - 1]] = 1
        _CACHE['crafted'] = (lab, np.packbits(lab[0].astype(bool), axis=0))
    return _CACHE['crafted']


@pytest.mark.parametrize('kind', ['packed', 'plain', 'shifted'])
def test_selection_equals_argwhere(kind):
    C = 10
    lab, packed = crafted()
    if kind == 'plain':
        counts = A().class_counts(torch.from_numpy(lab).to(DEV))
    else:
        counts = A().class_counts(PB(shifted(packed[None], 9 if kind == 'shifted' else 0), C))
    tot = counts.host(0)
    assert tot == R.totals(packed, C).tolist() and tot[1] == 4 and tot[3] == 3
    rs = np.random.RandomState(5)
    asked = []
    for col in (0, 1, 3, 9, C):                          # a large organ, the crafted classes, a lesion class in byte plane 1, the background
        ks = {0, tot[col] - 1} | ({1, 2} if col in (1, 3) else {int(k) for k in rs.randint(0, tot[col], 3)})
        asked += [(col, k) for k in sorted(ks)]
    got = [A().select_voxel(counts, col, k, tot[col], add=(0, 0, 0)) for col, k in asked]
    torch.cuda.synchronize()
    for (col, k), zyx in zip(asked, got):
        assert zyx.dtype == torch.int32 and zyx.cpu().tolist() == R.kth_voxel(packed, C, col, k), (col, k)
    # the offsets that turn real into padded coordinates
    z = A().select_voxel(counts, 1, 2, add=(1, 20, 300)).cpu().tolist()
    assert z == [a + b for a, b in zip(R.kth_voxel(packed, C, 1, 2), (1, 20, 300))]


def test_selection_in_a_batch_reads_its_own_sample():
    C = 26
    packed = np.stack([label(20 + b, C, ODD)[2] for b in range(3)])
    t = torch.from_numpy(packed).to(DEV)
    totals, table = A()._class_counts(t, C, False)
    tot = totals.cpu().tolist()
    for b in range(3):
        for col in (25, C):
            k = tot[b][col] // 2
            assert A()._select_voxel(t, C, False, table, b, col, k, tot[b][col], [0, 0, 0]).cpu().tolist() == R.kth_voxel(packed[b], C, col, k)


def test_rank_out_of_range_is_refused_on_the_host():
    from rsuper_amd.hip.lib import RSuperHipError
    counts = A().class_counts(PB(torch.from_numpy(crafted()[1][None]).to(DEV), 10))
    for col, k in ((1, 4), (1, -1), (3, 3), (2, 1 << 40)):
        with pytest.raises(RSuperHipError):
            A().select_voxel(counts, col, k)
    with pytest.raises(RSuperHipError):
        A().select_voxel(counts, 11, 0, 5)                # no such column
    empty = A().class_counts(PB(torch.zeros((1, 2, 3, 4, 5), dtype=torch.uint8, device=DEV), 10))
    with pytest.raises(RSuperHipError):
        A().select_voxel(empty, 0, 0)                     # an empty class has no voxel 0


# ------------------------------------------------------------------------------------------------------------------ box crop
BOX_SRC = (21, 23, 37)


def box_inputs(B=1):
    rs = np.random.RandomState(9)
    img = rs.standard_normal((B, 2) + BOX_SRC).astype(np.float32)
    vols = [rs.randint(0, 256, (B, p) + BOX_SRC).astype(np.uint8) for p in (2, 1, 4)]
    return img, vols


def run_box(img, vols, size, pad, **kw):
    out, outs, used = A().crop_box(None if img is None else torch.from_numpy(img).to(DEV), [torch.from_numpy(v).to(DEV) for v in vols], size, pad=pad, **kw)
    torch.cuda.synchronize()
    return (None if out is None else out.cpu().numpy()), [o.cpu().numpy() for o in outs], used.cpu().tolist()


FACES = [((0, 11, 18), (-9, 0, 0)), ((20, 11, 18), (9, 0, 0)), ((10, 0, 18), (0, -9, 0)), ((10, 22, 18), (0, 9, 0)),
         ((10, 11, 0), (0, 0, -9)), ((10, 11, 36), (0, 0, 9)), ((10, 11, 18), (1, -2, 3))]


@pytest.mark.parametrize('size', [(8, 10, 12), (7, 9, 13), (5, 3, 2)])
@pytest.mark.parametrize('pad', [None, (30, 20, 50)])
def test_box_crop_clipped_at_every_face_both_origin_forms(size, pad):
    img, vols = box_inputs()
    full, lo = A().padded_size(BOX_SRC, pad)
    for center, offset in FACES:
        cp = [c + l for c, l in zip(center, lo)]         # the centre in padded coordinates
        exp = R.shifted_origin(cp, size, offset, full)
        cdev = torch.tensor([cp], dtype=torch.int32, device=DEV)
        a_img, a_vols, a_org = run_box(img, vols, size, pad, center=cdev, offset=list(offset))
        b_img, b_vols, b_org = run_box(img, vols, size, pad, origin=exp)
        assert a_org == [exp] and b_org == [exp], (center, offset)
        assert np.array_equal(a_img.view(np.uint32), R.box(img, size, exp, pad).view(np.uint32)) and np.array_equal(a_img.view(np.uint32), b_img.view(np.uint32))
        for v, ga, gb in zip(vols, a_vols, b_vols):
            assert np.array_equal(ga, R.box(v, size, exp, pad)) and np.array_equal(ga, gb)


def test_box_crop_takes_int16_images_and_batches_past_eight_samples():
    B = 9
    rs = np.random.RandomState(4)
    hu = rs.randint(-1024, 3000, (B, 1) + BOX_SRC).astype(np.int16)
    vol = rs.randint(0, 256, (B, 3) + BOX_SRC).astype(np.uint8)
    size, pad = (9, 24, 16), (10, 30, 10)
    full, _ = A().padded_size(BOX_SRC, pad)
    orgs = [[int(rs.randint(0, f - s + 1)) for f, s in zip(full, size)] for _ in range(B)]
    out, (o,), used = run_box(hu, [vol], size, pad, origin=sum(orgs, []))
    assert out.dtype == np.float32 and used == orgs
    for b in range(B):
        assert np.array_equal(out[b], R.box(hu[b].astype(np.float32), size, orgs[b], pad)) and np.array_equal(o[b], R.box(vol[b], size, orgs[b], pad))
    as_f32 = run_box(hu.astype(np.float32), [vol], size, pad, origin=sum(orgs, []))[0]
    assert np.array_equal(out, as_f32)


def test_box_crop_refuses_bad_shapes_on_the_host():
    from rsuper_amd.hip.lib import RSuperHipError
    img, vols = box_inputs()
    for size, pad, org in (((22, 10, 12), None, [0, 0, 0]), ((8, 10, 12), None, [14, 0, 0]), ((8, 10, 12), None, [0, -1, 0]),
                           ((8, 10, 40), (0, 0, 39), [0, 0, 0]), ((0, 10, 12), None, [0, 0, 0])):
        with pytest.raises(RSuperHipError):
            run_box(img, vols, size, pad, origin=org)
    with pytest.raises(ValueError):
        A().crop_box(torch.from_numpy(img).to(DEV), [], (4, 4, 4))


def test_pad_volume_pair_is_the_zero_padded_copy():
    img, lab, packed = label(10, 10, GC.SMALL_ALL)
    want = (44, 68, 72)
    pi, pl = A().pad_volume_pair(torch.from_numpy(img).to(DEV), PB(torch.from_numpy(packed[None]).to(DEV), 10), *want)
    assert tuple(pi.shape) == (1, 1) + want and tuple(pl.shape) == (1, 10) + want
    assert np.array_equal(pi.cpu().numpy(), R.padded(img, want)) and np.array_equal(pl.packed.cpu().numpy()[0], R.padded(packed, want))
    qi, ql = A().pad_volume_pair(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).long().to(DEV), 10, 68, 10)
    assert ql.dtype == torch.int64 and np.array_equal(ql.cpu().numpy(), R.padded(lab, (10, 68, 10)))
    case = [k for k, c in enumerate(GC.CASES) if c['pad'] == (44, 93, 107)][0]
    i2, _, p2 = label(GC.CASES[case]['seed'], 10, GC.SIZE)
    ri, _ = A().pad_volume_pair(torch.from_numpy(i2).to(DEV), PB(torch.from_numpy(p2[None]).to(DEV), 10), 44, 93, 107)
    assert list(ri.shape[2:]) == [int(v) for v in G['padded_%d' % case]]


# ------------------------------------------------------------------------------------------------------------------ reference functions
def call_case(case, img, lab):
    lesion = GC.lesion_of(case['classes'])
    d, h, w = case['crop']
    np.random.seed(case['seed'])
    torch.manual_seed(case['seed'])
    if case['fn'] == 'random_crop_on_tumor':
        tp, fp, bp = case['probs'] if case['probs'] else (None, None, None)
        r = A().random_crop_on_tumor(img, lab, lesion, d, h, w, case['tumor_case'], tumor_prob=tp, foreground_prob=fp, background_prob=bp,
                                     return_crop_organ=True, class_names=list(range(case['classes'])), foreground_classes=GC.FOREGROUND, pad=case['pad'])
    elif case['fn'] == 'tumor_crop':
        r = A().tumor_crop(img, lab, lesion, d, h, w, return_crop_organ=True, pad=case['pad'])
    elif case['fn'] == 'organ_crop':
        r = A().organ_crop(img, lab, lesion, d, h, w, return_crop_organ=True, foreground_classes=GC.FOREGROUND, pad=case['pad'])
    else:
        r = A().negative_crop(img, lab, lesion, d, h, w, pad=case['pad']) + (None,)
    return r + (np.random.random(), float(torch.rand(1)))


@pytest.mark.parametrize('k', list(range(len(GC.CASES))))
def test_reference_functions_reproduce_the_fixture(k):
    case = GC.CASES[k]
    C = case['classes']
    img, lab, packed = label(case['seed'], C, case['size'], case['variant'])
    origin = [int(v) for v in G['origin_%d' % k]]
    dimg = torch.from_numpy(img).to(DEV)
    ci, cl, organ, nn, nt = call_case(case, dimg, PB(torch.from_numpy(packed[None]).to(DEV), C))
    padded = [int(v) for v in G['padded_%d' % k]]
    assert GC.corner_of(ci.cpu().numpy(), padded, case['size']) == origin
    assert nn == float(G['next_np_%d' % k]) and np.float32(nt) == G['next_torch_%d' % k]
    assert np.array_equal(ci.cpu().numpy(), R.box(img, case['crop'], origin, case['pad']))
    assert cl.C == C and np.array_equal(cl.packed.cpu().numpy()[0], R.box(packed, case['crop'], origin, case['pad']))
    if organ is not None:
        want = int(G['organ_%d' % k])
        assert organ == ('random' if want == -1 else want)
    # the same label inflated to u8: the same draws, the same crop
    ui, ul, _, un, ut = call_case(case, dimg, torch.from_numpy(lab).to(DEV))
    assert (un, ut) == (nn, nt) and torch.equal(ui, ci) and ul.dtype == torch.uint8
    assert np.array_equal(ul.cpu().numpy(), R.box(lab, case['crop'], origin, case['pad']))
    assert torch.equal(ul, cl.unpack())


def test_crop_around_coordinate_modes():
    img, lab, packed = label(3, 10, ODD)
    dimg, dlab = torch.from_numpy(img).to(DEV), PB(torch.from_numpy(packed[None]).to(DEV), 10)
    crop, zyx = [24, 28, 31], (30, 5, 60)
    fg = torch.from_numpy(lab[0, 0].astype(bool)).to(DEV)
    # 'center' (:544-549)
    exp = [min(max(0, c - -(-s // 2)), n - s) for c, s, n in zip(zyx, crop, ODD)]
    a, b, f = A().crop_around_coordinate_3d(dimg, dlab, crop, zyx, 'center', foreground=fg)
    assert np.array_equal(a.cpu().numpy(), R.box(img, crop, exp)) and np.array_equal(b.packed.cpu().numpy()[0], R.box(packed, crop, exp))
    assert f.dtype == torch.bool and np.array_equal(f.cpu().numpy()[0, 0], R.box(lab[0, 0].astype(bool), crop, exp))
    # 'random' (:513-522): three randint(min, max) draws
    np.random.seed(2)
    st = np.random.RandomState(2)
    exp = [int(st.randint(max(0, c - s), min(n - s, c + s))) for c, s, n in zip(zyx, crop, ODD)]
    a, _ = A().crop_around_coordinate_3d(dimg, dlab, crop, zyx, 'random')
    assert np.array_equal(a.cpu().numpy(), R.box(img, crop, exp)) and np.random.random() == st.random_sample()
    # 'small_rnd_shift' with host ints and with a device coordinate
    for coord in (zyx, torch.tensor(zyx, dtype=torch.int32, device=DEV)):
        np.random.seed(3)
        st = np.random.RandomState(3)
        exp = R.shifted_origin(zyx, crop, [int(st.randint(-int(s * 0.5), int(s * 0.5) + 1)) for s in crop], ODD)
        a, _ = A().crop_around_coordinate_3d(dimg, dlab, crop, coord, 'small_rnd_shift')
        assert np.array_equal(a.cpu().numpy(), R.box(img, crop, exp)) and np.random.random() == st.random_sample()


def test_two_runs_give_the_same_bytes():
    C = 26
    _, _, packed = label(20, C, ODD)
    img = torch.from_numpy(label(20, C, ODD)[0]).to(DEV)
    lab = PB(torch.from_numpy(packed[None]).to(DEV), C)
    runs = []
    for _ in range(2):
        c = A().class_counts(lab)
        tot = c.host(0)
        center = A().select_voxel(c, 24, tot[24] // 3, tot[24])
        out, (vol,), used = A().crop_box(img, (lab,), (24, 28, 30), center=center.reshape(1, 3), offset=[3, -4, 5])
        runs.append((c.table.clone(), c.totals.clone(), center, out, vol.packed, used))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ wrapper, batch
def test_large_crop_goes_into_affine_center_crop_with_identity_theta_as_the_centre_slice():
    img, _, packed = label(GC.WRAP_SEED, 10, GC.SIZE)
    d, h, w = GC.WRAP_CROP
    np.random.seed(1)
    torch.manual_seed(1)
    li, ll = A().random_crop_on_tumor(torch.from_numpy(img).to(DEV), PB(torch.from_numpy(packed[None]).to(DEV), 10), GC.lesion_of(10),
                                      d + 20, h + 40, w + 40, True, foreground_classes=GC.FOREGROUND)
    assert tuple(li.shape) == (1, 1, d + 20, h + 40, w + 40)
    ci, (cl,) = A().affine_center_crop(li, (ll,), torch.tensor(A().IDENTITY_THETA).unsqueeze(0), [d, h, w])
    assert torch.equal(ci, li[:, :, 10:10 + d, 20:20 + h, 20:20 + w]) and torch.equal(cl.packed, ll.packed[:, :, 10:10 + d, 20:20 + h, 20:20 + w])


def test_dataset_wrapper_follows_the_reference_sequence():
    from rsuper_amd.training.dataset import whole_volume as WV
    C = len(GC.WRAP_CLASSES)
    img, _, packed = label(GC.WRAP_SEED, C, GC.SIZE)
    dimg, dlab = torch.from_numpy(img).to(DEV), PB(torch.from_numpy(packed[None]).to(DEV), C)
    d, h, w = GC.WRAP_CROP
    np.random.seed(GC.WRAP_SEED)
    torch.manual_seed(GC.WRAP_SEED)
    for i in range(GC.WRAP_LEN):
        ci, cl = WV.random_crop_on_tumor(dimg, dlab, d, h, w, GC.WRAP_CLASSES, GC.lesion_of(C), GC.WRAP_TUMOR_NAMES, **GC.WRAP_ARGS)
        assert tuple(ci.shape) == (1, 1, d, h, w) and tuple(cl.shape) == (1, C, d, h, w)
        if not int(G['wrap_large'][i]):
            org = [int(v) for v in G['wrap_origins'][i]]
            assert np.array_equal(ci.cpu().numpy(), R.box(img, (d, h, w), org)) and np.array_equal(cl.packed.cpu().numpy()[0], R.box(packed, (d, h, w), org))
    assert np.random.random() == float(G['wrap_next_np']) and np.float32(float(torch.rand(1))) == G['wrap_next_torch']
    # crop_on_tumor off: the crop then goes through random_crop and keeps its shape and kind
    np.random.seed(5)
    ci, cl = WV.crop_annotated(dimg, dlab, d, h, w, GC.WRAP_CLASSES, GC.lesion_of(C), GC.WRAP_TUMOR_NAMES, crop_on_tumor=False, **GC.WRAP_ARGS)
    assert tuple(ci.shape) == (1, 1, d, h, w) and tuple(cl.shape) == (1, C, d, h, w)


def cropper_volumes():
    C = len(synth.TINY_CLASSES)
    out = []
    for seed, size, dtype in ((1, (60, 80, 76), np.float32), (2, (40, 50, 90), np.int16), (3, (56, 72, 72), np.float32)):
        img, lab = GC.case_inputs(seed, C, size)
        lab = lab.numpy()[0]
        lab[3] = lab[2] & lab[0]                          # class 3 is left empty by the generator; here it is a foreground organ
        image = (img.numpy()[0, 0] % 2000 - 1000).astype(dtype)
        out.append((image, np.packbits(lab.astype(bool), axis=0)))
    return out


def test_device_cropper_yields_the_packed_batch_calculate_loss_takes():
    from rsuper_amd.model.dim3.unet import UNet
    from rsuper_amd.training import losses_foundation as lf
    from rsuper_amd.training.dataset import PackedBits, ingest_packed_batch
    from rsuper_amd.training.dataset.whole_volume import DeviceCropper, foreground_class_indices, large_size
    classes, T = synth.TINY_CLASSES, 32
    C, vols = len(classes), cropper_volumes()
    cropper = DeviceCropper([T] * 3, classes, [1, 4], ['kidney_lesion', 'pancreatic_lesion'])

    def run():
        np.random.seed(5)
        torch.manual_seed(5)
        return cropper(vols)
    batch = run()
    P = (C + 7) // 8
    host = {'image': np.zeros((3, 1, T, T, T), np.float32), 'label': np.zeros((3, P, T, T, T), np.uint8), 'unk_channels': np.zeros((3, P, T, T, T), np.uint8),
            'mask': np.zeros((3, P, T, T, T), np.uint8), 'volumes': np.zeros((3, 10), np.float32), 'diameters': np.zeros((3, 10, 3), np.float32)}
    ref = ingest_packed_batch(host, C, device=DEV, keep_packed=True)
    assert set(batch) == set(ref)
    for k, v in ref.items():
        assert type(batch[k]) is type(v) and tuple(batch[k].shape) == tuple(v.shape) and batch[k].device.type == 'cuda', k
        if isinstance(v, PackedBits):
            assert batch[k].packed.dtype == v.packed.dtype and batch[k].packed.shape == v.packed.shape
        else:
            assert batch[k].dtype == v.dtype
    assert not batch['unk_channels'].packed.any() and not batch['mask'].packed.any() and not batch['volumes'].any() and not batch['diameters'].any()
    # the host replays the draws (the planning functions on the restatement's totals): a sample of the direct branch is the box at the planned corner
    forg = foreground_class_indices(['kidney_lesion', 'pancreatic_lesion'], classes)
    np.random.seed(5)
    torch.manual_seed(5)
    direct = 0
    for b, (image, packed) in enumerate(vols):
        pad = large_size(T, T, T)
        pimg, ppk = R.padded(image.astype(np.float32), pad), R.padded(packed, pad)
        tot, size = R.totals(ppk, C), list(ppk.shape[1:])
        large = np.random.random() < 0.4
        crop = pad if large else [T] * 3
        plan = A().plan_crop_on_tumor(tot, [1, 4], size, crop, tot[1] + tot[4] > 0, foreground_classes=forg)
        if large:
            A().draw_affine_3d(0.3, 45, 0.1)
            continue
        direct += 1
        org = plan.origin if plan.fallback else R.shifted_origin(R.kth_voxel(ppk, C, plan.column, plan.rank), crop, plan.offsets, size)
        assert np.array_equal(batch['image'][b, 0].cpu().numpy(), R.box(pimg, crop, org)), b
        assert np.array_equal(batch['label'].packed[b].cpu().numpy(), R.box(ppk, crop, org)), b
    assert 0 < direct < 3                                 # the seed gives both branches
    # determinism: the same seeds, the same bytes
    again = run()
    assert torch.equal(again['image'], batch['image']) and torch.equal(again['label'].packed, batch['label'].packed)
    # the loss takes the batch as it is
    net = UNet(1, 8, num_classes=C, compute_dtype='f32')
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, 3).items()})
    net = net.to(DEV)
    la = argparse.Namespace(loss='ball_dice_last', aux_weight=[0.5, 0.5], seg_loss=1.0, report_volume_loss_basic=0.1, volume_loss_tolerance=0.2,
                            ball_bce_weight=1.0, ball_dice_weight=1.0, ball_volume_margin=0.2, multi_ch_tumor=False, stardard_ce_ball=False,
                            classification_branch=False)
    out = net((batch['image'] / 1000.0).contiguous())
    r = lf.calculate_loss(out, batch['label'], batch['unk_channels'], la, None, batch['mask'], batch['volumes'], batch['diameters'], classes)
    r['overall'].backward()
    assert np.isfinite(float(r['overall'])) and all(torch.isfinite(p.grad).all() for p in net.parameters())


def test_dispatcher_ops_are_registered_and_refuse_cpu_tensors():
    from rsuper_amd.hip.lib import RSuperHipError
    _, lab, packed = label(3, 10, (3, 5, 7))
    counts = A().class_counts(PB(torch.from_numpy(packed[None]).to(DEV), 10))
    assert counts.host(0) == R.totals(packed, 10).tolist()
    for name in ('class_counts', 'select_voxel', 'crop_box'):
        assert hasattr(torch.ops.rsuper, name)
    totals, _ = torch.ops.rsuper.class_counts(torch.from_numpy(packed[None]).to(DEV), 10, False)
    assert totals.cpu()[0].tolist() == counts.host(0)
    with pytest.raises((NotImplementedError, RuntimeError, RSuperHipError)):
        torch.ops.rsuper.class_counts(torch.from_numpy(packed[None]), 10, False)
