"""The report-annotated crop on the device (csrc/crop_report.hip, training/augmentation.py) on a real MI355X.  Every check is bit-exact against
the numpy restatement tests/report_crop_ref.py, which tests/test_report_crop_cpu.py pins to scipy's literal denoise_mask.

Shapes: (5, 7, 9), (17, 19, 23) and (41, 53, 67): no voxel count is a multiple of 16, so every byte plane after the first is shifted against
16-byte alignment; (41, 53, 67) is eight whole chunks of 16384 voxels and a partial ninth.  Box widths 1, 63, 64, 65 and 130 put the box's edge
before, on and after a 64-bit word's edge."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import report_crop_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = [(5, 7, 9), (17, 19, 23), (41, 53, 67)]
_CACHE = {}


def A():
    from rsuper_amd.training import augmentation
    return augmentation


def PB(packed, C):
    from rsuper_amd.training.dataset import PackedBits
    return PackedBits(packed, C)


def labels(seed, C, size, density=0.03):
    """A random (C, D, H, W) bool label with a dense blob in class 0 and its np.packbits form, computed once."""
    key = (seed, C, tuple(size), density)
    if key not in _CACHE:
        rng = np.random.RandomState(seed)
        lab = rng.random_sample((C,) + tuple(size)) < density
        lab[0, size[0] // 3:size[0] // 3 + 2, 1:size[1] // 2, 2:size[2] - 1] = True
        _CACHE[key] = (lab, np.packbits(lab, axis=0))
    return _CACHE[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def read(buf, B=1):
    return A()._read_count_box(buf, B)


def sets_for(C):
    """A set inside one byte plane, one across two (when there are two), a single class, every class."""
    out = [0b101 if C > 2 else 1, 1 << (C - 1), (1 << C) - 1]
    if C > 8:
        out.append(1 << 6 | 1 << 9 | 1 << (C - 1))
    return out


# ------------------------------------------------------------------------------------------------------------------ union_bbox
@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('C', [5, 8, 10, 26, 42])
def test_union_bbox_equals_numpy(size, C):
    lab, packed = labels(1, C, size)
    t = PB(dev(packed[None]), C)
    for cset in sets_for(C):
        (count, box), = read(A().union_bbox(t, [cset]))
        assert (count, box) == R.count_bbox(R.union(packed, C, cset)), (size, C, bin(cset))


def test_union_bbox_empty_set_and_empty_class():
    C, size = 10, SIZES[1]
    lab, packed = labels(2, C, size)
    lab = lab.copy()
    lab[3] = False
    t = PB(dev(np.packbits(lab, axis=0)[None]), C)
    for cset in (0, 1 << 3):
        (count, box), = read(A().union_bbox(t, [cset]))
        assert count == 0 and box == list(size) + [-1, -1, -1] and all(lo > hi for lo, hi in zip(box[:3], box[3:]))


@pytest.mark.parametrize('size', SIZES)
def test_union_bbox_single_voxel_at_each_corner(size):
    C = 10
    for corner in np.ndindex(2, 2, 2):
        zyx = [c * (s - 1) for c, s in zip(corner, size)]
        lab = np.zeros((C,) + size, bool)
        lab[(9,) + tuple(zyx)] = True
        lab[2] = True                                          # another class everywhere: it must not be seen
        (count, box), = read(A().union_bbox(PB(dev(np.packbits(lab, axis=0)[None]), C), [1 << 9]))
        assert count == 1 and box == zyx + zyx, (size, corner)


def test_union_bbox_plain_label_and_batches_with_different_sets():
    C, size = 10, SIZES[2]
    labs = [labels(3 + b, C, size)[0] for b in range(3)]
    sets = [0b11, 1 << 9 | 1 << 2, 0]
    exp = [R.count_bbox(R.union_plain(l.astype(np.uint8) * 3, s)) for l, s in zip(labs, sets)]
    plain = dev(np.stack(labs).astype(np.uint8) * 3)
    assert read(A().union_bbox(plain, sets), 3) == exp
    packed = PB(dev(np.stack([np.packbits(l, axis=0) for l in labs])), C)
    assert read(A().union_bbox(packed, sets), 3) == exp
    assert read(A().union_bbox(plain.long(), sets), 3) == exp
    from rsuper_amd.hip import lib
    with pytest.raises(lib.RSuperHipError):
        A().union_bbox(packed, [1 << C, 0, 0])                 # a class the label does not have
    with pytest.raises(lib.RSuperHipError):
        A().union_bbox(plain.cpu(), sets)                      # no CPU kernel


def test_union_bbox_of_more_samples_than_one_launch_takes():
    C, size = 10, SIZES[1]
    labs = [labels(30 + b, C, size)[0] for b in range(11)]      # 8 + 3: two launches of the counting kernel, one fold
    sets = [1 << (b % C) | 1 << ((3 * b + 1) % C) for b in range(11)]
    sets[9] = 0
    packed = PB(dev(np.stack([np.packbits(l, axis=0) for l in labs])), C)
    assert read(A().union_bbox(packed, sets), 11) == [R.count_bbox(R.union(np.packbits(l, axis=0), C, s)) for l, s in zip(labs, sets)]


def test_bits_open_ignores_bits_past_nx_and_refuses_overlapping_buffers():
    m = box_mask(3, (9, 11, 70), 0.9)
    bits = R.to_bits(m).copy()
    bits[:, :, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(70 - 64)        # rubbish past nx in every row's last word
    out, mask, buf = A().bits_open(dev(bits.view(np.int64)), 70, 2)
    exp = R.opening(m, 2)
    assert np.array_equal(R.from_bits(out.cpu().numpy(), 70), exp) and np.array_equal(mask.cpu().numpy(), exp.astype(np.uint8))
    assert read(buf) == [R.count_bbox(exp)]
    from rsuper_amd.hip import lib
    L, t = lib.lib(), dev(R.to_bits(m).view(np.int64))
    need = L.rsuper_bits_open_workspace_bytes(9, 11, 70)
    ws = torch.empty(need // 8 + t.numel(), dtype=torch.int64, device=DEV)
    o, mk, cb = torch.empty_like(t), torch.empty(m.shape, dtype=torch.uint8, device=DEV), torch.empty(4, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda bits_, out_: (bits_, 9, 11, 70, 2, 0, 0, 0, ws.data_ptr(), need, out_, mk.data_ptr(), cb.data_ptr(), cb.data_ptr() + 8, st)  # noqa: E731
    assert L.rsuper_bits_open(*args(t.data_ptr(), o.data_ptr())) == 0
    assert L.rsuper_bits_open(*args(t.data_ptr(), t.data_ptr())) == 1                      # out == in
    assert L.rsuper_bits_open(*args(t.data_ptr(), ws.data_ptr() + 8)) == 1                 # out inside the workspace
    assert L.rsuper_bits_open(*args(ws.data_ptr() + need - 8, o.data_ptr())) == 1          # in overlapping its end
    torch.cuda.synchronize()


def test_union_bbox_on_a_shifted_base():
    C, size = 26, SIZES[1]
    _, packed = labels(5, C, size)
    exp = R.count_bbox(R.union(packed, C, 1 << 6 | 1 << 20))
    for off in (0, 1, 7, 15):
        buf = torch.empty(packed.size + 16, dtype=torch.uint8, device=DEV)
        v = buf[off:off + packed.size].view((1,) + packed.shape)
        v.copy_(torch.from_numpy(packed)[None])
        (count, box), = read(A()._union_bbox(v, C, False, [1 << 6 | 1 << 20]))
        assert (count, box) == exp, off


# ------------------------------------------------------------------------------------------------------------------ union_bits + bits_open
def box_mask(seed, shape, density):
    rng = np.random.RandomState(seed)
    m = rng.random_sample(shape) < density
    z, y, x = (max(1, s // 2) for s in shape)
    m[:z, :y, :x] |= rng.random_sample((z, y, x)) < 0.995      # a blob that survives an erosion or two
    return m


@pytest.mark.parametrize('nx', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('inside', [False, True])
def test_union_bits_and_opening_equal_the_restatement(nx, inside):
    C, nz, ny = 10, 9, 11
    pad = 2 if inside else 0
    size = (nz + 2 * pad, ny + 2 * pad, nx + 2 * pad)
    for k, density in enumerate((0.5, 0.8, 0.98)):
        lab = np.zeros((C,) + size, bool)
        m = box_mask(10 * nx + k, (nz, ny, nx), density)
        lab[1, pad:pad + nz, pad:pad + ny, pad:pad + nx] = m & (np.arange(nx) % 2 == 0)
        lab[9, pad:pad + nz, pad:pad + ny, pad:pad + nx] = m & (np.arange(nx) % 2 == 1)
        lab[4] = True
        if inside:
            lab[1, 0, 0, 0] = True                             # a voxel outside the box: the bits must not hold it
        t = PB(dev(np.packbits(lab, axis=0)[None]), C)
        bits = A().union_bits(t, 1 << 1 | 1 << 9, (pad, pad, pad, nz, ny, nx))
        assert np.array_equal(bits.cpu().numpy().view(np.uint64), R.to_bits(m)), (nx, density)
        for r in (1, 2, 3):
            out, mask, buf = A().bits_open(bits, nx, r, add=(pad, pad, pad))
            exp = R.opening(m, r)
            assert np.array_equal(R.from_bits(out.cpu().numpy(), nx), exp), (nx, density, r)
            assert np.array_equal(mask.cpu().numpy(), exp.astype(np.uint8)), (nx, density, r)
            assert read(buf) == [R.count_bbox(exp, (pad, pad, pad))], (nx, density, r)


@pytest.mark.parametrize('r', [1, 2, 3, 4])
def test_all_ones_box_of_side_2r_erodes_to_nothing_and_2r_plus_1_keeps_its_ball(r):
    for side, left in ((2 * r, False), (2 * r + 1, True)):
        m = np.ones((side,) * 3, bool)
        bits = dev(R.to_bits(m).view(np.int64))
        out, mask, buf = A().bits_open(bits, side, r)
        exp = R.opening(m, r)
        assert exp.any() == left
        assert np.array_equal(mask.cpu().numpy(), exp.astype(np.uint8)) and read(buf) == [R.count_bbox(exp)]


def test_opening_of_a_wide_box_with_many_blocks():
    m = box_mask(7, (33, 40, 200), 0.9)                        # 33 * 40 * 4 words = 21 blocks of 256
    bits = dev(R.to_bits(m).view(np.int64))
    out, mask, buf = A().bits_open(bits, 200, 3)
    exp = R.opening(m, 3)
    assert exp.any() and np.array_equal(mask.cpu().numpy(), exp.astype(np.uint8)) and read(buf) == [R.count_bbox(exp)]
    assert np.array_equal(R.from_bits(out.cpu().numpy(), 200), exp)


# ------------------------------------------------------------------------------------------------------------------ denoise_mask
def blob(shape, *boxes):
    m = np.zeros(shape, bool)
    for z, y, x, n in boxes:
        m[z:z + n, y:y + n, x:x + n] = True
    return m


@pytest.mark.parametrize('name, m', [
    ('none', blob((20, 22, 70), (1, 1, 1, 2))),                                   # the opening leaves nothing
    ('one', blob((20, 22, 70), (2, 3, 4, 7), (14, 1, 60, 2))),
    ('two', blob((20, 22, 70), (2, 3, 4, 7), (10, 12, 50, 9))),
    ('tie', blob((20, 22, 70), (11, 3, 60, 7), (2, 12, 5, 7))),                   # equal sizes: the first in C order wins
    ('empty', np.zeros((6, 7, 8), bool)),
])
def test_denoise_mask_and_the_component_step(name, m):
    exp = R.denoise_mask(m, 2)
    got = A().denoise_mask(dev(m), iterations=2)
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), exp), name
    assert exp.any() == (name in ('one', 'two', 'tie'))
    if name == 'tie':
        assert exp[2:9, 12:19, 5:12].any() and not exp[11:].any()
    if name == 'two':
        assert exp[10:19, 12:21, 50:59].any() and not exp[2:9, 3:10, 4:11].any()
    no_cc = A().denoise_mask(dev(m.astype(np.uint8)), iterations=2, connected_component=False)
    assert np.array_equal(no_cc.cpu().numpy(), R.opening(m, 2)), name


# ------------------------------------------------------------------------------------------------------------------ label_remap
def tables(seed, C_in, C_out, nvol):
    """Per volume: masks [C_out] that are ORs of 0, 1, 3 and 8 input classes, and a set of all-ones planes."""
    rng = np.random.RandomState(seed)
    masks, ones = [], []
    for v in range(nvol):
        row = []
        for j in range(C_out):
            n = (1, 3, 8, 0)[(j + v) % 4]
            row.append(sum(1 << int(c) for c in rng.choice(C_in, n, replace=False)))
        masks.append(row)
        ones.append(sum(1 << int(c) for c in rng.choice(C_out, 2, replace=False)) if v != 1 else 0)
    return masks, ones


@pytest.mark.parametrize('C_in, C_out', [(9, 10), (17, 26), (28, 42)])
@pytest.mark.parametrize('crop', [(6, 5, 7), (24, 28, 32)])
@pytest.mark.parametrize('B', [1, 9])
def test_label_remap_equals_numpy(C_in, C_out, crop, B):
    packed = np.stack([labels(40 + b, C_in, crop, 0.2)[1] for b in range(B)])
    tabs = [tables(100 + b, C_in, C_out, 3) for b in range(B)]
    outs = A().label_remap(PB(dev(packed), C_in), C_out, [t[0] for t in tabs], [t[1] for t in tabs])
    assert len(outs) == 3
    for v, o in enumerate(outs):
        got = o.packed.cpu().numpy()
        assert o.C == C_out and got.shape == (B, (C_out + 7) // 8) + crop
        for b in range(B):
            exp = R.remap(packed[b], C_in, C_out, tabs[b][0][v], tabs[b][1][v])
            assert np.array_equal(got[b], exp), (v, b)
        if C_out % 8:
            assert not (got[:, -1] & ((1 << (8 - C_out % 8)) - 1)).any()           # the padding bits of the last byte plane


def test_label_remap_one_and_two_volumes_and_refused_tables():
    C_in, C_out, crop = 17, 26, (6, 5, 7)
    packed = labels(41, C_in, crop, 0.2)[1][None]
    masks, ones = tables(5, C_in, C_out, 3)
    t = PB(dev(packed), C_in)
    for nvol in (1, 2):
        outs = A().label_remap(t, C_out, [masks[:nvol]], [ones[:nvol]])
        for v in range(nvol):
            assert np.array_equal(outs[v].packed.cpu().numpy()[0], R.remap(packed[0], C_in, C_out, masks[v], ones[v]))
    from rsuper_amd.hip import lib
    with pytest.raises(lib.RSuperHipError):
        A().label_remap(t, C_out, [[[1 << C_in] * C_out]], [[0]])
    with pytest.raises(lib.RSuperHipError):
        A().label_remap(t, C_out, [[[1] * C_out]], [[1 << C_out]])


# ------------------------------------------------------------------------------------------------------------------ run to run
def test_two_runs_give_identical_bytes():
    C, size = 26, SIZES[2]
    _, packed = labels(6, C, size)
    t = PB(dev(packed[None]), C)
    cset = 1 << 0 | 1 << 13
    box = (3, 4, 5, 30, 40, 60)
    masks, ones = tables(9, C, 10, 3)

    def run():
        bits = A().union_bits(t, cset, box)
        out, mask, buf = A().bits_open(bits, box[5], 2)
        rm = A().label_remap(t, 10, [masks], [ones])
        return [A().union_bbox(t, [cset]), bits, out, mask, buf] + [o.packed for o in rm]

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_ops_are_registered_for_the_device_only():
    C, size = 10, SIZES[0]
    _, packed = labels(8, C, size)
    A().union_bbox(PB(dev(packed[None]), C), [1])
    for name in ('union_bbox', 'union_bits', 'bits_open', 'label_remap'):
        assert hasattr(torch.ops.rsuper, name)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.rsuper.union_bbox(torch.from_numpy(packed[None]), C, False, [1])


# ------------------------------------------------------------------------------------------------------------------ end to end against the fixture
import hashlib  # noqa: E402
import json  # noqa: E402
import random  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import gen_golden_crop as GC  # noqa: E402
import gen_golden_report_crop as GR  # noqa: E402

RECS = json.loads(str(np.load(os.path.join(ROOT, 'tests', 'golden', 'report_crop.npz'))['cases']))
IDS = [c['name'] for c in GR.CASES]
ERRORS = {'KeyError': KeyError, 'AssertionError': AssertionError}


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def next_draws():
    return {'np': float(np.random.random()), 'random': random.random(), 'torch': float(torch.rand(1))}


def cropper(case, **kw):
    from rsuper_amd.training.dataset.whole_volume import DeviceCropper
    return DeviceCropper(case['crop'], GR.CLASSES[case['ufo']], [], GR.TUMOR_CLASS_NAMES, classes_ufo=GR.CLASSES_UFO[case['ufo']], **GR.ARGS, **kw)


def triple(case):
    key = ('triple', case['name'])
    if key not in _CACHE:
        img, lab, rows = GR.case_inputs(case)
        _CACHE[key] = (img, np.packbits(lab, axis=0), rows)
    return _CACHE[key]


def same_segment(a, b):
    return (sorted(a) if isinstance(a, list) else a) == (sorted(b) if isinstance(b, list) else b)


def check_volume(got, C, sums, sha, what):
    assert [int(v) for v in np.unpackbits(got, axis=0)[:C].sum((1, 2, 3))] == sums, what
    assert hashlib.sha256(got.tobytes()).hexdigest() == sha, what


@pytest.mark.parametrize('k', range(len(IDS)), ids=IDS)
def test_crop_report_reproduces_the_fixture(k):
    """The crop itself, fallbacks and the cases whose later steps raise included: chosen segment, corner, the cropped classes_UFO label, next draws."""
    from rsuper_amd.training.dataset.whole_volume import crop_report, large_size
    case, rec = GR.CASES[k], RECS[k]
    img, packed, rows = triple(case)
    ufo = GR.CLASSES_UFO[case['ufo']]
    d, h, w = case['crop']
    seed_all(case['seed'])
    ci, cl, selected = crop_report(dev(img[None, None]), PB(dev(packed[None]), len(ufo)), rows, d, h, w, ufo, GR.TUMOR_CLASS_NAMES,
                                   GR.ARGS['scale'], GR.ARGS['rotate'], GR.ARGS['translate'], pad=large_size(d, h, w))
    assert next_draws() == rec['next']
    assert same_segment(selected, rec['selected']) and not rec['affine']
    assert ci.shape == (1, 1, d, h, w) and GC.corner_of(ci.cpu().numpy(), GR.rec_full(case), case['size']) == rec['corner']
    check_volume(cl.packed.cpu().numpy()[0], len(ufo), rec['sums_ufo'], rec['sha_ufo'], 'cropped label')


@pytest.mark.parametrize('k', range(len(IDS)), ids=IDS)
def test_device_cropper_reproduces_the_fixture(k):
    case, rec = GR.CASES[k], RECS[k]
    dc = cropper(case)
    C = len(GR.CLASSES[case['ufo']])
    seed_all(case['seed'])
    if rec['error']:
        with pytest.raises(ERRORS[list(rec['error'].values())[0]]):
            dc([triple(case)])
        assert next_draws() == rec['next']                     # it raised after the crop (test_crop_report_... pins that crop), not before
        return
    batch = dc([triple(case)])
    assert next_draws() == rec['next']
    meta = dc.last_meta[0]
    assert same_segment(meta['tumor_in_crop'], rec['selected'])
    assert batch['image'].shape == (1, 1) + tuple(case['crop']) and batch['label'].C == C
    assert GC.corner_of(batch['image'].cpu().numpy(), GR.rec_full(case), case['size']) == rec['corner']
    assert meta['unknown_per_voxel'] == rec['unk_channels']
    for name, key in (('label', 'label'), ('unk_channels', 'unk')):
        check_volume(batch[name].packed.cpu().numpy()[0], C, rec['sums'][key], rec['sha'][key], name)
    if rec['selected'] == 'random':
        assert not batch['mask'].packed.any() and not batch['volumes'].any() and not batch['diameters'].any()
        return
    check_volume(batch['mask'].packed.cpu().numpy()[0], C, rec['sums']['mask'], rec['sha']['mask'], 'mask')
    assert batch['volumes'].cpu().tolist() == [rec['volumes']] and batch['diameters'].cpu().tolist() == [rec['diameters']]


@pytest.mark.parametrize('name', ['one_name', 'liver_str_open', 'tie', 'zero_after_open', 'pad_one_axis', 'pad_three_axes_fit'])
def test_crop_foreground_3d_reproduces_the_fixture(name):
    from rsuper_amd.training.dataset import reports
    from rsuper_amd.training.dataset.whole_volume import large_size
    k = IDS.index(name)
    case, rec = GR.CASES[k], RECS[k]
    img, packed, rows = triple(case)
    ufo = GR.CLASSES_UFO[case['ufo']]
    options = reports.segment_options(reports.get_tumor_segment_labels(rows))
    random.seed(case['seed'])
    seg = random.choice(options)                                  # the draw crop() makes before crop_foreground_3d's
    cset = reports.segment_class_set(seg, ufo)
    lab = PB(dev(packed[None]), len(ufo))
    out = A().crop_foreground_3d(dev(img[None, None]), lab, cset, case['crop'], pad=large_size(*case['crop']))
    if rec['outcomes'][0] != 'crop':
        assert out == rec['outcomes'][0]
        return
    ct, cl, fg = out
    c, (d, h, w) = rec['corner'], case['crop']
    assert GC.corner_of(ct.cpu().numpy(), GR.rec_full(case), case['size']) == c
    full, lo = GR.rec_full(case), [(f - s) // 2 for f, s in zip(GR.rec_full(case), case['size'])]
    plab = np.zeros((packed.shape[0],) + tuple(full), np.uint8)
    plab[:, lo[0]:lo[0] + case['size'][0], lo[1]:lo[1] + case['size'][1], lo[2]:lo[2] + case['size'][2]] = packed
    assert np.array_equal(cl.packed.cpu().numpy()[0], plab[:, c[0]:c[0] + d, c[1]:c[1] + h, c[2]:c[2] + w])
    m = R.union(plab, len(ufo), cset)
    if rec['opened']:
        m = R.denoise_mask(m, 3)
        assert [int(m.sum())] + [R.count_bbox(m)[1]] == rec['opened'][0]
    assert fg.dtype == torch.bool and np.array_equal(fg.cpu().numpy(), m[c[0]:c[0] + d, c[1]:c[1] + h, c[2]:c[2] + w])
    # the same foreground as a device mask and a plain label
    random.seed(case['seed'])
    random.choice(options)
    plain = dev(np.unpackbits(packed, axis=0)[:len(ufo)][None])
    mask = dev(R.union(packed, len(ufo), cset))
    ct2, cl2, fg2 = A().crop_foreground_3d(dev(img[None, None]), plain, mask, case['crop'], pad=large_size(*case['crop']))
    assert torch.equal(ct2, ct) and torch.equal(fg2, fg)
    assert np.array_equal(np.packbits(cl2.cpu().numpy()[0].astype(bool), axis=0), cl.packed.cpu().numpy()[0])


def test_mixed_batch_equals_the_samples_one_by_one_and_pairs_are_untouched():
    from rsuper_amd.training.dataset.whole_volume import DeviceCropper
    case = GR.CASES[IDS.index('pair')]
    img, packed, rows = triple(case)
    C = len(GR.CLASSES[17])
    pair_lab = np.packbits(labels(70, C, case['size'], 0.05)[0], axis=0)
    vols = [(img, pair_lab), (img, packed, rows), (img.astype(np.int16) % 1000, pair_lab), (img, packed, None)]
    dc = cropper(case)
    seed_all(5)
    batch = dc(vols)
    assert [m is None for m in dc.last_meta] == [True, False, True, False]
    seed_all(5)
    singles = [dc([v]) for v in vols]
    for key in ('image', 'volumes', 'diameters'):
        assert torch.equal(batch[key], torch.cat([s[key] for s in singles], 0)), key
    for key in ('label', 'unk_channels', 'mask'):
        assert torch.equal(batch[key].packed, torch.cat([s[key].packed for s in singles], 0)), key
    assert batch['unk_channels'].packed[1].any() and not batch['unk_channels'].packed[0].any() and not batch['mask'].packed[2].any()
    # a pair goes the way it went before classes_ufo existed
    plain = DeviceCropper(case['crop'], GR.CLASSES[17], [], GR.TUMOR_CLASS_NAMES, **GR.ARGS)
    for s in (3, 4):
        seed_all(s)
        a = dc(vols[:1] + vols[2:3])
        na = next_draws()
        seed_all(s)
        b = plain(vols[:1] + vols[2:3])
        assert next_draws() == na
        for key in ('image', 'volumes', 'diameters'):
            assert torch.equal(a[key], b[key])
        for key in ('label', 'unk_channels', 'mask'):
            assert torch.equal(a[key].packed, b[key].packed)
    with pytest.raises(ValueError):
        plain([(img, packed, rows)])                               # a triple needs classes_ufo


# ------------------------------------------------------------------------------------------------------------------ pairs: as the commit before triples existed
PAIRS_FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'device_cropper_pairs.json')


def run_pairs(DeviceCropper, **kw):
    """What DeviceCropper makes of two per-voxel-annotated volumes (one f32, one int16 and smaller than the padded size in every axis) under seeds
    0 .. 5, with crop_on_tumor on and off: SHA-256 of the image and of the packed label, and the next numpy draw.  tests/golden/
    device_cropper_pairs.json holds the same from the commit before DeviceCropper knew triples (recorded on an MI355X)."""
    vols = []
    for seed, size, as_int in ((3, (41, 53, 67), False), (4, (18, 20, 25), True)):
        img, lab = GC.case_inputs(seed, 10, size)
        img = img.numpy()[0, 0]
        vols.append(((img % 1000).astype(np.int16) if as_int else img, np.packbits(lab.numpy()[0].astype(bool), axis=0)))
    out = {}
    for on in (True, False):
        dc = DeviceCropper((24, 28, 32), GC.WRAP_CLASSES, [8, 9], GC.WRAP_TUMOR_NAMES, crop_on_tumor=on, **GC.WRAP_ARGS, **kw)
        for s in range(6):
            seed_all(s)
            b = dc(vols)
            assert not b['unk_channels'].packed.any() and not b['mask'].packed.any() and not b['volumes'].any()
            out['%d_%d' % (on, s)] = [hashlib.sha256(b['image'].cpu().numpy().tobytes()).hexdigest(),
                                      hashlib.sha256(b['label'].packed.cpu().numpy().tobytes()).hexdigest(), float(np.random.random())]
    return out


def test_pairs_give_what_the_previous_commit_gave():
    from rsuper_amd.training.dataset.whole_volume import DeviceCropper
    exp = json.load(open(PAIRS_FIXTURE))
    assert len(exp) == 12
    assert run_pairs(DeviceCropper, classes_ufo=GR.CLASSES_UFO[17]) == exp
