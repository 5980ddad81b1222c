"""Host side of crop-on-tumour (training/augmentation.py plan_crop_on_tumor and friends, training/dataset/whole_volume.py) and the numpy
restatement tests/crop_ref.py against the unmodified reference's results in tests/golden/crop.npz (tests/golden/gen_golden_crop.py).  No GPU needed."""
import json
import os
import re
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

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'crop.npz'))
CASES = list(range(len(GC.CASES)))
_INPUTS = {}


def inputs(case):
    """(image, padded packed label, padded extents) of a case as numpy, computed once."""
    key = (case['seed'], case['classes'], case['size'], case['variant'], case['pad'])
    if key not in _INPUTS:
        img, lab = GC.case_inputs(case['seed'], case['classes'], case['size'], case['variant'])
        packed = R.padded(np.packbits(lab.numpy()[0].astype(bool), axis=0), case['pad'])
        _INPUTS[key] = (R.padded(img.numpy()[0, 0], case['pad']), packed)
    return _INPUTS[key]


def plan_of(case, totals, size):
    from rsuper_amd.training import augmentation as A
    lesion, crop = GC.lesion_of(case['classes']), list(case['crop'])
    np.random.seed(case['seed'])
    torch.manual_seed(case['seed'])
    if case['fn'] == 'random_crop_on_tumor':
        tp, fp, bp = case['probs'] if case['probs'] else (None, None, None)
        return A.plan_crop_on_tumor(totals, lesion, size, crop, case['tumor_case'], tp, fp, bp, GC.FOREGROUND)
    if case['fn'] == 'tumor_crop':
        return A.plan_tumor_crop(totals, lesion, size, crop)
    if case['fn'] == 'organ_crop':
        return A.plan_organ_crop(totals, lesion, size, crop, GC.FOREGROUND)
    return A.plan_negative_crop(totals, size, crop)


def test_fixture_is_the_one_the_generator_describes():
    assert int(G['n_cases']) == len(GC.CASES)
    for k, case in enumerate(GC.CASES):
        assert int(G['seed_%d' % k]) == case['seed'] and json.loads(str(G['args_%d' % k])) == json.loads(json.dumps(case))
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'crop.npz')) < (1 << 18)
    seen = {str(G['calls_%d' % k]) for k in CASES}
    assert {'tumor_crop', 'organ_crop', 'negative_crop', 'tumor_crop>crop_3d', 'organ_crop>crop_3d', 'negative_crop>crop_3d'} <= seen
    assert {c['classes'] for c in GC.CASES} >= {5, 8, 10, 26, 42}
    small = [c for c in GC.CASES if c['pad'] is not None]
    assert any(sum(s < p for s, p in zip(c['size'], c['pad'])) == 1 for c in small)
    assert any(sum(s < p for s, p in zip(c['size'], c['pad'])) == 3 for c in small)


@pytest.mark.parametrize('k', CASES)
def test_plan_and_restatement_give_the_reference_crop(k):
    case = GC.CASES[k]
    img, packed = inputs(case)
    C = case['classes']
    size = list(packed.shape[1:])
    assert size == [int(v) for v in G['padded_%d' % k]]
    plan = plan_of(case, R.totals(packed, C), size)
    nxt = (np.random.random(), float(torch.rand(1)))
    calls = str(G['calls_%d' % k]).split('>')
    assert plan.branch == {'tumor_crop': 'tumor', 'organ_crop': 'organ', 'negative_crop': 'background'}[calls[0]]
    assert plan.fallback == (calls[-1] == 'crop_3d')
    organ = int(G['organ_%d' % k])
    if organ != -2 and calls[0] != 'negative_crop':
        assert plan.crop_organ == ('random' if organ == -1 else organ)
    nd = G['ndraws_%d' % k]
    if plan.fallback:
        origin = plan.origin
        assert origin == [int(v) for v in nd[:, 2]] and plan.column is None
    else:
        assert plan.column == (C if calls[0] == 'negative_crop' else organ)
        assert (plan.rank, plan.count) == (int(G['rank_%d' % k]), int(G['count_%d' % k]))
        assert plan.offsets == [int(v) for v in nd[:, 2]]
        center = R.kth_voxel(packed, C, plan.column, plan.rank)
        assert center == [int(v) for v in G['center_%d' % k]]
        origin = R.shifted_origin(center, case['crop'], plan.offsets, size)
    assert origin == [int(v) for v in G['origin_%d' % k]]
    # both generators stand where the reference left them
    assert nxt[0] == float(G['next_np_%d' % k]) and np.float32(nxt[1]) == G['next_torch_%d' % k]
    # the padded box of the restatement is the slice the generator verified the reference crop against
    d, h, w = case['crop']
    raw_img, raw_lab = GC.case_inputs(case['seed'], C, case['size'], case['variant'])
    got = R.box(raw_img.numpy()[0, 0], case['crop'], origin, case['pad'])
    assert got.shape == (d, h, w) and np.array_equal(got, img[origin[0]:origin[0] + d, origin[1]:origin[1] + h, origin[2]:origin[2] + w])
    assert GC.corner_of(got, size, case['size']) == origin


def test_chunk_table_sums_to_totals_and_kth_voxel_walks_it():
    case = GC.CASES[0]
    _, packed = inputs(case)
    C = case['classes']
    tab, tot = R.chunk_table(packed, C), R.totals(packed, C)
    assert tab.shape == (-(-packed[0].size // R.CHUNK), C + 1) and np.array_equal(tab.sum(0), tot)
    assert tot[3] == 0 and tot[C] > 0
    full = np.unpackbits(packed, axis=0)[:C]
    assert np.array_equal(tot[:C], full.reshape(C, -1).sum(1)) and tot[C] == (full.sum(0) == 0).sum()


def test_padded_size_is_pad_volume_pair():
    from rsuper_amd.training.augmentation import padded_size
    assert padded_size((41, 53, 67), (44, 93, 107)) == ([44, 93, 107], [1, 20, 20])
    assert padded_size((41, 53, 67), (20, 93, 10)) == ([41, 93, 67], [0, 20, 0])
    assert padded_size((41, 53, 67), None) == ([41, 53, 67], [0, 0, 0])
    a = np.ones((2, 3, 4, 5))
    assert R.padded(a, (6, 4, 8)).shape == (2, 6, 4, 8) and R.padded(a, (6, 4, 8))[:, 1:4, :, 1:6].all() and R.padded(a, (6, 4, 8)).sum() == a.sum()


def test_forg_mapping():
    from rsuper_amd.training.dataset import whole_volume as WV
    assert WV.foreground_class_names(GC.WRAP_TUMOR_NAMES) == ['kidney_left', 'kidney_right', 'liver', 'pancreas']
    assert WV.foreground_class_names(['gallbladder_lesion', 'kidney_cyst', 'kidney_lesion', 'spleen']) == ['gall_bladder', 'kidney_left', 'kidney_right', 'spleen']
    assert sorted(WV.foreground_class_indices(GC.WRAP_TUMOR_NAMES, GC.WRAP_CLASSES)) == [int(v) for v in G['wrap_forg']]
    with pytest.raises(ValueError):
        WV.foreground_class_indices(['colon_lesion'], GC.WRAP_CLASSES)
    assert WV.large_size(96, 96, 96) == [116, 136, 136]


def test_wrapper_branch_order_and_draws():
    """The wrapper's draws restated on the host: 0.4 gate, the crop's draws, then (large branch) the affine's -- origins, thetas and both generators."""
    from rsuper_amd.training import augmentation as A
    from rsuper_amd.training.dataset import whole_volume as WV
    C = len(GC.WRAP_CLASSES)
    _, lab = GC.case_inputs(GC.WRAP_SEED, C, GC.SIZE)
    packed = np.packbits(lab.numpy()[0].astype(bool), axis=0)
    totals, lesion = R.totals(packed, C), GC.lesion_of(C)
    forg = WV.foreground_class_indices(GC.WRAP_TUMOR_NAMES, GC.WRAP_CLASSES)
    d, h, w = GC.WRAP_CROP
    np.random.seed(GC.WRAP_SEED)
    torch.manual_seed(GC.WRAP_SEED)
    for i in range(GC.WRAP_LEN):
        tumor_case = sum(totals[c] for c in lesion) > 0
        large = np.random.random() < 0.4
        crop = WV.large_size(d, h, w) if large else [d, h, w]
        plan = A.plan_crop_on_tumor(totals, lesion, list(GC.SIZE), crop, tumor_case, foreground_classes=forg)
        origin = plan.origin if plan.fallback else R.shifted_origin(R.kth_voxel(packed, C, plan.column, plan.rank), crop, plan.offsets, GC.SIZE)
        assert int(large) == int(G['wrap_large'][i]) and origin == [int(v) for v in G['wrap_origins'][i]]
        if large:
            theta = A.draw_affine_3d(**GC.WRAP_ARGS)
            assert np.array_equal(theta.numpy().view(np.uint32), G['wrap_thetas'][i].view(np.uint32))
    assert np.random.random() == float(G['wrap_next_np']) and np.float32(float(torch.rand(1))) == G['wrap_next_torch']


def test_cpu_tensors_are_refused():
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.training import augmentation as A
    from rsuper_amd.training.dataset import whole_volume as WV
    img, lab = GC.case_inputs(0, 5, (8, 9, 10))
    for call in (lambda: A.random_crop_on_tumor(img, lab, [3, 4], 4, 4, 4, True),
                 lambda: A.tumor_crop(img, lab, [3, 4], 4, 4, 4),
                 lambda: A.organ_crop(img, lab, [3, 4], 4, 4, 4),
                 lambda: A.negative_crop(img, lab, [3, 4], 4, 4, 4),
                 lambda: A.crop_around_coordinate_3d(img, lab, 4, (1, 2, 3), 'center'),
                 lambda: A.pad_volume_pair(img, lab, 12, 12, 12),
                 lambda: A.class_counts(lab),
                 lambda: WV.random_crop_on_tumor(img, lab, 4, 4, 4, ['a', 'b', 'c', 'd', 'e'], [3, 4], ['a'], 0.3, 45, 0.1)):
        with pytest.raises(RSuperHipError):
            call()
    assert A.pad_volume_pair(img, lab, 8, 9, 10)[0] is img       # nothing to pad: the tensors themselves, as in the reference


def test_c_abi_is_declared_in_header_and_signatures():
    from rsuper_amd.hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    for name in ('rsuper_class_counts_workspace_bytes', 'rsuper_class_counts', 'rsuper_select_voxel', 'rsuper_crop_box'):
        m = re.search(r'(?:int|long)\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, '%s is not declared in include/rsuper_hip.h' % name
        assert name in lib._SIGS and len(lib._SIGS[name][1]) == len(m.group(1).split(','))
    assert int(re.search(r'#define\s+RSUPER_CROP_CHUNK\s+(\d+)', hdr).group(1)) == R.CHUNK
    from rsuper_amd.training import augmentation as A
    assert A.CROP_CHUNK == R.CHUNK
