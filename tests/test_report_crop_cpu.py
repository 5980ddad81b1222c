"""Host side of the report-annotated crop (training/dataset/reports.py, training/augmentation.py plan_crop_foreground) and the numpy restatement
tests/report_crop_ref.py against the unmodified reference's results in tests/golden/report_crop.npz (tests/golden/gen_golden_report_crop.py) and
against scipy's literal denoise_mask.  No GPU needed."""
import hashlib
import json
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import report_crop_ref as R  # noqa: E402
import gen_golden_report_crop as GR  # noqa: E402

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'report_crop.npz'))
RECS = json.loads(str(G['cases']))
SEGS = json.loads(str(G['segments']))
IDS = [c['name'] for c in GR.CASES]
_INPUTS = {}


def inputs(k):
    """(image, packed label, rows, padded extents, padding on the low side) of case k, padded as pad_volume_pair pads, computed once."""
    if k not in _INPUTS:
        case = GR.CASES[k]
        img, lab, rows = GR.case_inputs(case)
        full = GR.rec_full(case)
        lo = [(f - s) // 2 for f, s in zip(full, case['size'])]
        sl = tuple(slice(l, l + s) for l, s in zip(lo, case['size']))
        pimg = np.zeros(full, np.float32)
        pimg[sl] = img
        plab = np.zeros((lab.shape[0],) + tuple(full), bool)
        plab[(slice(None),) + sl] = lab
        _INPUTS[k] = (pimg, np.packbits(plab, axis=0), rows, full, lo)
    return _INPUTS[k]


def norm(v):
    """A segment dict value with everything the reference builds through set() sorted."""
    return sorted(sorted(x) if isinstance(x, list) else x for x in v) if isinstance(v, list) else v


def same_segment(a, b):
    return (sorted(a) if isinstance(a, list) else a) == (sorted(b) if isinstance(b, list) else b)


class Draws:
    """Records random.choice / random.randint / np.random.random as the generator's spy does."""

    def __enter__(self):
        self.log = []
        self._o = (random.choice, random.randint, np.random.random)

        def choice(seq):
            r = self._o[0](seq)
            self.log.append(['choice', len(seq), list(seq).index(r)])
            return r

        def randint(a, b):
            r = self._o[1](a, b)
            self.log.append(['randint', a, b, r])
            return r

        def nprandom(*a):
            r = self._o[2](*a)
            if not a:
                self.log.append(['np.random', float(r)])
            return r
        random.choice, random.randint, np.random.random = choice, randint, nprandom
        return self

    def __exit__(self, *a):
        random.choice, random.randint, np.random.random = self._o


def replay(k):
    """The plan of case k, fed the fixture's counts and boxes -> (plan, outcomes, corner, draws)."""
    from rsuper_amd.training import augmentation as A
    from rsuper_amd.training.dataset import reports
    case, rec = GR.CASES[k], RECS[k]
    _, packed, rows, full, _ = inputs(k)
    ufo = GR.CLASSES_UFO[case['ufo']]
    random.seed(case['seed'])
    np.random.seed(case['seed'])
    torch.manual_seed(case['seed'])
    outcomes, corner, nfg, nopen = [], None, 0, 0
    with Draws() as d:
        plan = reports.plan_report_crop(reports.get_tumor_segment_labels(rows))
        while plan.action not in plan.FINAL:
            cset = reports.segment_class_set(plan.tumor_segment, ufo)
            count, box = R.count_bbox(R.union(packed, len(ufo), cset))
            if plan.action == 'mask':
                plan.feed(count)
                continue
            assert [count, box] == rec['fg'][nfg]                           # the restatement's union is the reference's foreground
            nfg += 1
            out = A.ZERO_MASK if count == 0 else None
            if out is None and not A.bbox_fits(A.bbox_with_margin(box, full, 1), case['crop']):
                count, box = rec['opened'][nopen]
                nopen += 1
                out = A.ZERO_MASK if count == 0 else None
            if out is None:
                out = A.plan_crop_foreground(box, full, case['crop'])
            outcomes.append('crop' if isinstance(out, list) else out)
            corner = out if isinstance(out, list) else corner
            plan.feed(True if isinstance(out, list) else out)
        log = list(d.log)
    assert nfg == len(rec['fg']) and nopen == len(rec['opened'])
    return plan, outcomes, corner, log


def test_fixture_reaches_every_branch():
    assert [r['name'] for r in RECS] == IDS and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'report_crop.npz')) < (1 << 16)
    by = dict(zip(IDS, RECS))
    assert by['no_rows']['entered'] == ['random_crop_on_tumor'] and by['gate']['entered'] == ['random_crop']
    assert not any(r['affine'] for r in RECS) and all('corner' in r and 'sha_ufo' in r for r in RECS)     # every crop is a plain one: pinned
    assert by['one_name']['selected'] == ['head'] and sorted(by['pair']['selected']) == ['body', 'head']
    assert by['pancreas_list']['selected'] == ['pancreas'] and by['liver_str_open']['selected'] == 'liver' and by['pancreas_str']['selected'] == 'pancreas'
    assert by['empty_then_second']['entered'][:3] == ['get_random_tumor_seg_mask'] * 2 + ['crop_foreground_3d']
    assert by['empty_no_option']['entered'] == ['get_random_tumor_seg_mask', 'random_crop_on_tumor']
    assert by['one_name']['outcomes'] == ['crop'] and not by['one_name']['opened']
    assert by['liver_str_open']['outcomes'] == ['crop'] and by['liver_str_open']['opened'][0][0] > 0
    assert by['no_fit_then_second']['outcomes'] == ['mask does not fit crop size', 'crop']
    assert by['zero_after_open']['outcomes'] == ['zero mask'] and by['zero_after_open']['opened'][0][0] == 0
    assert by['tie']['opened'][0][0] == 63 and by['tie']['opened'][0][1][0] == 4
    assert by['liver_str_open']['error'] == {'get_chosen_segment_mask': 'AssertionError'} == by['pancreas_str']['error']
    pads = [sum(s < f for s, f in zip(c['size'], GR.rec_full(c))) for c in GR.CASES]
    assert {0, 1, 3} <= set(pads) and {c['ufo'] for c in GR.CASES} == {9, 17, 28}


def test_get_tumor_segment_labels_equals_the_reference():
    from rsuper_amd.training.dataset import reports
    import pandas as pd
    assert len(SEGS) == len(GR.SEGMENT_ROWS) >= 12
    for rows, exp in zip(GR.SEGMENT_ROWS, SEGS):
        for form in (rows, None if rows is None else pd.DataFrame(rows)):
            got = reports.get_tumor_segment_labels(form)
            assert set(got) == set(exp)
            for key in exp:
                assert norm(got[key]) == norm(exp[key]), (rows, key)
    with pytest.raises(NotImplementedError):
        reports.get_tumor_segment_labels(GR.SEGMENT_ROWS[2], no_pancreas_subseg=True)


def test_segment_class_sets_and_expansions():
    from rsuper_amd.training.dataset import reports
    ufo = GR.CLASSES_UFO[17]
    assert reports.segment_class_names('liver') == ['liver_segment_%d' % i for i in range(1, 9)]
    assert reports.segment_class_names(['pancreas']) == ['pancreas_head', 'pancreas_body', 'pancreas_tail']
    assert reports.segment_class_names(['left', 'segment 3']) == ['kidney_left', 'liver_segment_3']
    assert reports.segment_class_set('liver', ufo) == sum(1 << ufo.index('liver_segment_%d' % i) for i in range(1, 9))
    assert reports.segment_class_set(['head', 'body'], ufo) == 1 << ufo.index('pancreas_head') | 1 << ufo.index('pancreas_body')
    with pytest.raises(ValueError):
        reports.segment_class_set(['segment 3'], GR.CLASSES_UFO[9])
    with pytest.raises(RuntimeError):
        reports.segment_class_set(['head'], ['background', 'pancreas'], classes_ufo=ufo)


@pytest.mark.parametrize('k', range(len(IDS)), ids=IDS)
def test_plan_reproduces_the_reference_draws(k):
    rec = RECS[k]
    plan, outcomes, corner, log = replay(k)
    assert outcomes == rec['outcomes']
    assert same_segment(plan.tumor_segment, rec['selected'])
    assert log == rec['draws'][:len(log)]
    if plan.action == 'done':
        assert log == rec['draws'] and corner == rec['corner']
        assert [np.random.random(), random.random(), float(torch.rand(1))] == [rec['next']['np'], rec['next']['random'], rec['next']['torch']]
    else:
        assert plan.action == rec['entered'][-1] and rec['selected'] == 'random'


def test_plan_crop_foreground_margins_and_centre():
    from rsuper_amd.training import augmentation as A
    assert A.bbox_with_margin([0, 5, 55, 3, 9, 55], (40, 48, 56), 1) == [0, 4, 54, 4, 10, 55]
    assert A.plan_crop_foreground([5, 5, 5, 10, 10, 10], (40, 48, 56), (20, 24, 28), rand=False) == [2, 2, 2]
    assert A.plan_crop_foreground([5, 5, 5, 30, 10, 10], (40, 48, 56), (20, 24, 28)) == A.NO_FIT


@pytest.mark.parametrize('k', range(len(IDS)), ids=IDS)
def test_tables_give_the_reference_volumes(k):
    from rsuper_amd.training.dataset import reports
    from rsuper_amd.training.dataset.augmented import estimate_tumor_volume
    case, rec = GR.CASES[k], RECS[k]
    _, packed, rows, _, _ = inputs(k)
    ufo, classes = GR.CLASSES_UFO[case['ufo']], GR.CLASSES[case['ufo']]
    c, (d, h, w) = rec['corner'], case['crop']
    crop = np.ascontiguousarray(packed[:, c[0]:c[0] + d, c[1]:c[1] + h, c[2]:c[2] + w])
    present = [int(v) for v in R.unpack(crop, len(ufo)).sum((1, 2, 3))]
    assert not rec['affine'] and present == rec['sums_ufo'] and hashlib.sha256(crop.tobytes()).hexdigest() == rec['sha_ufo']
    sha = lambda v: hashlib.sha256(v.tobytes()).hexdigest()  # noqa: E731
    sums = lambda v: [int(x) for x in R.unpack(v, len(classes)).sum((1, 2, 3))]  # noqa: E731
    volumes, diameters = estimate_tumor_volume(rows, rec['selected'])
    if rec['selected'] == 'random':
        assert not any(volumes) and not diameters.any()
    else:
        assert torch.tensor(volumes).float().tolist() == rec['volumes'] and diameters.tolist() == rec['diameters']
    if 'assign_labels' in rec['error']:
        with pytest.raises({'KeyError': KeyError, 'AssertionError': AssertionError}[rec['error']['assign_labels']]):
            reports.assign_labels_tables(classes, ufo, rows, present)
        return
    ml, ol, mu, ou, unk = reports.assign_labels_tables(classes, ufo, rows, present)
    assert unk == rec['unk_channels']
    label, unk_map = R.remap(crop, len(ufo), len(classes), ml, ol), R.remap(crop, len(ufo), len(classes), mu, ou)
    assert sums(label) == rec['sums']['label'] and sums(unk_map) == rec['sums']['unk']
    assert sha(label) == rec['sha']['label'] and sha(unk_map) == rec['sha']['unk']
    if 'get_chosen_segment_mask' in rec['error']:
        with pytest.raises(AssertionError):
            reports.chosen_segment_table(classes, rec['selected'], ufo)
        return
    _, masks = reports.chosen_segment_table(classes, rec['selected'], ufo)
    if rec['selected'] == 'random':
        assert not any(masks)
        return
    mask = R.remap(label, len(classes), len(classes), masks, 0)
    assert sums(mask) == rec['sums']['mask'] and sha(mask) == rec['sha']['mask']


def test_restatement_equals_scipy_denoise_mask():
    ndi = pytest.importorskip('scipy.ndimage')

    def literal(m, r):
        final = ndi.binary_dilation(ndi.binary_erosion(m, iterations=r), iterations=r) & m
        labeled, n = ndi.label(final)
        if n < 2:
            return final
        counts = np.bincount(labeled.ravel())
        counts[0] = 0
        return labeled == np.argmax(counts)

    rng = np.random.RandomState(0)
    masks = []
    for i in range(12):
        m = rng.random_sample((12, 14, 70)) < (0.5, 0.8, 0.95, 0.98)[i % 4]
        m[:6, :7, :30] |= rng.random_sample((6, 7, 30)) < 0.99
        if i % 3 == 0:
            m[:, 0] = m[:, -1] = True                                       # touching the volume's faces
        masks.append(m)
    tie = np.zeros((20, 22, 70), bool)
    tie[11:18, 3:10, 60:67] = tie[2:9, 12:19, 5:12] = True
    masks.append(tie)
    for m in masks:
        for r in (1, 2, 3):
            assert np.array_equal(R.opening(m, r), ndi.binary_dilation(ndi.binary_erosion(m, iterations=r), iterations=r) & m)
            assert np.array_equal(R.denoise_mask(m, r), literal(m, r))
            n, box = R.count_bbox(m)                                        # the opening restricted to the mask's own bounding box is the same
            sub = m[box[0]:box[3] + 1, box[1]:box[4] + 1, box[2]:box[5] + 1]
            assert np.array_equal(R.opening(m, r)[box[0]:box[3] + 1, box[1]:box[4] + 1, box[2]:box[5] + 1], R.opening(sub, r))
        assert np.array_equal(R.from_bits(R.to_bits(m), m.shape[2]), m)


def test_restatement_equals_the_fixture_openings():
    for k, (case, rec) in enumerate(zip(GR.CASES, RECS)):
        if not rec['opened']:
            continue
        from rsuper_amd.training.dataset import reports
        _, packed, _, full, _ = inputs(k)
        ufo = GR.CLASSES_UFO[case['ufo']]
        first = rec['draws'][1][2]
        seg = reports.segment_options(reports.get_tumor_segment_labels(case['rows']))[first]
        m = R.union(packed, len(ufo), reports.segment_class_set(seg, ufo))
        assert R.count_bbox(m) == tuple(rec['fg'][0])
        got = R.count_bbox(R.denoise_mask(m, 3))
        assert [got[0], got[1]] == rec['opened'][0], case['name']


def test_header_declares_the_new_entry_points():
    from rsuper_amd.hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    for name in ('rsuper_union_bbox_workspace_bytes', 'rsuper_union_bbox', 'rsuper_union_bits', 'rsuper_bits_open_workspace_bytes', 'rsuper_bits_open',
                 'rsuper_label_remap'):
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(',')) == len(lib._SIGS[name][1]), name
