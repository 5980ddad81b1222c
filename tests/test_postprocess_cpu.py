"""CPU checks of the prediction post-processing restatement (tests/postprocess_ref.py) and of the host rules of inference/detection.py and
inference/postprocess.py: the level decomposition of eval_AUC.detection, the scipy fixture, the organ-name map and the zoom shape rule."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import postprocess_ref as R  # noqa: E402
import synth  # noqa: E402

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'postprocess.npz'))


def test_level_decomposition_equals_the_literal_scipy_loop():
    """min(max5(min3(L)), L) > t == binary_dilation(binary_erosion(B_t), iterations=2) & B_t for every threshold."""
    ndimage = pytest.importorskip('scipy.ndimage')
    box = np.ones((3, 3, 3))
    r = np.random.default_rng(0)
    for k in range(12):
        shape = tuple(int(v) for v in r.integers(1, 24, 3))
        v = ndimage.gaussian_filter(r.standard_normal(shape), 1.2)
        v = 1.0 / (1.0 + np.exp(-3.0 * (v - v.mean()) / (v.std() + 1e-12)))
        F = R.final_levels(R.levels(v, R.THRESHOLDS))
        for t, th in enumerate(R.THRESHOLDS):
            b = v > th
            a = ndimage.binary_dilation(ndimage.binary_erosion(b, structure=box), structure=box, iterations=2) & b
            assert np.array_equal(F > t, a), (shape, th)


def test_reference_reproduces_the_scipy_fixture():
    for name in sorted({k[4:-2] for k in G.files if k.startswith('det_') and k.endswith('_x')}):
        x, sp = G[f'det_{name}_x'], G[f'det_{name}_spacing']
        for erode, key in ((True, 'erode'), (False, 'plain')):
            vols, m = R.detection(x, sp, erode=erode)
            assert [vols[t] for t in R.THRESHOLDS] == [int(v) for v in G[f'det_{name}_vol_{key}']], (name, key)
            assert m == float(G[f'det_{name}_max'])
    for name in sorted({k[3:-5] for k in G.files if k.startswith('cc_') and k.endswith('_mask')}):
        shape = tuple(int(v) for v in G[f'cc_{name}_shape'])
        n = int(np.prod(shape))
        m = np.unpackbits(G[f'cc_{name}_mask'])[:n].reshape(shape)
        assert np.array_equal(R.largest_component(m), np.unpackbits(G[f'cc_{name}_out'])[:n].reshape(shape)), name
    for lname, classes in (('tiny', synth.TINY_CLASSES), ('m42', synth.MASK42_CLASSES)):
        for dt in ('u8', 'f32'):
            out = R.postprocess(G[f'om_{lname}_{dt}'], classes)
            les = np.stack([out[c] for c in classes if 'lesion' in c])
            exp = G[f'om_{lname}_{dt}_out']
            assert les.dtype == exp.dtype and np.array_equal(les.view(np.uint8), exp.view(np.uint8)), (lname, dt)


def test_empty_mask_quirk_and_tie_rule():
    assert np.array_equal(R.largest_component(np.zeros((3, 4, 5), np.uint8)), np.ones((3, 4, 5), np.uint8))
    m = np.zeros((4, 6, 8), np.uint8)
    m[3, 0, 0:3] = 1
    m[0, 5, 5:8] = 1
    assert np.array_equal(np.flatnonzero(R.largest_component(m)), np.flatnonzero(m)[:3])


def test_organ_name_map():
    from rsuper_amd.inference.postprocess import organ_planes
    organs26 = {c: i for i, c in enumerate(synth.PANTS_CLASSES) if 'lesion' not in c}
    assert organ_planes('pancreatic_lesion', organs26) == ['pancreas']
    organs42 = {c: i for i, c in enumerate(synth.MASK42_CLASSES) if 'lesion' not in c}
    expect = {'kidney_lesion': ['kidney_right', 'kidney_left'], 'liver_lesion': ['liver'], 'pancreatic_lesion': ['pancreas'],
              'adrenal_lesion': ['adrenal_gland_right', 'adrenal_gland_left'], 'lung_lesion': ['lung_right', 'lung_left'],
              'uterus_lesion': ['prostate'], 'gallbladder_lesion': ['gall_bladder'], 'bone_lesion': None, 'breast_lesion': None,
              'spleen_lesion': ['spleen'], 'colon_lesion_2': ['colon']}
    for lesion, planes in expect.items():
        assert organ_planes(lesion, organs42) == planes, lesion
        assert R.organ_of(lesion, organs42) == planes, lesion
    tiny = {c: i for i, c in enumerate(synth.TINY_CLASSES) if 'lesion' not in c}
    for lesion in ('liver_lesion', 'bone_lesion', 'lung_lesion', 'esophagus_lesion'):
        with pytest.raises(KeyError):
            organ_planes(lesion, tiny)
        with pytest.raises(KeyError):
            R.organ_of(lesion, tiny)
    for lesion in ('uterus_lesion', 'breast_lesion'):              # the 26-class list has a prostate plane
        assert organ_planes(lesion, organs26) == R.organ_of(lesion, organs26)


def test_zoom_shape_rule():
    from rsuper_amd.inference import zoom_shape
    assert zoom_shape((5, 7, 2), (0.5, 0.5, 0.5)) == (2, 4, 1)                # round half to even; n_out == 1
    assert zoom_shape((30, 26, 20), (0.55, 0.9, 0.7)) == (16, 23, 14)         # 30 * 0.55 = 16.5 -> 16, 26 * 0.9 = 23.400000000000002
    assert zoom_shape((400, 512, 512), (2.5, 0.8, 0.8)) == (1000, 410, 410)
    ndimage = pytest.importorskip('scipy.ndimage')
    r = np.random.default_rng(2)
    for _ in range(20):
        shape = tuple(int(v) for v in r.integers(1, 12, 3))
        f = tuple(float(v) for v in r.choice([0.5, 0.55, 0.7, 0.8, 1.0, 1.25, 1.5, 2.5], 3))
        assert zoom_shape(shape, f) == ndimage.zoom(np.zeros(shape), f, order=1).shape == R.zoom_shape(shape, f)


def test_postprocess_needs_the_device():
    import torch
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import postprocess_npz
    with pytest.raises(lib.RSuperHipError):
        postprocess_npz(torch.zeros((5, 4, 4, 4)), synth.TINY_CLASSES, None)
