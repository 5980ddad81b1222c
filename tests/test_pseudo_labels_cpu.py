"""CPU tests of the report-guided pseudo-label refinement: the scipy restatement (tests/pseudo_labels_ref.py) against the reference's own results in
tests/golden/pseudo_labels.npz / .json, the host logic of refine_case and merge_pseudo_labels, the tool's discovery, slicing and lists, and the C ABI
surface that needs no device."""
import json
import os
import re

import numpy as np
import pytest
import torch

import pseudo_labels_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'rsuper_lesion_candidates_workspace_bytes': 4, 'rsuper_lesion_candidates_begin': 8, 'rsuper_lesion_candidates_run': 13}
J = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'pseudo_labels.json')))
CALLS = {c['name']: c for c in J['calls']}


@pytest.fixture(scope='module')
def g(golden):
    return golden['pseudo_labels']


@pytest.mark.parametrize('name', sorted(CALLS))
def test_restatement_reproduces_the_reference(g, name):
    c = CALLS[name]
    x = g[c['input'] + '_x']
    want = np.unpackbits(g[name + '_mask'])[:x.size].reshape(x.shape)
    mask, kept, its = pr.candidates(x, c['n_lesions'], c['peak_cut'], c['min_voxels'], c['min_peak'])
    assert (kept, its, int(mask.sum())) == (c['kept'], c['iterations'], c['voxels']) and np.array_equal(mask, want)


def test_fixture_covers_the_cases_of_the_issue(g):
    assert len(pr.DIRECTIONS) == 13 and all(f'dir_{i}' in CALLS for i in range(13))
    for i, d in enumerate(pr.DIRECTIONS):
        x = g[f'dir_{i}_x']
        assert np.array_equal(x, pr.direction_volume(d)) and x.shape == (16, 16, 64)
        z, y, xs = np.nonzero(x)
        assert CALLS[f'dir_{i}']['voxels'] == 12 == len(z)
        for axis, cut in ((z, 8), (y, 8), (xs, 32)):                             # the staircase crosses the tile borders of every axis it moves along
            assert axis.min() == axis.max() == cut or (axis.min() < cut <= axis.max())
    assert np.array_equal(g['ties_x'], pr.ties_volume()) and CALLS['ties']['voxels'] == 12
    got = {(c['n_lesions'], c['min_voxels']): (c['kept'], c['voxels'], c['iterations']) for c in J['calls'] if c['input'] == 'reject'}
    assert got == {(1, 11): (1, 11, 2), (2, 11): (2, 51, 3), (3, 11): (2, 51, 3), (2, 10): (2, 21, 2)}
    assert (CALLS['bridge32']['kept'], CALLS['bridge32']['voxels'], CALLS['bridge32']['min_voxels']) == (1, 7, 7)
    assert (CALLS['minpeak_eq']['kept'], CALLS['minpeak_eq']['iterations']) == (1, 1)
    assert (CALLS['minpeak_lt']['kept'], CALLS['minpeak_lt']['iterations']) == (0, 0)
    assert g['minpeak_eq_x'].max() == np.float32(0.01) and g['minpeak_lt_x'].max() == np.nextafter(np.float32(0.01), np.float32(0))
    assert (CALLS['zero']['n_lesions'], CALLS['zero']['kept'], CALLS['zero']['voxels']) == (0, 0, 0)
    assert (CALLS['plateau']['kept'], CALLS['plateau']['voxels']) == (2, 64) and g['plateau_x'].shape == (9, 9, 70)
    assert (CALLS['snake']['kept'], CALLS['snake']['voxels']) == (1, 5759) and g['snake_x'].shape == (17, 18, 70)
    assert [g[f'smooth_{i}_x'].shape for i in range(3)] == pr.SMOOTH_SHAPES
    for i in range(3):
        assert [(CALLS[f'smooth_{i}_{j}'][k]) for j in range(5) for k in ('n_lesions', 'peak_cut', 'min_voxels', 'min_peak')] == \
            [v for ps in pr.SMOOTH_PARAMS for v in ps]
    assert CALLS['smooth_0_2']['kept'] < 60 and CALLS['smooth_0_2']['iterations'] > 150
    assert (CALLS['speckle']['iterations'], CALLS['speckle']['kept'], CALLS['speckle']['voxels'], CALLS['speckle']['peak_cut']) == (49, 5, 69, 0.6)
    assert [f['included'] for f in J['case']['folders']] == [True, False, False, False, True, False, True]


def test_the_threshold_is_a_float32_product(g):
    """bridge32: the joining voxel equals float32(0.4) * peak rounded to float32 and lies below the float64 product, so a float64 threshold cuts the
    component in two and nothing reaches min_voxels = 7."""
    x = g['bridge32_x']
    p = x.max()
    thr32 = np.float32(np.float32(0.4) * p)
    assert p == pr.BRIDGE_PEAK and x[1, 1, 3] == thr32 and float(thr32) < 0.4 * float(p)
    assert pr.candidates(x, 1, min_voxels=7)[1] == 1
    from scipy import ndimage
    lab, n = ndimage.label(x.astype(np.float64) >= 0.4 * float(p), structure=pr.BOX26)
    assert n == 2


class _Extractor:
    """Stands in for extract_lesion_candidates: plane k yields found[k] candidates and a mask of k + 1."""

    def __init__(self, found):
        self.found, self.calls = found, []

    def __call__(self, stack, counts):
        self.calls.append((tuple(stack.shape), list(counts), stack.clone()))
        return torch.stack([torch.full(stack.shape[1:], k + 1, dtype=torch.uint8) for k in range(stack.shape[0])]), self.found[:len(counts)]


def test_refine_case_decisions_with_a_stubbed_extractor():
    from rsuper_amd.baselines.pseudo_labels import refine_case
    from rsuper_amd.baselines.pseudo_labels.pseudo_label_report_refinement import lesion_column
    classes = ['liver', 'Liver_lesion', 'kidney_lesion', 'pancreatic_lesion_extra', 'spleen']
    assert lesion_column('Liver_lesion') == 'number of liver lesion instances'
    assert lesion_column('pancreatic_lesion_extra') == 'number of pancreatic lesion instances'
    raw = torch.arange(5 * 2 * 3 * 4, dtype=torch.float32).reshape(5, 2, 3, 4)
    row = {'number of liver lesion instances': 2, 'number of kidney lesion instances': 0, 'number of pancreatic lesion instances': 1.0}
    ex = _Extractor([2, 1])
    ok, masks = refine_case(raw, classes, row, extractor=ex)
    assert ok and sorted(masks) == ['Liver_lesion', 'pancreatic_lesion_extra']                 # no mask for a zero count, none for organs
    assert ex.calls[0][:2] == ((2, 2, 3, 4), [2, 1]) and torch.equal(ex.calls[0][2], raw[[1, 3]])
    assert int(masks['Liver_lesion'][0, 0, 0]) == 1 and int(masks['pancreatic_lesion_extra'][0, 0, 0]) == 2
    assert refine_case(raw, classes, row, extractor=_Extractor([2, 0])) == (False, {})       # found < n
    assert refine_case(raw, classes, row, extractor=_Extractor([1, 1])) == (False, {})
    assert refine_case(raw, classes, row, extractor=_Extractor([5, 1]))[0]                     # more than asked for cannot happen, but is no failure
    for bad in (None, {k: v for k, v in row.items() if 'kidney' not in k}, dict(row, **{'number of liver lesion instances': float('nan')}),
                dict(row, **{'number of liver lesion instances': None}), dict(row, **{'number of pancreatic lesion instances': 'two'})):
        ex = _Extractor([2, 1])
        assert refine_case(raw, classes, bad, extractor=ex) == (False, {}) and not ex.calls   # decided before any volume is touched
    ex = _Extractor([])
    none = {k: -1 for k in row}
    assert refine_case(raw, classes, none, extractor=ex) == (True, {}) and not ex.calls
    assert refine_case(raw, ['liver', 'spleen'], None, extractor=ex) == (True, {})           # no lesion class: nothing to ask of the report
    ex = _Extractor([2, 1])
    four = torch.stack([raw, -raw], dim=-1)
    ok, _ = refine_case(four, classes, row, extractor=ex)
    assert ok and torch.equal(ex.calls[0][2], raw[[1, 3]])                                   # [..., 0]
    with pytest.raises(ValueError):
        refine_case(raw[:4], classes, row, extractor=_Extractor([2, 1]))


def test_merge_plan_orders_planes_like_the_numpy_form():
    from rsuper_amd.baselines.pseudo_labels.to_npz import merge_plan
    r = np.random.default_rng(3)
    organ_names = ['spleen', 'liver', 'kidney_left', 'aorta']
    organs = r.integers(0, 2, (4, 3, 4, 5)).astype(np.uint8)
    labels = ['liver_lesion', 'aorta', 'kidney_lesion', 'liver', 'pancreatic_lesion', 'spleen', 'kidney_left']
    masks = {'liver_lesion': r.integers(0, 2, (3, 4, 5)).astype(np.uint8), 'pancreatic_lesion': r.integers(0, 2, (3, 4, 5)).astype(np.uint8),
             'unused_lesion': np.ones((3, 4, 5), np.uint8)}
    plan = merge_plan(organ_names, masks, labels)
    assert plan == [('organ', 3), ('organ', 2), ('zeros', 'kidney_lesion'), ('organ', 1), ('lesion', 'liver_lesion'), ('lesion', 'pancreatic_lesion'),
                    ('organ', 0)]
    built = np.stack([organs[key] if kind == 'organ' else masks[key] if kind == 'lesion' else np.zeros((3, 4, 5), np.uint8) for kind, key in plan])
    assert np.array_equal(built, pr.merge_numpy(organs, organ_names, masks, labels))
    with pytest.raises(AssertionError):
        merge_plan(organ_names, masks, labels + ['stomach'])


def test_slice_indices_and_yaml_helpers_equal_the_reference(tmp_path):
    from rsuper_amd.baselines.pseudo_labels import dump_yaml, load_yaml, slice_indices
    assert len(J['slices']) == sum(parts for n in range(8) for parts in range(1, 4))
    for n, parts, part, start, stop in J['slices']:
        s = slice_indices(n, parts, part)
        assert (s.start, s.stop, s.step) == (start, stop, None)
    assert [list(range(7))[slice_indices(7, 3, k)] for k in range(3)] == [[0, 1, 2], [3, 4], [5, 6]]
    names = J['yaml']['names']
    path = tmp_path / 'list' / 'dataset.yaml'                                                # the folder does not exist yet
    dump_yaml(path, iter(names))
    assert path.read_text() == J['yaml']['text'] and load_yaml(path) == set(names)
    assert load_yaml(tmp_path / 'missing.yaml') == set()
    dump_yaml(path, [])
    assert load_yaml(path) == set()


def _tree(tmp_path, with_raw):
    """An input tree: four folders with probabilities, one without predictions_raw, one with an empty predictions_raw."""
    root = tmp_path / 'in'
    for cid in with_raw:
        d = root / (cid + '.npz') / 'predictions_raw'
        d.mkdir(parents=True)
        np.save(d / 'liver_lesion.npy', np.zeros((2, 2, 2), np.float32))
        np.savez(d / 'kidney_lesion.npz', probs=np.ones((2, 2, 2, 3), np.float32))
        (d / 'notes.txt').write_text('not a probability file')
    e1 = root / 'BDMAP_00000090.npz' / 'predictions'
    e1.mkdir(parents=True)
    np.savez(e1 / 'liver_lesion.npz', mask=np.ones((2, 2, 2), np.uint8))
    (root / 'BDMAP_00000091.npz' / 'predictions_raw').mkdir(parents=True)
    (root / 'stray.npz').write_bytes(b'')                                                    # a file, not a case folder
    return root


def test_tool_discovery_slicing_and_lists(tmp_path, monkeypatch):
    from rsuper_amd.hip import lib
    from rsuper_amd.tools import refine_pseudo_labels as tool
    ids = ['BDMAP_00000004', 'BDMAP_00000001', 'BDMAP_00000003', 'BDMAP_00000002']
    root = _tree(tmp_path, ids)
    empty, full = tool.discover(root)
    assert sorted(tool.case_id(p) for p in empty) == ['BDMAP_00000090', 'BDMAP_00000091']
    assert sorted(tool.case_id(p) for p in full) == sorted(ids)
    files = tool.probability_files(full[0])
    assert [tool.class_of(p) for p in files] == ['kidney_lesion', 'liver_lesion']
    assert tool.load_probability(files[0]).shape == (2, 2, 2) and tool.load_probability(files[0]).dtype == np.float32     # first array, [..., 0]
    assert tool.case_id('x/BDMAP_00000007.nii.gz') == 'BDMAP_00000007' and tool.class_of('a/b/colon_lesion.nii.gz') == 'colon_lesion'
    nii = tmp_path / 'liver_lesion.nii.gz'
    nii.write_bytes(b'')
    with pytest.raises(RuntimeError, match='liver_lesion.nii.gz'):
        tool.load_probability(nii)
    with pytest.raises(ValueError, match='case folders'):
        tool.discover(tmp_path / 'in' / 'BDMAP_00000090.npz')

    meta = tmp_path / 'meta.csv'
    meta.write_text('BDMAP ID,number of liver lesion instances,number of kidney lesion instances,sex\n'
                    'BDMAP_00000001,2,,F\nBDMAP_00000002,1.0,0,M\nBDMAP_00000003,two,1,F\n')
    m = tool.read_metadata(meta)
    assert sorted(m) == ['BDMAP_00000001', 'BDMAP_00000002', 'BDMAP_00000003']
    assert m['BDMAP_00000001']['number of liver lesion instances'] == 2 and np.isnan(m['BDMAP_00000001']['number of kidney lesion instances'])
    assert m['BDMAP_00000002']['number of liver lesion instances'] == 1.0 and m['BDMAP_00000003']['number of liver lesion instances'] == 'two'

    seen = []

    def fake_case(folder, meta_rows, out_root, device='cuda'):
        cid = tool.case_id(folder)
        seen.append(cid)
        ok = cid != 'BDMAP_00000003'
        if ok:
            (out_root / cid).mkdir(parents=True, exist_ok=True)
        return cid, ok, {}

    monkeypatch.setattr(tool, 'process_case', fake_case)
    monkeypatch.setattr(lib, 'require_device', lambda: None)
    out = tmp_path / 'out'
    args = ['--input_dir', str(root), '--metadata', str(meta), '--out_npz_dir', str(out)]
    kept, skipped = tool.main(args + ['--parts', '2', '--part', '1'])
    assert seen == ['BDMAP_00000003', 'BDMAP_00000004']                                      # the second half of the sorted pending folders
    assert kept == ['BDMAP_00000004', 'BDMAP_00000090', 'BDMAP_00000091'] and skipped == ['BDMAP_00000003']
    assert (out / 'BDMAP_00000090' / 'liver_lesion.npz').exists() and (out / 'BDMAP_00000091').is_dir()
    from rsuper_amd.baselines.pseudo_labels import load_yaml
    assert load_yaml(out / 'list' / 'dataset.yaml') == set(kept) and load_yaml(out / 'list' / 'skipped.yaml') == set(skipped)
    del seen[:]
    kept, skipped = tool.main(args)                                                          # what is listed is not done again
    assert seen == ['BDMAP_00000001', 'BDMAP_00000002']
    assert kept == ['BDMAP_00000001', 'BDMAP_00000002', 'BDMAP_00000004', 'BDMAP_00000090', 'BDMAP_00000091'] and skipped == ['BDMAP_00000003']
    del seen[:]
    tool.main(args)
    assert seen == []
    with pytest.raises(ValueError):
        tool.main(args + ['--parts', '2', '--part', '2'])
    with pytest.raises(ValueError):
        tool.main(args + ['--tgt_path', str(tmp_path / 'tgt')])


def test_symbols_are_declared_and_bound_with_matching_arity():
    from rsuper_amd.hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, arity in NEW_SYMBOLS.items():
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/rsuper_hip.h'
        params = [p for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']
        assert len(params) == arity == len(lib._SIGS[name][1]), name
        assert hasattr(lib.lib(), name)
    assert 'pseudo_label.hip' in open(os.path.join(ROOT, 'r-super_amd', 'csrc', 'Makefile')).read()


def test_argument_validation_without_a_device():
    """Everything here is rejected before a launch (the pointers are never dereferenced on the host)."""
    import ctypes
    from rsuper_amd.hip import lib
    L = lib.lib()
    assert L.rsuper_lesion_candidates_workspace_bytes(1, 4, 5, 6) == 128 * 4                  # parent words, padded to 64 per plane
    assert L.rsuper_lesion_candidates_workspace_bytes(3, 16, 16, 64) == 3 * 16 * 16 * 64 * 4
    assert L.rsuper_lesion_candidates_workspace_bytes(64, 1, 1, 1) == 64 * 64 * 4
    for bad in [(0, 4, 4, 4), (65, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 2048, 2048, 513)]:
        assert L.rsuper_lesion_candidates_workspace_bytes(*bad) == 0
    assert L.rsuper_lesion_candidates_workspace_bytes(1, 2048, 2048, 512) == (1 << 31) * 4     # 2^31 voxels are allowed
    work, out, state, ws = 4096, 8192, 16384, 32768                                           # stand-ins for device addresses
    n = (ctypes.c_int * 2)(1, 2)
    for bad in [(None, 2, 4, 4, 4, n, state), (out, 2, 4, 4, 4, None, state), (out, 2, 4, 4, 4, n, None), (out, 0, 4, 4, 4, n, state),
                (out, 65, 4, 4, 4, n, state), (out, 2, 0, 4, 4, n, state), (out, 1, 2048, 2048, 513, n, state)]:
        assert L.rsuper_lesion_candidates_begin(*bad, None) == 1
    ok = (work, out, 2, 4, 4, 4, 0.4, 11, 0.01, state, ws, 1)
    for k, v in [(0, None), (1, None), (9, None), (10, None), (2, 0), (2, 65), (3, 0), (5, -2), (6, 0.0), (6, -0.4), (6, 1.0000001), (6, float('nan')),
                 (8, 0.0), (8, -1.0), (8, float('nan')), (7, 0), (7, -3), (11, 0), (11, -1)]:
        assert L.rsuper_lesion_candidates_run(*(ok[:k] + (v,) + ok[k + 1:]), None) == 1, (k, v)
    assert L.rsuper_lesion_candidates_run(*(ok[:3] + (2048, 2048, 513) + ok[6:]), None) == 1


def test_python_errors_that_need_no_device():
    from rsuper_amd.baselines.pseudo_labels import DEFAULT_BATCH, extract_lesion_candidates, last_state, merge_pseudo_labels
    from rsuper_amd.baselines.pseudo_labels.pseudo_label_report_refinement import _check_params
    from rsuper_amd.hip.lib import RSuperHipError
    assert torch.ops.rsuper.lesion_candidates.default._schema.name == 'rsuper::lesion_candidates'
    assert str(torch.ops.rsuper.lesion_candidates.default._schema) == ('rsuper::lesion_candidates(Tensor prob, int[] n_lesions, float peak_cut, int min_voxels, '
                                                                       'float min_peak, int batch) -> (Tensor mask, Tensor state)')
    assert torch._C._dispatch_has_kernel_for_dispatch_key('rsuper::lesion_candidates', 'CUDA')
    assert not torch._C._dispatch_has_kernel_for_dispatch_key('rsuper::lesion_candidates', 'CPU')
    with pytest.raises(RSuperHipError):
        extract_lesion_candidates(torch.zeros(2, 3, 4), 1)
    with pytest.raises(RSuperHipError):
        extract_lesion_candidates(np.zeros((2, 3, 4), np.float32), 1)
    with pytest.raises(RSuperHipError):
        merge_pseudo_labels(torch.zeros(1, 2, 3, 4, dtype=torch.uint8), ['liver'], {}, ['liver'])
    with pytest.raises(NotImplementedError):
        torch.ops.rsuper.lesion_candidates(torch.zeros(1, 2, 3, 4), [1], 0.4, 11, 0.01, 4)
    _check_params(0.40, 11, 0.01, DEFAULT_BATCH)
    _check_params(1.0, 1, 1e-45, 1)
    for bad in [(0.0, 11, 0.01, 4), (-0.1, 11, 0.01, 4), (1.0000001, 11, 0.01, 4), (1e-50, 11, 0.01, 4), (float('nan'), 11, 0.01, 4),
                (0.4, 0, 0.01, 4), (0.4, 2.5, 0.01, 4), (0.4, 11, 0.0, 4), (0.4, 11, -1.0, 4), (0.4, 11, 1e-50, 4), (0.4, 11, float('nan'), 4),
                (0.4, 11, 0.01, 0), (0.4, 11, 0.01, 1.5)]:
        with pytest.raises(ValueError):
            _check_params(*bad)
    assert DEFAULT_BATCH >= 1 and set(last_state) == {'kept', 'iterations', 'reads', 'batch'}


def test_restatement_ends_on_a_nan_volume():
    """A NaN is the caller's error and the result unspecified, but the loop ends: in the reference's form NaN is the maximum, nothing passes the NaN
    threshold, the label of the seed is the background's and the whole volume is taken in one pass.  (The device ends such a plane with no pass at
    all, tests/test_gpu_pseudo_labels.py.)"""
    x = pr.ties_volume()
    x[3, 3, 3] = np.nan
    mask, kept, its = pr.candidates(x, 3)
    assert its == 1 and kept == 1 and mask.all()
    mask, kept, its = pr.candidates(x, 3, min_voxels=x.size + 1)
    assert its == 1 and kept == 0 and not mask.any()


def test_yaml_helpers_and_label_lists_without_pyyaml(tmp_path, monkeypatch):
    import sys
    from rsuper_amd.baselines.pseudo_labels import dump_yaml, load_yaml
    monkeypatch.setitem(sys.modules, 'yaml', None)                                           # `import yaml` now raises ModuleNotFoundError
    with pytest.raises(ModuleNotFoundError):
        import yaml  # noqa: F401
    names = ['liver_lesion', 'aorta', 'kidney left']
    dump_yaml(tmp_path / 'list' / 'label_names.yaml', names)
    assert (tmp_path / 'list' / 'label_names.yaml').read_text() == '- liver_lesion\n- aorta\n- kidney left\n'
    assert load_yaml(tmp_path / 'list' / 'label_names.yaml') == set(names)
    (tmp_path / 'pyyaml.yaml').write_text(J['yaml']['text'])                                   # what PyYAML wrote reads back the same way
    assert load_yaml(tmp_path / 'pyyaml.yaml') == set(J['yaml']['names'])


def test_training_label_checks_the_image_before_it_writes(tmp_path):
    import argparse
    from rsuper_amd.tools import refine_pseudo_labels as tool
    organs, tgt = tmp_path / 'organs', tmp_path / 'tgt'
    organs.mkdir(), tgt.mkdir()
    np.savez_compressed(organs / 'BDMAP_00000001_gt.npz', np.zeros((1, 2, 2, 2), np.int8))
    a = argparse.Namespace(organs_path=organs, tgt_path=tgt, packed=False)
    with pytest.raises(ValueError, match='BDMAP_00000001'):
        tool.write_training_label('BDMAP_00000001', {}, a, ['liver'], ['liver'])
    assert list(tgt.iterdir()) == []
