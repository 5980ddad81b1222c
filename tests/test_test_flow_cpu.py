"""Host tests of the test flow (predict_abdomenatlas / test_with_reports / eval_AUC / calculate_sensitivity_specificity[_F1_AUC]) against
tests/golden/test_flow.npz + test_flow.json, which the unmodified reference wrote (tests/golden/gen_golden_test_flow.py).  Every comparison is
exact: integer counts and CSV text."""
import ctypes
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import test_flow_ref as fr  # noqa: E402

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'test_flow.npz'))
META = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'test_flow.json')))
CONF = [i / 10 for i in range(1, 10)]


def det_volume(case):
    if f'det_{case["name"]}_x' in G.files:
        return G[f'det_{case["name"]}_x']
    n = int(np.prod(case['shape']))
    return np.unpackbits(G[f'det_{case["name"]}_bits'])[:n].reshape(case['shape'])


def text(key):
    return G[key].tobytes().decode()


def write_tables(d):
    gt = os.path.join(d, 'gt.csv')
    open(gt, 'w').write(text('csv_gt'))
    for t in CONF:
        open(os.path.join(d, f'tumor_detection_results_th{t}.csv'), 'w').write(text(f'csv_pred_th{t}'))
    return gt


@pytest.mark.parametrize('case', META['det'], ids=[c['name'] for c in META['det']])
def test_numpy_restatement_matches_the_reference(case):
    v = det_volume(case)
    assert fr.zoom_shape(case['shape'], case['spacing']) == tuple(case['out_shape'])
    assert fr.detection_binary(v, case['spacing'], case['th'], case['erode']) == case['expected']
    assert fr.detection_binary(v, case['spacing'], case['th'], False) == case['plain']
    assert fr.detection_binary(v, case['spacing'], case['th'], case['erode'], clamp=True) == case['clamped']


def test_fixture_covers_what_it_is_there_for():
    det = META['det']
    assert len(det) >= 12
    assert all(c['expected'] > 0 for c in det if c['erode'])
    assert 2 * sum(c['expected'] != c['plain'] for c in det) >= len(det)
    assert sum(bool(c['quirk_axes']) and c['clamped'] != c['expected'] for c in det) >= 2
    shapes = {(tuple(c['shape']), tuple(c['out_shape'])) for c in det}
    for pair in (((9, 17, 33), (9, 17, 33)), ((6, 11, 16), (9, 16, 80)), ((20, 40, 70), (10, 20, 35)), ((2, 9, 9), (1, 9, 9))):
        assert pair in shapes
    up = next(c for c in det if c['name'] == 'up_f32')
    assert (det_volume(up) == np.float32(up['th'])).any()                       # values exactly at th, which must not count


def test_sensitivity_specificity_csv_is_byte_identical(tmp_path):
    from rsuper_amd import calculate_sensitivity_specificity as S
    gt = write_tables(str(tmp_path))
    out = str(tmp_path / 'out.csv')
    S.main(['--ground_truth_csv', gt, '--predictions_csv', str(tmp_path / 'tumor_detection_results_th0.5.csv'), '--output_csv', out])
    assert open(out, 'rb').read() == G['csv_sens_spec'].tobytes()
    assert 'N/A (0/0)' in text('csv_sens_spec')                                 # kidney has a single class


def test_f1_auc_csvs_are_byte_identical(tmp_path):
    from rsuper_amd import calculate_sensitivity_specificity_F1_AUC as F
    gt = write_tables(str(tmp_path))
    F.main(['--ground_truth_csv', gt, '--preds_dir', str(tmp_path)])
    for t in CONF:
        assert open(tmp_path / f'metrics_th{t}.csv', 'rb').read() == G[f'csv_metrics_th{t}'].tobytes(), t
    os.remove(tmp_path / 'tumor_detection_results_th0.3.csv')
    with pytest.raises(RuntimeError):
        F.evaluate_all(gt, str(tmp_path))


def test_auroc_matches_the_fixture_and_counts_ties_at_one_half(tmp_path):
    import pandas as pd
    from rsuper_amd import calculate_sensitivity_specificity_F1_AUC as F
    gt = write_tables(str(tmp_path))
    auc = F.prob_auc(F.load_ground_truth(gt), pd.read_csv(tmp_path / 'tumor_detection_results_th0.1.csv').drop_duplicates(subset='BDMAP_ID'))
    for organ, exp in META['auc'].items():
        assert (np.isnan(auc[organ]) if exp is None else auc[organ] == exp), organ
    assert sum(v is None for v in META['auc'].values()) == 1
    assert F.auroc([0, 0, 1, 1], [0.1, 0.4, 0.35, 0.8]) == 0.75
    assert F.auroc([0, 1], [0.5, 0.5]) == 0.5 and F.auroc([0, 1, 1], [0.5, 0.5, 0.9]) == 0.75
    assert np.isnan(F.auroc([1, 1], [0.2, 0.3]))


def test_split_ids_filter_and_columns(tmp_path):
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd import test_with_reports as T
    from rsuper_amd.inference.scoring import column_name, normalize_id
    for n in range(0, 12):
        for parts in (1, 2, 3, 5):
            got = [T.split_into_parts(list(range(n)), parts, k) for k in range(parts)]
            assert sum(got, []) == list(range(n))
            assert max(map(len, got)) - min(map(len, got)) <= 1
    assert T.split_into_parts(list(range(7)), 3, 0) == [0, 1, 2] and T.split_into_parts(list(range(7)), 3, 2) == [5, 6]
    with pytest.raises(ValueError):
        T.split_into_parts([1], 0, 0)
    with pytest.raises(ValueError):
        T.split_into_parts([1], 2, 2)
    assert normalize_id('BDMAP_00000001_0000.nii.gz') == 'BDMAP_00000001' == fr.normalize_id('BDMAP_00000001_0000.nii.gz')
    assert normalize_id('BDMAP_00000002') == 'BDMAP_00000002'
    names = {'liver_lesion': 'liver tumor volume predicted', 'pancreatic_lesion': 'pancreatic tumor volume predicted',
             'pancreas_pdac': 'pancreas pdac volume predicted', 'pancreas_pnet': 'pancreas pnet volume predicted',
             'pancreas_cyst': 'pancreas cyst volume predicted', 'liver': None, 'kidney_left': None}
    for cls, col in names.items():
        assert column_name(cls) == col == fr.column_name(cls)
    # the already-predicted filter on a temp tree: per-class files, a packed file, an incomplete case
    classes = ['liver', 'liver_lesion']
    save = tmp_path / 'save'
    os.makedirs(save / 'a' / 'predictions')
    for c in classes:
        np.savez(save / 'a' / 'predictions' / f'{c}.npz', np.zeros((2, 2, 2), np.uint8))
    os.makedirs(save / 'b')
    np.savez(save / 'b' / 'predictions.npz', arr_0=np.zeros((1, 2, 2, 2), np.uint8), classes=np.array(classes))
    os.makedirs(save / 'c' / 'predictions')
    np.savez(save / 'c' / 'predictions' / 'liver.npz', np.zeros((2, 2, 2), np.uint8))
    ids = ['a.npz', 'b.npy', 'c.npz', 'd.npz']
    assert P.filter_already_predicted(ids, str(save), classes, overwrite=False) == ['c.npz', 'd.npz']
    assert P.filter_already_predicted(ids, str(save), classes, overwrite=True) == ids
    assert P.filter_already_predicted(ids, str(save), classes, False, scored_ids={'d'}) == ['c.npz']
    assert P.case_id_of('x/ct.nii.gz') == 'x' and P.case_id_of('y.npy') == 'y'
    # the packed file reads back through the scorers' loader, lesion planes only
    planes = T.load_planes(str(save / 'b'), 'binary')
    assert list(planes) == ['liver_lesion'] and planes['liver_lesion'].shape == (2, 2, 2)
    # CSV layout: sorted columns, header once
    T.append_rows(str(save), {'BDMAP_ID': 'a', 'liver tumor volume predicted': 3}, None)
    T.append_rows(str(save), {'liver tumor volume predicted': 0, 'BDMAP_ID': 'b'}, None)
    assert open(save / 'tumor_detection_results.csv', 'rb').read() == b'BDMAP_ID,liver tumor volume predicted\r\na,3\r\nb,0\r\n'
    assert [os.path.basename(p) for p in T.csv_paths(str(save), 'auc')] == [f'tumor_detection_results_th{t}.csv' for t in CONF]
    sp = tmp_path / 'sp.csv'
    sp.write_text('BDMAP_ID,z,y,x\na,2.5,0.8,0.7\n')
    assert T.read_spacing_csv(str(sp)) == {'a': (2.5, 0.8, 0.7)} and T.read_spacing_csv(None) == {}


def test_parsers_and_refusals(tmp_path):
    from rsuper_amd import eval_AUC as E
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd import test_with_reports as T
    a = T.get_parser().parse_args(['--outputs_folder', 'x'])
    assert (a.th, a.parts, a.part, a.continuing, a.cases, a.spacing_csv, a.any_lesion) == (0.5, 1, 0, False, None, None, False)
    assert 'NOT SUPPORTED' in T.get_parser().format_help() and 'any_lesion' in T.get_parser('auc').format_help()
    os.makedirs(tmp_path / 'out' / 'case')
    for main in (T.main, E.main):
        with pytest.raises(SystemExit, match='any_lesion'):
            main(['--outputs_folder', str(tmp_path / 'out'), '--any_lesion'])
    cl = tmp_path / 'classes.yaml'
    cl.write_text('[liver_lesion, liver]\n')
    argv = ['--load', str(tmp_path / 'run1' / 'a.pth') + ',' + str(tmp_path / 'run2' / 'b.pth'), '--img_path', str(tmp_path / 'img'),
            '--class_list', str(cl), '--save_path', str(tmp_path / 'res'), '--dataset', 'abdomenatlas_ufo']
    args = P.get_parser(argv)
    assert len(args.load) == 2 and args.save_path == str(tmp_path / 'res' / 'abdomenatlas_ufo' / 'run1')
    assert args.sliding_window is True and args.window_size == args.training_size == [96, 96, 96] and args.base_chan == 32
    assert (args.th, args.parts, args.current_part, args.gpu, args.model, args.dimension) == (0.5, 1, 0, '0', 'unet', '3d')
    for flag in ('EMA', 'organ_mask_on_lesion', 'connected_components', 'predict_pancreas_only', 'save_probabilities', 'save_probabilities_lesions',
                 'not_save_binary', 'save_pancreas_lesion_only', 'overwrite', 'update_output_layer', 'packed', 'score'):
        assert getattr(args, flag) is False
    cfg = tmp_path / 'cfg.yaml'
    cfg.write_text('training_size: [32, 32, 32]\nbase_chan: 8\n')
    assert P.get_parser(argv + ['--config', str(cfg)]).window_size == [32, 32, 32]
    with pytest.raises(ValueError, match='configuration'):
        P.get_parser(argv + ['--model', 'nope'])
    os.makedirs(tmp_path / 'img')
    (tmp_path / 'img' / 'BDMAP_1.nii.gz').write_bytes(b'')
    with pytest.raises(ValueError, match='INTEGRATION section 3b'):
        P.main(argv)
    with pytest.raises(ValueError, match='INTEGRATION section 3b'):
        P.load_case(args, 'BDMAP_1/ct.nii.gz', ['liver'])


def test_symbol_declared_bound_exported_with_matching_arity():
    from rsuper_amd.hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    m = re.search(r'int rsuper_detection_binary\(([^)]*)\)', hdr)
    assert m, 'rsuper_detection_binary is not declared in include/rsuper_hip.h'
    assert 'rsuper_detection_binary' in lib.exported_symbols()
    res, argtypes = lib._SIGS['rsuper_detection_binary']
    assert res is ctypes.c_int and len(argtypes) == len(m.group(1).split(',')) == 14
    assert argtypes[9] is ctypes.c_double
    from rsuper_amd.hip import library
    assert 'detection_binary' in inspect.signature(library.install_postprocess_ops).parameters


def test_argument_validation_without_a_device():
    from rsuper_amd.hip import lib
    L = lib.lib()
    ERR_ARG = 1
    p = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before anything is launched

    def call(x=p, is_u8=1, planes=1, din=(4, 4, 4), dout=(4, 4, 4), th=0.5, counts=p, ws=p):
        return L.rsuper_detection_binary(x, is_u8, planes, *din, *dout, th, 1, counts, ws, None)

    assert call(x=None) == ERR_ARG and call(counts=None) == ERR_ARG and call(ws=None) == ERR_ARG
    assert call(planes=0) == ERR_ARG and call(planes=-3) == ERR_ARG and call(planes=65536) == ERR_ARG
    assert call(dout=(0, 4, 4)) == ERR_ARG and call(dout=(4, 4, 0)) == ERR_ARG and call(din=(4, 0, 4)) == ERR_ARG
    assert call(dout=(2048, 2048, 2048)) == ERR_ARG and call(th=float('nan')) == ERR_ARG
    assert L.rsuper_detection_workspace_bytes(3) == 3 * 257 * 8
