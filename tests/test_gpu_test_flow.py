"""MI355X tests of the test flow: rsuper_detection_binary (csrc/postproc.hip) against the reference's own numbers (tests/golden/test_flow.npz,
written by test_with_reports.detection) and the numpy restatement tests/test_flow_ref.py, then predict_abdomenatlas / test_with_reports / eval_AUC
end to end on three synthetic cases.  Counts and CSV rows compare exactly."""
import csv
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
import postprocess_ref as R  # noqa: E402
import resample_ref as rr  # noqa: E402
import synth  # noqa: E402
import test_flow_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'test_flow.npz'))
META = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'test_flow.json')))
CLASSES = ['kidney_left', 'kidney_lesion', 'kidney_right', 'liver', 'liver_lesion', 'pancreas', 'pancreatic_lesion']
LESIONS = [c for c in CLASSES if c.endswith('_lesion')]
SPACING = {'BDMAP_00000001': (1.0, 1.0, 1.0), 'BDMAP_00000002': (1.5, 0.8, 1.25), 'BDMAP_00000003': (0.7, 1.0, 2.5)}
SHAPES = {'BDMAP_00000001': (40, 36, 44), 'BDMAP_00000002': (38, 36, 42), 'BDMAP_00000003': (40, 34, 44)}


def det_volume(case):
    if f'det_{case["name"]}_x' in G.files:
        return G[f'det_{case["name"]}_x']
    n = int(np.prod(case['shape']))
    return np.unpackbits(G[f'det_{case["name"]}_bits'])[:n].reshape(case['shape'])


@pytest.mark.parametrize('case', META['det'], ids=[c['name'] for c in META['det']])
def test_kernel_matches_the_reference_fixture(case):
    """Every fixture case (the four shapes of the issue's list among them: identity over 2 x 2 x 2 tiles, (6, 11, 16) -> (9, 16, 80) with the
    half-to-even side, the beyond-the-input x plane and three x tiles, (20, 40, 70) -> (10, 20, 35), and the single output plane), erode as
    recorded and off, from a numpy array and from a device tensor."""
    from rsuper_amd.inference import detection_binary
    v, sp, th = det_volume(case), case['spacing'], case['th']
    got = detection_binary(v, spacing=sp, th=th, erode=case['erode'])
    print(case['name'], got, case['expected'])
    assert type(got) is int and got == case['expected'] == fr.detection_binary(v, sp, th, case['erode'])
    assert detection_binary(torch.from_numpy(v).to(DEV), spacing=sp, th=th, erode=False) == case['plain']
    if case['quirk_axes']:
        assert got != case['clamped']


def test_planes_and_dtypes_in_one_launch():
    """P = 3 planes (one empty, one full, one busy) in one launch, erode on and off, uint8 / bool / float32, numpy / host tensor / device tensor;
    the float32 plane holds values exactly equal to th, which do not count."""
    from rsuper_amd.inference import detection_binary
    r = np.random.default_rng(11)
    shape, sp, th = (10, 20, 40), (1.3, 0.9, 1.1), 0.25
    busy = np.zeros(shape, bool)
    busy[2:8, 3:15, 5:30] = True
    busy ^= r.random(shape) < 0.05
    m = np.stack([np.zeros(shape, bool), np.ones(shape, bool), busy])
    f = np.where(m, np.float32(0.5), np.float32(0.0)).astype(np.float32)
    at_th = r.random(m.shape) < 0.1
    f[at_th] = np.float32(th)                                                   # set or not before: now exactly th -> not set
    assert at_th[2].any() and (m & at_th).any()
    for erode in (True, False):
        exp_m = [fr.detection_binary(m[p], sp, 0.5, erode) for p in range(3)]
        exp_f = [fr.detection_binary(f[p], sp, th, erode) for p in range(3)]
        assert exp_m[0] == 0 and exp_m[1] > 0 and 0 < exp_m[2] < exp_m[1] and exp_f[2] != exp_m[2]
        assert detection_binary(m.astype(np.uint8), sp, 0.5, erode) == exp_m
        assert detection_binary(m, sp, 0.5, erode) == exp_m                                                   # bool numpy
        assert detection_binary(torch.from_numpy(m), sp, 0.5, erode) == exp_m                                 # bool host tensor
        assert detection_binary(torch.from_numpy(m.astype(np.uint8)).to(DEV), sp, 0.5, erode) == exp_m
        assert detection_binary(f, sp, th, erode) == exp_f
        assert detection_binary(torch.from_numpy(f).to(DEV), sp, th, erode) == exp_f
        assert [detection_binary(f[p], sp, th, erode) for p in range(3)] == exp_f
        assert detection_binary((m * 2).astype(np.uint8), sp, 2.0, erode) == [0, 0, 0]                        # 2 > 2 is false
    counts = torch.ops.rsuper.detection_binary(torch.from_numpy(m.astype(np.uint8)).to(DEV), list(fr.zoom_shape(shape, sp)), 0.5, True, None)
    assert counts.is_cuda and counts.dtype == torch.int64 and counts.tolist() == [fr.detection_binary(m[p], sp, 0.5, True) for p in range(3)]
    with pytest.raises(TypeError):
        detection_binary(m.astype(np.int32), sp)
    with pytest.raises(ValueError):
        detection_binary(m[0], (0.01, 1, 1))


def test_order_1_detection_is_unchanged():
    from rsuper_amd.inference import detection
    P = np.load(os.path.join(ROOT, 'tests', 'golden', 'postprocess.npz'))
    for erode in (True, False):
        vols, mx = detection(P['det_down_big_x'], spacing=tuple(float(v) for v in P['det_down_big_spacing']), erode=erode)
        assert [vols[t] for t in R.THRESHOLDS] == [int(v) for v in P['det_down_big_vol_' + ('erode' if erode else 'plain')]]
        assert abs(mx - float(P['det_down_big_max'])) <= 1e-12 * float(P['det_down_big_max'])


# ------------------------------------------------------------------------------------------------ end to end
def read_rows(path):
    with open(path, newline='') as f:
        return list(csv.DictReader(f))


def base_argv(d, save):
    return ['--load', os.path.join(d, 'run7', 'latest.pth'), '--img_path', os.path.join(d, 'img'), '--class_list', os.path.join(d, 'classes.yaml'),
            '--config', os.path.join(d, 'unet8.yaml'), '--save_path', os.path.join(d, save), '--dataset', 'synthetic',
            '--spacing_csv', os.path.join(d, 'spacing.csv'), '--organ_mask_on_lesion']


@pytest.fixture(scope='module')
def flow(tmp_path_factory):
    """The tree of one scored run and what direct predict_case calls return for the same cases (computed once, read by every test below)."""
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd.inference import postprocess_npz, predict_case
    from rsuper_amd.model.dim3.unet import UNet
    d = str(tmp_path_factory.mktemp('test_flow'))
    os.makedirs(os.path.join(d, 'img'))
    os.makedirs(os.path.join(d, 'run7'))
    with open(os.path.join(d, 'classes.yaml'), 'w') as f:
        f.write('[' + ', '.join(reversed(CLASSES)) + ']\n')                     # unsorted on disk: the command sorts
    with open(os.path.join(d, 'unet8.yaml'), 'w') as f:
        f.write('in_chan: 1\nbase_chan: 8\ndown_scale: [[2,2,2], [2,2,2], [2,2,2], [2,2,2]]\nkernel_size: [[3,3,3], [3,3,3], [3,3,3], [3,3,3], [3,3,3]]\n'
                'block: BasicBlock\nnorm: in\ncompute_dtype: f32\ntraining_size: [32, 32, 32]\n')
    with open(os.path.join(d, 'spacing.csv'), 'w') as f:
        f.write('BDMAP_ID,z,y,x\n' + ''.join(f'{k},{v[0]},{v[1]},{v[2]}\n' for k, v in SPACING.items()))
    net = UNet(1, 8, num_classes=len(CLASSES), block='BasicBlock', norm='in', compute_dtype='f32')
    sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 7)
    ema = synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 8)
    torch.save({'epoch': 1, 'model_state_dict': {k: torch.from_numpy(v) for k, v in sd.items()},
                'ema_model_state_dict': {k: torch.from_numpy(v) for k, v in ema.items()}}, os.path.join(d, 'run7', 'latest.pth'))
    hus = {}
    for k, (case, shape) in enumerate(SHAPES.items()):
        hus[case] = rr.ct_volume(shape, -200.0, 400.0, 40 + k, np.int16)
        if k == 1:
            np.save(os.path.join(d, 'img', case + '.npy'), hus[case])           # the packed dataset's image form
        else:
            np.savez(os.path.join(d, 'img', case + '.npz'), hus[case])
    argv = base_argv(d, 'res') + ['--save_probabilities_lesions', '--score']
    done, times = P.main(argv)
    args = P.get_parser(argv)
    args.class_list, args.classes = CLASSES, len(CLASSES)
    models = P.init_model(args, CLASSES)
    direct = {}
    for case, hu in hus.items():
        pred, raw = predict_case(models, hu, args, CLASSES)
        rawd = postprocess_npz(raw, CLASSES, args)
        direct[case] = ({c: pred[c].cpu().numpy() for c in CLASSES}, {c: rawd[c].cpu().numpy() for c in LESIONS})
    return {'dir': d, 'save': args.save_path, 'done': done, 'times': times, 'direct': direct}


def test_saved_planes_equal_direct_predict_case(flow):
    assert flow['save'] == os.path.join(flow['dir'], 'res', 'synthetic', 'run7')
    assert flow['done'] == sorted(SHAPES) and set(flow['times']) == {'read', 'predict', 'postprocess', 'measure', 'write'}
    some = 0
    for case, (pred, raw) in flow['direct'].items():
        for c in CLASSES:
            with np.load(os.path.join(flow['save'], case, 'predictions', c + '.npz')) as z:
                assert z['arr_0'].dtype == np.uint8 and z['arr_0'].shape == SHAPES[case] and np.array_equal(z['arr_0'], pred[c])
            some += int(pred[c].sum())
        assert sorted(os.listdir(os.path.join(flow['save'], case, 'predictions_raw'))) == sorted(c + '.npz' for c in LESIONS)
        for c in LESIONS:
            with np.load(os.path.join(flow['save'], case, 'predictions_raw', c + '.npz')) as z:
                assert z['arr_0'].dtype == np.float32 and np.array_equal(z['arr_0'], raw[c])
    assert some > 0


def test_score_rows_equal_the_numpy_reference_for_both_flows(flow):
    from rsuper_amd.inference import detection
    rows = read_rows(os.path.join(flow['save'], 'tumor_detection_results.csv'))
    assert [r['BDMAP_ID'] for r in rows] == sorted(SHAPES)
    cols = sorted(['BDMAP_ID'] + [fr.column_name(c) for c in LESIONS])
    assert list(rows[0]) == cols and 'pancreatic tumor volume predicted' in cols and 'kidney tumor volume predicted' in cols
    for r in rows:
        pred, _ = flow['direct'][r['BDMAP_ID']]
        exp = fr.row(r['BDMAP_ID'], {c: pred[c] for c in LESIONS}, SPACING[r['BDMAP_ID']], 0.5)
        print(r, exp)
        assert r == {k: str(v) for k, v in exp.items()}
    for t in R.THRESHOLDS:
        rows_t = read_rows(os.path.join(flow['save'], f'tumor_detection_results_th{t}.csv'))
        assert [r['BDMAP_ID'] for r in rows_t] == sorted(SHAPES)
        assert list(rows_t[0]) == sorted(cols + [fr.column_name(c).replace('volume predicted', 'maximum probability') for c in LESIONS])
        for r in rows_t:
            _, raw = flow['direct'][r['BDMAP_ID']]
            for c in LESIONS:
                vols, mx = R.detection(raw[c], SPACING[r['BDMAP_ID']], R.THRESHOLDS)
                col = fr.column_name(c)
                assert r[col] == str(vols[t])
                got = float(r[col.replace('volume predicted', 'maximum probability')])
                assert got == detection(raw[c], SPACING[r['BDMAP_ID']])[1] and abs(got - mx) <= 1e-12 * abs(mx)


def test_second_run_without_overwrite_predicts_nothing(flow):
    from rsuper_amd import predict_abdomenatlas as P
    before = open(os.path.join(flow['save'], 'tumor_detection_results.csv'), 'rb').read()
    done, _ = P.main(base_argv(flow['dir'], 'res') + ['--save_probabilities_lesions', '--score'])
    assert done == [] and open(os.path.join(flow['save'], 'tumor_detection_results.csv'), 'rb').read() == before


def test_packed_output_unpacks_to_the_same_planes_and_parts_cover_each_case_once(flow):
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd import test_with_reports as T
    d = flow['dir']
    got = [P.main(base_argv(d, 'packed') + ['--packed', '--parts', '2', '--current_part', str(k)])[0] for k in range(2)]
    assert sorted(got[0] + got[1]) == sorted(SHAPES) and not set(got[0]) & set(got[1]) and got[0] and got[1]
    save = os.path.join(d, 'packed', 'synthetic', 'run7')
    for case, (pred, _) in flow['direct'].items():
        assert os.listdir(os.path.join(save, case)) == ['predictions.npz']
        with np.load(os.path.join(save, case, 'predictions.npz')) as z:
            assert [str(c) for c in z['classes']] == CLASSES and z['arr_0'].shape == (1,) + SHAPES[case]
            bits = np.unpackbits(z['arr_0'], axis=0)[:len(CLASSES)]
        assert np.array_equal(bits, np.stack([pred[c] for c in CLASSES]))
    # the scorer reads the packed tree too
    rows = T.main(['--outputs_folder', save, '--spacing_csv', os.path.join(d, 'spacing.csv')])
    assert [{k: str(v) for k, v in r.items()} for r in rows] == read_rows(os.path.join(flow['save'], 'tumor_detection_results.csv'))
    part = T.main(['--outputs_folder', save, '--spacing_csv', os.path.join(d, 'spacing.csv'), '--parts', '2', '--part', '1'])
    assert [r['BDMAP_ID'] for r in part] == sorted(SHAPES)[2:]


def test_scorers_over_the_saved_tree_reproduce_the_score_rows(flow):
    from rsuper_amd import eval_AUC as E
    from rsuper_amd import test_with_reports as T
    names = ['tumor_detection_results.csv'] + [f'tumor_detection_results_th{t}.csv' for t in R.THRESHOLDS]
    before = {n: open(os.path.join(flow['save'], n), 'rb').read() for n in names}
    sp = ['--spacing_csv', os.path.join(flow['dir'], 'spacing.csv')]
    assert len(T.main(['--outputs_folder', flow['save']] + sp)) == 3 and len(E.main(['--outputs_folder', flow['save']] + sp)) == 3
    assert {n: open(os.path.join(flow['save'], n), 'rb').read() for n in names} == before
    assert T.main(['--outputs_folder', flow['save'], '--continuing'] + sp) == []          # --continuing skips what the CSV holds


def test_ensemble_ema_pancreas_only_and_the_saving_flags(flow):
    """--load A,A --EMA --ids --predict_pancreas_only (bit-packed <id>_gt.npz) --connected_components --save_pancreas_lesion_only --save_probabilities
    against the same steps made by hand."""
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd.inference import postprocess_npz, prediction, preprocess_array
    d, case = flow['dir'], 'BDMAP_00000001'
    lab = np.zeros((len(CLASSES),) + SHAPES[case], np.uint8)
    lab[CLASSES.index('pancreas'), 0:4, 0:3, 0:6] = 1                            # a corner: only the first 32^3 window touches it
    np.savez(os.path.join(d, 'img', case + '_gt.npz'), np.packbits(lab, axis=0))
    with open(os.path.join(d, 'ids.csv'), 'w') as f:
        f.write('BDMAP ID\n' + case + '\n')
    ck = os.path.join(d, 'run7', 'latest.pth')
    argv = base_argv(d, 'panc') + ['--ids', os.path.join(d, 'ids.csv'), '--EMA', '--predict_pancreas_only', '--connected_components',
                                   '--save_pancreas_lesion_only', '--save_probabilities']
    argv[argv.index('--load') + 1] = ck + ',' + ck
    done, _ = P.main(argv)
    assert done == [case]
    os.remove(os.path.join(d, 'img', case + '_gt.npz'))                         # the image folder is shared: leave it as it was
    args = P.get_parser(argv)
    args.class_list, args.classes = CLASSES, len(CLASSES)
    models = P.init_model(args, CLASSES)
    ema = torch.load(ck, weights_only=False)['ema_model_state_dict']
    k0 = sorted(ema)[0]
    assert len(models) == 2 and torch.equal(models[1].state_dict()[k0].cpu(), ema[k0])
    with np.load(os.path.join(d, 'img', case + '.npz')) as z:
        img, _ = preprocess_array(z['arr_0'], args)
    pancreas = torch.from_numpy(lab[CLASSES.index('pancreas')].astype(np.float32)).to(DEV)
    label, raw = prediction(models, img, args, tgt_organ=pancreas, to_cpu=False)
    pred, rawd = postprocess_npz(label, CLASSES, args), postprocess_npz(raw, CLASSES, args)
    save = os.path.join(d, 'panc', 'synthetic', 'run7', case)
    kept = ['pancreas', 'pancreatic_lesion']
    for sub, ref, dt in (('predictions', pred, np.uint8), ('predictions_raw', rawd, None)):
        assert sorted(os.listdir(os.path.join(save, sub))) == sorted(c + '.npz' for c in kept)
        for c in kept:
            with np.load(os.path.join(save, sub, c + '.npz')) as z:
                assert np.array_equal(z['arr_0'], ref[c].cpu().numpy()) and (dt is None or z['arr_0'].dtype == dt)
    assert raw[:, 32:].abs().sum().item() == 0 and raw[:, :, 32:].abs().sum().item() == 0 and raw[..., 32:].abs().sum().item() == 0
    assert raw[:, :32, :32, :32].min().item() > 0                               # the other seven windows were skipped
    assert not np.array_equal(pred['pancreas'].cpu().numpy(), flow['direct'][case][0]['pancreas'])
