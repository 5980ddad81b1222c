"""CPU tests of the lesion table: the scipy / numpy restatement (tests/lesion_table_ref.py) on hand-made shapes with known answers, the C ABI surface
that needs no device (symbols, argument rules, workspace sizes), and the host side of rsuper_amd.inference.lesions (report rows through
estimate_tumor_volume, compare_with_report, the CSV text, the errors)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import lesion_table_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'rsuper_lesion_table_workspace_bytes': 5, 'rsuper_lesion_table_launches': 0, 'rsuper_lesion_table': 19, 'rsuper_label_overlap': 8}


def lin(shape, *zyx):
    return int(np.ravel_multi_index(zyx, shape))


def row(t, k=0):
    return dict(zip(('root', 'voxels', 'zmin', 'ymin', 'xmin', 'zmax', 'ymax', 'xmax', 'sz', 'sy', 'sx', 'p3', 'q3', 'pa', 'qa', 'flags'),
                    (int(v) for v in t['rows_i'][k]))), [float(v) for v in t['rows_f'][k]]


# ------------------------------------------------------------------------------------------------ the restatement on shapes with known answers
def test_box_5_6_7():
    shape = (8, 9, 10)
    m = np.zeros(shape, np.uint8)
    m[1:6, 2:8, 1:8] = 1                                                    # 5 x 6 x 7 voxels: centre-to-centre extents 4, 5, 6
    for conn in (6, 26):
        t = R.table(m, conn=conn)
        i, f = row(t)
        assert t['totals'].tolist() == [1, 0, 210, 1] and i['voxels'] == 210 and i['root'] == lin(shape, 1, 2, 1)
        assert (i['zmin'], i['ymin'], i['xmin'], i['zmax'], i['ymax'], i['xmax']) == (1, 2, 1, 5, 7, 7)
        assert (i['sz'], i['sy'], i['sx']) == (3 * 210, 4.5 * 210, 4 * 210)
        # four space diagonals tie; the smallest p is the first corner, its partner the last voxel
        assert f[0] == math.sqrt(77) and (i['p3'], i['q3']) == (lin(shape, 1, 2, 1), lin(shape, 5, 7, 7))
        # every slice attains sqrt(61) twice: the lowest slice, and of its two diagonals the one from the first corner
        assert f[1] == math.sqrt(61) and (i['pa'], i['qa']) == (lin(shape, 1, 2, 1), lin(shape, 1, 7, 7))
        assert abs(f[2] - 2 * 5 * 6 / math.sqrt(61)) < 1e-12 and f[3] == 4.0
        assert np.array_equal(t['labels'], m) and not t['rows_i'][1:].any() and not t['rows_f'][1:].any()
    t = R.table(m, spacing=(2.5, 0.7, 0.8))
    i, f = row(t)
    q = (2.5 * 2.5, 0.7 * 0.7, 0.8 * 0.8)
    assert f[0] == math.sqrt((q[0] * 16.0 + q[1] * 25.0) + q[2] * 36.0) and f[1] == math.sqrt(q[1] * 25.0 + q[2] * 36.0) and f[3] == 10.0
    assert abs(f[2] - 2 * (5 * 0.7) * (6 * 0.8) / f[1]) < 1e-12


def test_voxelised_ball():
    shape, c, r = (11, 12, 13), (5, 5, 6), 4
    t = R.table(R.ball(shape, c, r))
    i, f = row(t)
    # diameter 8 along the three axes only (16 = 4^2 + 0 + 0 has no other integer solution): the z pair has the smallest p
    assert f[0] == 8.0 and (i['p3'], i['q3']) == (lin(shape, 1, 5, 6), lin(shape, 9, 5, 6))
    # in-slice: only the centre slice reaches 8, along y before along x
    assert f[1] == 8.0 and (i['pa'], i['qa']) == (lin(shape, 5, 1, 6), lin(shape, 5, 9, 6)) and f[2] == 8.0 and f[3] == 8.0
    assert i['voxels'] == 257 and (i['sz'], i['sy'], i['sx']) == (5 * 257, 5 * 257, 6 * 257)


def test_plus_sign_and_one_voxel():
    shape = (3, 9, 9)
    m = np.zeros(shape, np.uint8)
    m[1, 4, 1:8] = 1
    m[1, 1:8, 4] = 1
    m[2, 8, 8] = 1                                                          # a second, one-voxel component
    t = R.table(m)
    i, f = row(t)
    assert t['totals'].tolist() == [2, 0, 14, 2] and i['voxels'] == 13
    assert f[:2] == [6.0, 6.0] and (i['p3'], i['q3']) == (i['pa'], i['qa']) == (lin(shape, 1, 1, 4), lin(shape, 1, 7, 4))      # the y arm comes first
    assert f[2] == 6.0 and f[3] == 0.0
    i, f = row(t, 1)
    one = lin(shape, 2, 8, 8)
    assert (i['root'], i['voxels'], i['p3'], i['q3'], i['pa'], i['qa']) == (one, 1, one, one, one, one) and f == [0.0, 0.0, 0.0, 0.0]
    assert t['labels'][2, 8, 8] == 2 and t['labels'][1, 4, 4] == 1
    t = R.table(m, min_voxels=2, max_lesions=1)
    assert t['totals'].tolist() == [1, 1, 14, 1] and t['labels'][2, 8, 8] == 255
    t = R.table(m, max_lesions=1)
    assert t['totals'].tolist() == [2, 0, 14, 1] and t['labels'][2, 8, 8] == 255


def test_l_shape_decided_by_the_tie_rule():
    """An L of two slices: tip to tip is attained four times in 3-D terms (same slice twice, across the slices twice); the across pairs are the longest and tie with
    each other, the in-slice pairs tie between the slices."""
    shape = (4, 7, 7)
    m = np.zeros(shape, np.uint8)
    m[1:3, 1:6, 1] = 1                                                      # arm along y, x = 1
    m[1:3, 5, 1:6] = 1                                                      # arm along x, y = 5
    t = R.table(m)
    i, f = row(t)
    assert f[0] == math.sqrt(1 + 16 + 16)
    assert (i['p3'], i['q3']) == (lin(shape, 1, 1, 1), lin(shape, 2, 5, 5))                 # not (1, 5, 5) - (2, 1, 1): its p is larger
    assert f[1] == math.sqrt(32) and (i['pa'], i['qa']) == (lin(shape, 1, 1, 1), lin(shape, 1, 5, 5))       # the lower slice
    assert abs(f[2] - 4 / math.sqrt(2)) < 1e-12 and f[3] == 1.0
    t6 = R.table(m, conn=6)
    assert np.array_equal(t6['rows_i'], t['rows_i']) and np.array_equal(t6['rows_f'], t['rows_f'])


def test_order_ties_and_the_issue_fixture():
    m = R.blobs((17, 20, 70))
    for conn, n, ties in ((6, 46, 16), (26, 38, 11)):                 # the issue's figures: components, rows that tie with the row before
        t = R.table(m, conn=conn, max_lesions=64)
        v, r = t['rows_i'][:n, 1], t['rows_i'][:n, 0]
        assert t['totals'].tolist() == [n, 0, int(m.sum()), n] and (v[:-1] >= v[1:]).all()
        same = v[:-1] == v[1:]
        assert (r[:-1][same] < r[1:][same]).all()
        assert int(same.sum()) == ties
    assert int(R.table(m, conn=26)['rows_i'][0, 1]) == 1413
    d = R.diagonal((20, 20, 70), 20)
    assert R.table(d, conn=26)['totals'].tolist() == [1, 0, 20, 1] and R.table(d, conn=6, max_lesions=8)['totals'].tolist() == [20, 0, 20, 8]
    a, b = np.array([0, 1, 2, 255, 3, 0]), np.array([0, 1, 1, 1, 255, 2])
    assert R.overlap(a, b, 2, 2).tolist() == [[0, 0, 1], [0, 1, 0], [0, 1, 0]]


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_symbols_are_declared_bound_and_exported_with_matching_arity():
    from rsuper_amd.hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, arity in NEW_SYMBOLS.items():
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/rsuper_hip.h'
        params = [p for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']
        assert len(params) == arity == len(lib._SIGS[name][1]), name
        assert hasattr(lib.lib(), name) and name in lib.exported_symbols()
    assert 'lesion_table.hip' in open(os.path.join(ROOT, 'r-super_amd', 'csrc', 'Makefile')).read()
    assert lib.lib().rsuper_lesion_table_launches() == 11


def expected_workspace(planes, D, H, W, rows):
    ps = (D * H * W + 63) // 64 * 64
    kd = (rows * D + 1) // 2 * 2
    return planes * (13 * ps + 64 + 3 * 1024 + 24 * kd + 1024 * rows)


def test_workspace_size_answers():
    from rsuper_amd.hip import lib
    L = lib.lib()
    for args in [(1, 4, 5, 6, 64), (3, 16, 16, 64, 4), (64, 1, 1, 1, 254), (1, 1, 1, 1, 1), (2, 9, 9, 33, 7), (1, 2048, 2048, 512, 64)]:
        assert L.rsuper_lesion_table_workspace_bytes(*args) == expected_workspace(*args), args
    for bad in [(0, 4, 4, 4, 8), (65, 4, 4, 4, 8), (1, 0, 4, 4, 8), (1, 4, -1, 4, 8), (1, 4, 4, 0, 8), (1, 2048, 2048, 513, 8), (1, 4, 4, 4, 0),
                (1, 4, 4, 4, 255)]:
        assert L.rsuper_lesion_table_workspace_bytes(*bad) == 0, bad


def test_argument_rules_without_a_device():
    """Everything here is refused before a launch: the pointers are stand-ins and are never dereferenced."""
    from rsuper_amd.hip import lib
    L = lib.lib()
    masks, ri, rf, tot, lab, ws = 4096, 8192, 16384, 32768, 65536, 131072
    need = L.rsuper_lesion_table_workspace_bytes(2, 4, 5, 6, 8)
    ok = (masks, 2, 4, 5, 6, 26, 1, 8, 65536, 1.0, 1.0, 1.0, ri, rf, tot, lab, ws, need)
    nan, inf = float('nan'), float('inf')
    bad = [(0, None), (12, None), (13, None), (14, None), (16, None),               # null pointers (labels, 15, may be null: no such case here)
           (1, 0), (1, 65), (2, 0), (3, -1), (4, 0),                                # planes, D, H, W
           (5, 0), (5, 18), (5, 8), (6, 0), (6, -3), (7, 0), (7, 255), (8, 1), (8, 0), (8, -5),
           (9, 0.0), (9, -1.0), (9, nan), (9, inf), (10, 0.0), (10, nan), (11, -inf), (11, inf), (11, nan),
           (12, ri + 4), (13, rf + 1), (14, tot + 2), (16, ws + 4),                 # misaligned outputs
           (17, need - 1), (17, 0), (17, -1)]
    for k, v in bad:
        assert L.rsuper_lesion_table(*(ok[:k] + (v,) + ok[k + 1:]), None) == 1, (k, v)
    assert L.rsuper_lesion_table(*(ok[:2] + (2048, 2048, 513) + ok[5:]), None) == 1                          # more than 2^31 voxels
    a, b, counts = 4096, 8192, 16384
    okl = (a, b, 2, 1000, 5, 3, counts)
    for k, v in [(0, None), (1, None), (6, None), (2, 0), (2, 65536), (3, 0), (3, -4), (4, -1), (4, 255), (5, -1), (5, 255), (6, counts + 4)]:
        assert L.rsuper_label_overlap(*(okl[:k] + (v,) + okl[k + 1:]), None) == 1, (k, v)


# ------------------------------------------------------------------------------------------------ the host side of inference/lesions.py
def fixed_table():
    """Two planes by hand: plane 0 holds a 12 x 8 x 5 mm lesion and a one-voxel lesion, plane 1 none."""
    from rsuper_amd.inference.lesions import LesionTable
    ri = np.zeros((2, 3, 16), np.int64)
    rf = np.zeros((2, 3, 4), np.float64)
    ri[0, 0] = [1234, 300, 2, 3, 4, 4, 12, 14, 900, 2100, 2700, 1300, 2500, 1400, 1490, 0]
    rf[0, 0] = [12.5, 12.0, 8.0, 5.0]
    ri[0, 1] = [77, 1, 0, 7, 7, 0, 7, 7, 0, 7, 7, 77, 77, 77, 77, 0]
    totals = np.array([[2, 5, 306, 2], [0, 0, 0, 0]], np.int64)
    return LesionTable.from_host(ri, rf, totals, (10, 20, 30), (2.5, 0.7, 0.9))


def test_report_rows_round_trip_through_estimate_tumor_volume():
    from rsuper_amd.inference.lesions import lesion_report_rows, padded_diameters
    from rsuper_amd.training.dataset.augmented import estimate_tumor_volume
    t = fixed_table()
    rows = lesion_report_rows(t, 'liver', location=['segment 4', 'u'])
    assert [set(r) for r in rows] == [{'Standardized Organ', 'Standardized Location', 'Tumor Size (mm)'}] * 2
    assert rows[0] == {'Standardized Organ': 'liver', 'Standardized Location': 'segment 4', 'Tumor Size (mm)': '12.8 x 8.8 x 7.5'}
    assert rows[1]['Tumor Size (mm)'] == '0.8 x 0.8 x 2.5' and rows[1]['Standardized Location'] == 'u'       # one voxel measures one voxel
    assert padded_diameters(t.rows(0)[0], t.spacing) == (12.0 + 0.8, 8.0 + 0.8, 5.0 + 2.5)
    assert lesion_report_rows(t, 'liver', pad=None)[0]['Tumor Size (mm)'] == '12.0 x 8.0 x 5.0'
    assert lesion_report_rows(t, 'liver', spacing=(1, 1, 1))[0]['Tumor Size (mm)'] == '13.0 x 9.0 x 6.0'
    assert lesion_report_rows(t, 'liver', plane=1) == []
    vols, diam = estimate_tumor_volume(rows, ['liver'])                                       # organ crop: both rows count
    assert diam[:2].tolist() == torch.tensor([[12.8, 8.8, 7.5], [0.8, 0.8, 2.5]]).tolist() and not diam[2:].any()
    assert vols[0] == (4 / 3) * math.pi * (6.4 * 4.4 * 3.75) and vols[2:] == [0] * 8
    vols, diam = estimate_tumor_volume(rows, ['segment 4'])                                   # segment crop: the located row only
    assert diam[0].tolist() == torch.tensor([12.8, 8.8, 7.5]).tolist() and not diam[1:].any()
    with pytest.raises(ValueError):
        lesion_report_rows(t, 'liver', location=['a'])
    with pytest.raises(ValueError):
        lesion_report_rows(t, 'liver', pad='mm')


def test_compare_with_report_on_a_fixed_table():
    from rsuper_amd.inference.lesions import compare_with_report
    t = fixed_table()
    report = [{'Standardized Organ': 'liver', 'Standardized Location': 'u', 'Tumor Size (mm)': '4'},
              {'Standardized Organ': 'liver', 'Standardized Location': 'liver segment 2', 'Tumor Size (mm)': '10 x 14'},
              {'Standardized Organ': 'kidney', 'Standardized Location': 'u', 'Tumor Size (mm)': '30 x 30 x 30'},
              {'Standardized Organ': 'liver', 'Standardized Location': 'liver segment 2', 'Tumor Size (mm)': '2 x 3 x 1'}]
    got = compare_with_report(t, report, 'liver')
    assert (got['n_pred'], got['n_report']) == (2, 3) and len(got['pairs']) == 2
    first, second = got['pairs']
    voxel = 2.5 * 0.7 * 0.9
    assert first['pred_diameter'] == 12.8 and first['report_diameter'] == 14.0 and abs(first['diameter_error'] - 1.2) < 1e-12
    assert first['pred_volume'] == 300 * voxel and first['report_volume'] == (4 / 3) * math.pi * (5 * 7 * 6)
    assert first['volume_error'] == abs(300 * voxel - (4 / 3) * math.pi * 210)
    assert second['pred_diameter'] == 2.5 and second['report_diameter'] == 4.0 and second['pred_volume'] == voxel
    assert second['report_volume'] == (4 / 3) * math.pi * 8
    none = compare_with_report(t, report, 'liver', plane=1)
    assert (none['n_pred'], none['n_report'], none['pairs']) == (0, 3, [])
    assert compare_with_report(t, report, 'kidney')['pairs'][0]['report_diameter'] == 30.0
    with pytest.raises(ValueError):
        compare_with_report(t, report, 'spleen')                                              # no organ word of estimate_tumor_volume


def test_csv_text_of_a_fixed_table(tmp_path):
    from rsuper_amd.inference.lesions import CSV_COLUMNS, append_csv, csv_text, lesion_csv_rows
    t = fixed_table()
    rows = lesion_csv_rows(t, 'BDMAP_00000001', 'liver_lesion', ['liver_segment_4', 'u'])
    text = csv_text(rows)
    assert text == ('BDMAP_ID,class,lesion,root,voxels,zmin,ymin,xmin,zmax,ymax,xmax,sum_z,sum_y,sum_x,p3,q3,pa,qa,flags,d3,a,b,c,location\n'
                    'BDMAP_00000001,liver_lesion,1,1234,300,2,3,4,4,12,14,900,2100,2700,1300,2500,1400,1490,0,12.5,12.0,8.0,5.0,liver_segment_4\n'
                    'BDMAP_00000001,liver_lesion,2,77,1,0,7,7,0,7,7,0,7,7,77,77,77,77,0,0.0,0.0,0.0,0.0,u\n')
    assert text.splitlines()[0].split(',') == list(CSV_COLUMNS)
    path = tmp_path / 'lesions.csv'
    append_csv(path, rows[:1])
    append_csv(path, lesion_csv_rows(t, 'BDMAP_00000002', 'liver_lesion', plane=1))           # no lesion: nothing but the file
    append_csv(path, rows[1:])
    assert path.read_text() == text
    t.host()[1][0, 0, 0] = float('nan')
    assert lesion_csv_rows(t, 'x', 'y')[0]['d3'] == 'nan' and lesion_csv_rows(t, 'x', 'y')[0]['location'] == ''


def test_python_errors_that_need_no_device():
    from rsuper_amd import inference
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.inference import lesions as LS
    for name in ('LesionTable', 'lesion_table', 'match_lesions', 'locate_lesions', 'lesion_report_rows', 'compare_with_report', 'lesion_csv_rows'):
        assert getattr(inference, name) is getattr(LS, name)
    assert str(torch.ops.rsuper.lesion_table.default._schema) == (
        'rsuper::lesion_table(Tensor masks, float[] spacing, int conn, int min_voxels, int max_lesions, int max_candidates, bool return_labels) '
        '-> (Tensor rows_i, Tensor rows_f, Tensor totals, Tensor labels)')
    assert str(torch.ops.rsuper.label_overlap.default._schema) == 'rsuper::label_overlap(Tensor labels_a, Tensor labels_b, int Ka, int Kb) -> Tensor'
    for op in ('lesion_table', 'label_overlap'):
        assert torch._C._dispatch_has_kernel_for_dispatch_key('rsuper::' + op, 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key('rsuper::' + op, 'CPU')
    with pytest.raises(RSuperHipError):
        LS.lesion_table(torch.zeros(2, 3, 4, dtype=torch.uint8))
    with pytest.raises(RSuperHipError):
        LS.lesion_table(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(NotImplementedError):
        torch.ops.rsuper.lesion_table(torch.zeros(1, 2, 3, 4, dtype=torch.uint8), [1.0, 1.0, 1.0], 26, 1, 8, 64, False)
    with pytest.raises(NotImplementedError):
        torch.ops.rsuper.label_overlap(torch.zeros(1, 8, dtype=torch.uint8), torch.zeros(1, 8, dtype=torch.uint8), 2, 2)
    LS._check_params((1, 1, 1), 26, 1, 64, 65536)
    LS._check_params((2.5, 0.7, 0.8), 6, 7, 254, 2)
    for bad in [((1, 1), 26, 1, 64, 8), ((1, 0, 1), 26, 1, 64, 8), ((1, float('nan'), 1), 26, 1, 64, 8), ((1, float('inf'), 1), 26, 1, 64, 8),
                ((1, 1, 1), 18, 1, 64, 8), ((1, 1, 1), 26, 0, 64, 8), ((1, 1, 1), 26, 1.5, 64, 8), ((1, 1, 1), 26, 1, 0, 8), ((1, 1, 1), 26, 1, 255, 8),
                ((1, 1, 1), 26, 1, 64, 1)]:
        with pytest.raises(ValueError):
            LS._check_params(*bad)
    t = fixed_table()
    assert (t.planes, t.max_lesions, t.count(0), t.count(1), t.single) == (2, 3, 2, 0, False)
    assert t.rows(0)[0]['voxels'] == 300 and t.rows(0)[0]['a'] == 12.0 and t.plane(0).single and t.plane(0).count() == 2
    with pytest.raises(ValueError, match='return_labels'):
        LS.match_lesions(t, t)
    with pytest.raises(ValueError, match='return_labels'):
        LS.locate_lesions(t, torch.zeros(1, 10, 20, 30), ['a'])
    assert LS.segment_classes('liver_lesion', ['liver', 'liver_lesion', 'liver_segment_1', 'liver_segment_2', 'pancreas_head']) == \
        ['liver_segment_1', 'liver_segment_2']
    assert LS.segment_classes('pancreatic_lesion', ['pancreas', 'pancreas_head', 'pancreas_tail', 'pancreatic_lesion']) == ['pancreas_head', 'pancreas_tail']
    assert LS.segment_classes('kidney_lesion', ['kidney_left', 'kidney_lesion', 'kidney_right', 'liver']) == ['kidney_left', 'kidney_right']


def test_measure_lesions_tool_lists_and_splits(tmp_path):
    from rsuper_amd.tools import measure_lesions as M
    for k in (3, 1, 2):
        (tmp_path / f'BDMAP_0000000{k}_gt.npy').write_bytes(b'')
        (tmp_path / f'BDMAP_0000000{k}.npy').write_bytes(b'')
    assert M.list_cases(tmp_path) == ['BDMAP_00000001', 'BDMAP_00000002', 'BDMAP_00000003']
    assert M.lesion_channels(['kidney_left', 'kidney_lesion', 'liver', 'liver_lesion']) == [1, 3]
    a = M.get_parser().parse_args(['--data_root', str(tmp_path), '--out', str(tmp_path / 'r.csv'), '--parts', '2', '--current_part', '1'])
    assert (a.parts, a.current_part, a.min_voxels, a.max_lesions, a.conn, a.pad) == (2, 1, 1, 64, 26, 'voxel')
    M.append_rows(tmp_path / 'out' / 'r.csv', [{'BDMAP ID': 'x', 'Standardized Organ': 'liver', 'Standardized Location': 'u', 'Tumor Size (mm)': '1.0 x 1.0 x 1.0'}])
    M.append_rows(tmp_path / 'out' / 'r.csv', [])
    assert (tmp_path / 'out' / 'r.csv').read_text() == 'BDMAP ID,Standardized Organ,Standardized Location,Tumor Size (mm)\nx,liver,u,1.0 x 1.0 x 1.0\n'
