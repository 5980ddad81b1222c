"""MI355X tests of the lesion table (csrc/lesion_table.hip, rsuper_amd.inference.lesions) against the scipy / numpy restatement
tests/lesion_table_ref.py, which searches all voxels of a component by brute force.  Every comparison is exact -- integers, canonical pairs, labels,
d3, a and c as float64 -- except b, which is held to 1e-9 relative (a float64 expression whose rounding order is not fixed).  Shapes are chosen
against the 8 x 8 x 32 labelling tile."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import lesion_table_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ISO, ANISO = (1.0, 1.0, 1.0), (2.5, 0.7, 0.8)


def symmetric_planes():
    """Box, ball, plus sign and the two-slice L across the tile borders at z = 8, y = 8 and x = 32: pair ties everywhere at spacing 1."""
    shape = (13, 14, 40)
    box, plus, ell = (np.zeros(shape, np.uint8) for _ in range(3))
    box[5:10, 4:10, 29:36] = 1
    plus[7, 8, 29:36] = 1
    plus[7, 5:12, 32] = 1
    plus[12, 13, 39] = 1
    ell[7:9, 5:10, 30] = 1
    ell[7:9, 9, 30:35] = 1
    return np.stack([box, R.ball(shape, (6, 7, 32), 4), plus, ell])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(P, D, H, W) uint8 stacks, made once."""
    if name == 'one_set':
        return np.ones((1, 1, 1, 1), np.uint8)
    if name == 'one_unset':
        return np.zeros((1, 1, 1, 1), np.uint8)
    if name == 'small':                                                    # one voxel past the tile on every axis
        return R.blobs((9, 9, 33), seed=1, quantile=0.7)[None]
    if name == 'blobs':                                                    # 46 components at 6-connectivity, 38 at 26, 16 and 11 equal-size ties
        return R.blobs((17, 20, 70))[None]
    if name == 'three':                                                    # three densities in one call
        return np.stack([R.blobs((17, 20, 70)), R.salt((17, 20, 70), 3), R.ball((17, 20, 70), (8, 9, 33), 6)])
    if name == 'diagonal':
        return R.diagonal((20, 20, 70), 20)[None]
    if name == 'symmetric':
        return symmetric_planes()
    if name == 'salt':
        return R.salt((16, 16, 64), 5)[None]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref(name, conn, spacing, min_voxels=1, max_lesions=64):
    return R.tables(inputs(name), spacing=spacing, conn=conn, min_voxels=min_voxels, max_lesions=max_lesions)


def compare(ri, rf, totals, labels, want, what, capped=False):
    """Host arrays against the restatement; capped: rows may carry the skipped-search form of d3 / p3 / q3 / flags instead."""
    ri, rf = ri.copy(), rf.copy()
    assert np.array_equal(totals, want['totals']), (what, totals, want['totals'])
    if capped:
        cut = ri[..., 15] == 1
        assert np.isnan(rf[cut][:, 0]).all() and (ri[cut][:, 11:13] == -1).all()
        ri[cut, 11:13], ri[cut, 15], rf[cut, 0] = want['rows_i'][cut][:, 11:13], 0, want['rows_f'][cut][:, 0]
    bad = np.argwhere(ri != want['rows_i'])
    assert bad.size == 0, (what, bad[:5], ri[tuple(bad[0][:2])], want['rows_i'][tuple(bad[0][:2])])
    for j, f in ((0, 'd3'), (1, 'a'), (3, 'c')):
        assert np.array_equal(rf[..., j], want['rows_f'][..., j]), (what, f, rf[..., j], want['rows_f'][..., j])
    b, wb = rf[..., 2], want['rows_f'][..., 2]
    err = float(np.max(np.abs(b - wb) / np.where(wb != 0, np.abs(wb), 1.0))) if b.size else 0.0
    print(f'{what}: rows {int(totals[..., 3].sum())}, max relative error of b {err:.3e}')
    assert (np.abs(b - wb) <= 1e-9 * np.abs(wb)).all(), (what, err)
    if labels is not None:
        assert np.array_equal(labels, want['labels']), what


def run(name, conn=26, spacing=ISO, min_voxels=1, max_lesions=64, max_candidates=65536, labels=True):
    from rsuper_amd.inference import lesion_table
    t = lesion_table(torch.from_numpy(inputs(name)).to(DEV), spacing=spacing, conn=conn, min_voxels=min_voxels, max_lesions=max_lesions,
                     max_candidates=max_candidates, return_labels=labels)
    ri, rf, to = t.host()
    return t, ri, rf, to, (t.labels.cpu().numpy() if labels else None)


@pytest.mark.parametrize('spacing', [ISO, ANISO], ids=['iso', 'aniso'])
@pytest.mark.parametrize('conn', [6, 26])
@pytest.mark.parametrize('name', ['one_set', 'one_unset', 'small', 'blobs', 'three', 'diagonal', 'symmetric'])
def test_table_equals_the_restatement(name, conn, spacing):
    _, ri, rf, to, lab = run(name, conn, spacing)
    compare(ri, rf, to, lab, ref(name, conn, spacing), f'{name} conn {conn} {spacing}')
    if name == 'blobs':
        assert int(to[0, 0]) == {6: 46, 26: 38}[conn]
    if name == 'diagonal':
        assert to[0].tolist() == ([20, 0, 20, 20] if conn == 6 else [1, 0, 20, 1])
    if name == 'one_set':
        assert ri[0, 0].tolist() == [0, 1] + [0] * 14 and rf[0, 0].tolist() == [0.0] * 4 and to[0].tolist() == [1, 0, 1, 1]
    if name == 'one_unset':
        assert to[0].tolist() == [0, 0, 0, 0] and not ri.any() and not rf.any() and not lab.any()


def test_single_plane_bool_and_no_labels():
    from rsuper_amd.inference import lesion_table
    m = torch.from_numpy(inputs('blobs')[0]).to(DEV)
    want = ref('blobs', 26, ISO)
    for x in (m, m.bool(), m * 7):
        t = lesion_table(x)
        assert t.single and t.labels is None and t.count() == 38 and len(t.rows()) == 38
        ri, rf, to = t.host()
        compare(ri, rf, to, None, want, 'single plane')
    assert t.rows()[0]['voxels'] == 1413 and t.rows()[0]['flags'] == 0


@pytest.mark.parametrize('conn', [6, 26])
@pytest.mark.parametrize('min_voxels', [1, 2])
def test_more_components_than_rows(conn, min_voxels):
    _, ri, rf, to, lab = run('salt', conn, ISO, min_voxels=min_voxels, max_lesions=4)
    want = ref('salt', conn, ISO, min_voxels, 4)
    compare(ri, rf, to, lab, want, f'salt conn {conn} min_voxels {min_voxels}')
    kept, dropped, fg, rows = (int(v) for v in to[0])
    assert rows == 4 and kept > 4 and fg == int(inputs('salt').sum()) and (dropped > 0) == (min_voxels == 2)
    assert int((lab == 255).sum()) == fg - int(ri[0, :, 1].sum()) > 0 and sorted(np.unique(lab)) == [0, 1, 2, 3, 4, 255]


def test_candidate_cap_flags_d3_and_leaves_the_rest_exact():
    _, ri, rf, to, lab = run('blobs', 26, ANISO, max_candidates=8)
    compare(ri, rf, to, lab, ref('blobs', 26, ANISO), 'max_candidates 8', capped=True)
    flags = ri[0, :38, 15]
    assert flags[0] == 1 and np.isnan(rf[0, 0, 0]) and ri[0, 0, 11:13].tolist() == [-1, -1]        # the 1413-voxel blob
    assert set(flags.tolist()) == {0, 1} and not np.isnan(rf[0, :38, 1:]).any()


def abi(masks, conn, min_voxels, K, max_candidates, sp, rows_i, rows_f, totals, labels, ws):
    from rsuper_amd.hip import lib
    P, D, H, W = masks.shape
    rc = lib.lib().rsuper_lesion_table(masks.data_ptr(), P, D, H, W, conn, min_voxels, K, max_candidates, sp[0], sp[1], sp[2], rows_i.data_ptr(),
                                       rows_f.data_ptr(), totals.data_ptr(), None if labels is None else labels.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()


def test_dirty_buffers_repeat_calls_and_odd_offsets():
    """Workspace and outputs filled with 0xFF bytes, then with NaN words: the same table.  The same call twice on the same buffers: the same bytes.
    Outputs at odd multiples of their element size inside a 0xAA buffer: the bytes around them stay 0xAA."""
    from rsuper_amd.hip import lib
    masks = torch.from_numpy(inputs('three')).to(DEV)
    P, D, H, W = masks.shape
    K, sp = 9, ANISO
    want = R.tables(inputs('three'), spacing=sp, conn=26, min_voxels=2, max_lesions=K)
    nws = lib.lib().rsuper_lesion_table_workspace_bytes(P, D, H, W, K)
    sizes = [P * K * 16 * 8, P * K * 4 * 8, P * 4 * 8, P * D * H * W]
    offs, o = [], 24                                                        # rows_i, rows_f, totals at odd multiples of 8, the labels at an odd byte
    for j, n in enumerate(sizes):
        offs.append(o + (1 if j == 3 else 0))
        o = (offs[-1] + n + 16 + 15) // 16 * 16 + 8
    assert [v % 16 for v in offs] == [8, 8, 8, 9]
    results = []
    for fill in (0xFF, 'nan', 'repeat'):
        if fill != 'repeat':
            ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
            buf = torch.full((o + 64,), 0xAA, device=DEV, dtype=torch.uint8)
            if fill == 'nan':
                ws.view(torch.float64).fill_(float('nan'))
                for off, s in zip(offs[:3], sizes[:3]):
                    buf[off:off + s].view(torch.float64).fill_(float('nan'))
            else:
                ws.fill_(0xFF)
                for off, s in zip(offs, sizes):
                    buf[off:off + s] = 0xFF
        views = [buf[off:off + s] for off, s in zip(offs, sizes)]
        abi(masks, 26, 2, K, 65536, sp, views[0], views[1], views[2], views[3], ws)
        host = buf.cpu().numpy()
        outside = np.ones(host.size, bool)
        for off, s in zip(offs, sizes):
            outside[off:off + s] = False
        assert (host[outside] == 0xAA).all(), fill
        got = [host[off:off + s].copy() for off, s in zip(offs, sizes)]
        compare(got[0].view(np.int64).reshape(P, K, 16), got[1].view(np.float64).reshape(P, K, 4), got[2].view(np.int64).reshape(P, 4),
                got[3].reshape(P, D, H, W), want, f'fill {fill}')
        results.append(b''.join(g.tobytes() for g in got))
    assert results[0] == results[1] == results[2]


def test_label_overlap_equals_add_at():
    r = np.random.default_rng(9)
    shape = (2, 5, 7, 37)                                                   # 1295 voxels per plane: no multiple of the block
    a = r.choice(np.array([0, 0, 0, 1, 2, 3, 4, 5, 6, 255], np.uint8), shape)
    b = r.choice(np.array([0, 0, 1, 2, 3, 4, 255], np.uint8), shape)
    a[:, :2] = 0
    a[:, 2, :3] = 3                                                         # long runs of one pair
    b[:, 2, :3] = 2
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for Ka, Kb in ((5, 3), (6, 4), (2, 7), (0, 4)):
        out = torch.full((2 * (Ka + 1) * (Kb + 1) + 2,), -7, device=DEV, dtype=torch.int64)
        from rsuper_amd.hip import lib
        assert lib.lib().rsuper_label_overlap(ta.data_ptr(), tb.data_ptr(), 2, a[0].size, Ka, Kb, out[1:].data_ptr(),
                                              torch.cuda.current_stream().cuda_stream) == 0
        got = out.cpu().numpy()
        assert got[0] == -7 and got[-1] == -7
        want = np.stack([R.overlap(a[p], b[p], Ka, Kb) for p in range(2)])
        assert np.array_equal(got[1:-1].reshape(want.shape), want), (Ka, Kb)
        assert np.array_equal(torch.ops.rsuper.label_overlap(ta, tb, Ka, Kb).cpu().numpy(), want)
        assert want[:, 0, 0].tolist() == [0, 0] and want.sum() > 0


def test_match_and_locate_end_to_end():
    from scipy import ndimage
    from rsuper_amd.inference import lesion_table, locate_lesions, match_lesions
    gt = inputs('blobs')[0]
    pred = np.roll(ndimage.binary_dilation(gt, iterations=1).astype(np.uint8), 2, axis=2)
    pred[:, :, :2] = 0
    pred[0:3, 0:3, 60:63] = 1 - gt[0:3, 0:3, 60:63]
    tp = lesion_table(torch.from_numpy(pred).to(DEV), conn=26, min_voxels=3, max_lesions=20, return_labels=True)
    tg = lesion_table(torch.from_numpy(gt).to(DEV), conn=26, min_voxels=3, max_lesions=30, return_labels=True)
    rp, rg = R.table(pred, conn=26, min_voxels=3, max_lesions=20), R.table(gt, conn=26, min_voxels=3, max_lesions=30)
    na, nb = int(rp['totals'][3]), int(rg['totals'][3])
    ov = R.overlap(rp['labels'], rg['labels'], 20, 30)[1:na + 1, 1:nb + 1]
    for min_overlap in (1, 40):
        m = match_lesions(tp, tg, min_overlap=min_overlap)
        assert np.array_equal(m['overlap'], ov)
        p2g = [int(ov[i].argmax()) if ov[i].max() >= min_overlap else -1 for i in range(na)]
        g2p = [int(ov[:, j].argmax()) if ov[:, j].max() >= min_overlap else -1 for j in range(nb)]
        assert m['pred_to_gt'] == p2g and m['gt_to_pred'] == g2p
        tpn = sum(j >= 0 for j in g2p)
        assert (m['tp'], m['fn'], m['fp']) == (tpn, nb - tpn, sum(j < 0 for j in p2g)) and m['tp'] > 0
        assert m['dice'] == {(i, j): 2.0 * int(ov[i, j]) / (int(rp['rows_i'][i, 1]) + int(rg['rows_i'][j, 1])) for i, j in enumerate(p2g) if j >= 0}
    assert match_lesions(tp, tg, 40)['fn'] > match_lesions(tp, tg, 1)['fn']
    seg = np.zeros((3,) + gt.shape, np.uint8)
    seg[0, :, :, :30] = 1
    seg[1, :, :, 30:55] = 1                                                 # x >= 55: no segment; plane 2 stays empty
    names = ['left', 'right', 'nowhere']
    got = locate_lesions(tg, torch.from_numpy(seg).to(DEV), names)
    want = []
    for k in range(nb):
        c = [int(((rg['labels'] == k + 1) & (seg[s] != 0)).sum()) for s in range(3)]
        want.append(names[int(np.argmax(c))] if max(c) > 0 else 'u')
    assert got == want and {'left', 'right', 'u'} <= set(got) and 'nowhere' not in got


def test_packed_bits_input_equals_its_unpacked_twin():
    from rsuper_amd.inference import lesion_table
    from rsuper_amd.training.dataset.packed import pack_bits_device
    planes = inputs('three')
    C = 11
    vol = np.zeros((1, C) + planes.shape[1:], np.uint8)
    chs = [9, 2, 10]
    for c, m in zip(chs, planes):
        vol[0, c] = m
    vol[0, 5] = 1                                                           # a channel that is not asked for
    packed = pack_bits_device(torch.from_numpy(vol).to(DEV))
    a = lesion_table(packed, spacing=ANISO, conn=6, return_labels=True, channels=chs)
    b = lesion_table(torch.from_numpy(planes).to(DEV), spacing=ANISO, conn=6, return_labels=True)
    for x, y in zip(a.host(), b.host()):
        assert x.tobytes() == y.tobytes()
    assert torch.equal(a.labels, b.labels) and not a.single
    compare(*a.host(), a.labels.cpu().numpy(), ref('three', 6, ANISO), 'packed')
    with pytest.raises(ValueError):
        lesion_table(packed)
    with pytest.raises(ValueError):
        lesion_table(packed, channels=[11])


# ------------------------------------------------------------------------------------------------ predict_abdomenatlas --lesion_table
CLASSES = ['kidney_left', 'kidney_lesion', 'kidney_right', 'liver', 'liver_lesion', 'pancreas', 'pancreatic_lesion']
LESIONS = [c for c in CLASSES if c.endswith('_lesion')]
SPACING = {'BDMAP_00000001': (1.0, 1.0, 1.0), 'BDMAP_00000002': (1.5, 0.8, 1.25)}
SHAPES = {'BDMAP_00000001': (40, 36, 44), 'BDMAP_00000002': (38, 36, 42)}


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = os.path.join(d, f)
    return out


def test_predict_abdomenatlas_lesion_table_flag(tmp_path):
    """Two synthetic cases through the command with and without --lesion_table: lesions.csv holds the rows a direct lesion_table call gives for the
    saved planes (counts checked against scipy), and apart from that file both runs write the same files with the same arrays."""
    import resample_ref as rr
    import synth
    from scipy import ndimage
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd.inference import lesion_table, locate_lesions
    from rsuper_amd.inference.lesions import CSV_COLUMNS, csv_text, lesion_csv_rows
    from rsuper_amd.model.dim3.unet import UNet
    d = str(tmp_path)
    os.makedirs(os.path.join(d, 'img'))
    os.makedirs(os.path.join(d, 'run7'))
    with open(os.path.join(d, 'classes.yaml'), 'w') as f:
        f.write('[' + ', '.join(CLASSES) + ']\n')
    with open(os.path.join(d, 'unet8.yaml'), 'w') as f:
        f.write('in_chan: 1\nbase_chan: 8\ndown_scale: [[2,2,2], [2,2,2], [2,2,2], [2,2,2]]\nkernel_size: [[3,3,3], [3,3,3], [3,3,3], [3,3,3], [3,3,3]]\n'
                'block: BasicBlock\nnorm: in\ncompute_dtype: f32\ntraining_size: [32, 32, 32]\n')
    with open(os.path.join(d, 'spacing.csv'), 'w') as f:
        f.write('BDMAP_ID,z,y,x\n' + ''.join(f'{k},{v[0]},{v[1]},{v[2]}\n' for k, v in SPACING.items()))
    net = UNet(1, 8, num_classes=len(CLASSES), block='BasicBlock', norm='in', compute_dtype='f32')
    sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 7)
    torch.save({'epoch': 1, 'model_state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, os.path.join(d, 'run7', 'latest.pth'))
    for k, (case, shape) in enumerate(SHAPES.items()):
        np.savez(os.path.join(d, 'img', case + '.npz'), rr.ct_volume(shape, -200.0, 400.0, 40 + k, np.int16))

    def argv(save):
        return ['--load', os.path.join(d, 'run7', 'latest.pth'), '--img_path', os.path.join(d, 'img'), '--class_list', os.path.join(d, 'classes.yaml'),
                '--config', os.path.join(d, 'unet8.yaml'), '--save_path', os.path.join(d, save), '--dataset', 'synthetic',
                '--spacing_csv', os.path.join(d, 'spacing.csv')]

    done, _ = P.main(argv('plain'))
    done2, _ = P.main(argv('les') + ['--lesion_table', '--lesion_min_voxels', '2'])
    assert done == done2 == sorted(SHAPES)
    plain, les = tree(os.path.join(d, 'plain')), tree(os.path.join(d, 'les'))
    csv_rel = os.path.join('synthetic', 'run7', 'lesions.csv')
    assert sorted(les) == sorted(list(plain) + [csv_rel]) and csv_rel not in plain
    for rel, path in plain.items():
        with np.load(path) as x, np.load(les[rel]) as y:
            assert x.files == y.files and all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in x.files), rel
    rows, n = [], 0
    for case in sorted(SHAPES):
        planes = {}
        for c in CLASSES:
            with np.load(os.path.join(d, 'plain', 'synthetic', 'run7', case, 'predictions', c + '.npz')) as z:
                planes[c] = z['arr_0']
        stack = torch.from_numpy(np.stack([planes[c] for c in LESIONS])).to(DEV)
        t = lesion_table(stack, spacing=SPACING[case], min_voxels=2, return_labels=True)
        for p, c in enumerate(LESIONS):
            sizes = np.bincount(ndimage.label(planes[c], structure=R.STRUCT[26])[0].ravel())[1:]
            assert t.count(p) == min(64, int((sizes >= 2).sum()))
            loc = None
            if c == 'kidney_lesion' and t.count(p):
                loc = locate_lesions(t.plane(p), torch.from_numpy(np.stack([planes['kidney_left'], planes['kidney_right']])).to(DEV),
                                     ['kidney_left', 'kidney_right'])
            rows += lesion_csv_rows(t, case, c, loc, plane=p)
            n += t.count(p)
    text = open(les[csv_rel]).read()
    print(f'lesions.csv: {n} rows')
    assert text.splitlines()[0].split(',') == list(CSV_COLUMNS) and text == csv_text(rows)


def test_measure_lesions_tool_end_to_end(tmp_path):
    """tools.measure_lesions on a two-case packed directory: the rows of reports.csv are those the restatement gives, located in the kidney planes,
    and estimate_tumor_volume reads them."""
    from rsuper_amd.tools import measure_lesions as M
    from rsuper_amd.training.dataset.augmented import estimate_tumor_volume
    classes = ['kidney_left', 'kidney_lesion', 'kidney_right', 'liver', 'liver_lesion']
    root = tmp_path / 'packed'
    (root / 'list').mkdir(parents=True)
    (root / 'list' / 'label_names.yaml').write_text(''.join(f'- {c}\n' for c in reversed(classes)))
    shape = (12, 20, 40)
    spacing = {'BDMAP_00000001': (1.0, 1.0, 1.0), 'BDMAP_00000002': (2.0, 0.5, 0.75)}
    (tmp_path / 'spacing.csv').write_text('BDMAP_ID,z,y,x\nBDMAP_00000002,2.0,0.5,0.75\n')
    want = []
    for k, cid in enumerate(sorted(spacing)):
        lab = np.zeros((5,) + shape, np.uint8)
        lab[0, :, :, :15] = 1                                               # kidney_left
        lab[2, :, :, 25:] = 1                                               # kidney_right
        lab[3, 2:10, 2:18, 10:30] = 1                                       # liver
        lab[1, 3:6, 4:9, 2 + k:9] = 1                                       # kidney lesions: left, right, between the two, a small one astride
        lab[1, 7:9, 10:12, 30:38] = 1
        lab[1, 5, 15, 18:22] = 1
        lab[1, 10, 1, 13:17 + k] = 1
        lab[4, 4:7, 5 + k:12, 12:20] = 1                                    # liver lesions
        lab[4, 8, 16, 28] = 1
        np.save(root / f'{cid}_gt.npy', np.packbits(lab, axis=0))
        sp = spacing[cid]
        for c, organ, segs in ((1, 'kidney', (0, 2)), (4, 'liver', ())):
            t = R.table(lab[c], spacing=sp, conn=26)
            for r in range(int(t['totals'][3])):
                ov = [int(((t['labels'] == r + 1) & (lab[s] != 0)).sum()) for s in segs]
                loc = classes[segs[int(np.argmax(ov))]] if segs and max(ov) > 0 else 'u'
                a, b, cc = t['rows_f'][r, 1:]
                ip = (sp[1] + sp[2]) / 2
                want.append({'BDMAP ID': cid, 'Standardized Organ': organ, 'Standardized Location': loc,
                             'Tumor Size (mm)': f'{a + ip:.1f} x {b + ip:.1f} x {cc + sp[0]:.1f}'})
    out = tmp_path / 'reports.csv'
    argv = ['--data_root', str(root), '--out', str(out), '--spacing_csv', str(tmp_path / 'spacing.csv')]
    cases, n = M.main(argv + ['--parts', '2', '--current_part', '0'])
    assert cases == ['BDMAP_00000001'] and n == 6
    cases, n = M.main(argv + ['--parts', '2', '--current_part', '1'])
    assert cases == ['BDMAP_00000002'] and n == 6
    import csv
    with open(out, newline='') as f:
        got = list(csv.DictReader(f))
    print(got)
    assert got == want and {r['Standardized Location'] for r in got} == {'kidney_left', 'kidney_right', 'u'}
    assert got[0]['Tumor Size (mm)'] == '8.2 x 7.7 x 3.0'                    # 5 x 7 voxels in the slice, 3 slices: sqrt(16 + 36) + 1, 2 * 4 * 6 / sqrt(52) + 1, 2 + 1
    vols, diam = estimate_tumor_volume([r for r in got if r['BDMAP ID'] == 'BDMAP_00000001'], ['kidney'])
    assert (diam[:4] > 0).all() and not diam[4:].any() and vols[0] > 0
