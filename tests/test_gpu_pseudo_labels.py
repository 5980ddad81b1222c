"""MI355X tests of the report-guided pseudo-label refinement (baselines/pseudo_labels; kernels in csrc/pseudo_label.hip) against the reference's own
results (tests/golden/pseudo_labels.npz / .json, written by tests/golden/gen_golden_pseudo_labels.py) and the scipy restatement
tests/pseudo_labels_ref.py.  Everything is integer: every comparison is exact."""
import ctypes
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
import pseudo_labels_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'pseudo_labels.npz'))
J = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'pseudo_labels.json')))
CALLS = {c['name']: c for c in J['calls']}


def _expected(c):
    x = G[c['input'] + '_x']
    return x, np.unpackbits(G[c['name'] + '_mask'])[:x.size].reshape(x.shape)


def _params(c):
    return dict(peak_cut=c['peak_cut'], min_voxels=c['min_voxels'], min_peak=c['min_peak'])


def _abi(x, counts, runs, peak_cut=0.40, min_voxels=11, min_peak=0.01, fill=None, bufs=None):
    """The C ABI on caller-owned buffers: begin, then one run call per entry of `runs` (its iteration count).  fill: how out, state and the workspace
    are pre-filled ('ff' bytes or 'nan' words).  bufs: (out, state, workspace) of an earlier call, used as they are."""
    from rsuper_amd.hip import lib
    L = lib.lib()
    x = x[None] if x.ndim == 3 else x
    P, D, H, W = x.shape
    work = torch.from_numpy(x).to(DEV).contiguous()
    if bufs is None:
        out = torch.empty((P, D, H, W), device=DEV, dtype=torch.uint8)
        state = torch.empty((P, 8), device=DEV, dtype=torch.int32)
        ws = torch.empty((L.rsuper_lesion_candidates_workspace_bytes(P, D, H, W) // 4,), device=DEV, dtype=torch.float32)
        if fill == 'ff':
            out.fill_(0xFF), state.fill_(-1), ws.view(torch.int32).fill_(-1)
        elif fill == 'nan':
            out.fill_(0x7F), state.view(torch.float32).fill_(float('nan')), ws.fill_(float('nan'))
    else:
        out, state, ws = bufs
    st = torch.cuda.current_stream().cuda_stream
    lib.check(L.rsuper_lesion_candidates_begin(out.data_ptr(), P, D, H, W, (ctypes.c_int * P)(*counts), state.data_ptr(), st), 'begin')
    for k in runs:
        lib.check(L.rsuper_lesion_candidates_run(work.data_ptr(), out.data_ptr(), P, D, H, W, peak_cut, min_voxels, min_peak, state.data_ptr(),
                                                 ws.data_ptr(), k, st), 'run')
    torch.cuda.synchronize()
    return work, out, state, ws


@pytest.mark.parametrize('name', sorted(CALLS))
def test_every_fixture_call_is_bit_exact(name):
    from rsuper_amd.baselines.pseudo_labels import extract_lesion_candidates, last_state
    c = CALLS[name]
    x, want = _expected(c)
    t = torch.from_numpy(x).to(DEV)
    mask, kept = extract_lesion_candidates(t, c['n_lesions'], **_params(c))
    assert mask.dtype == torch.uint8 and mask.shape == t.shape and mask.is_cuda
    got = mask.cpu().numpy()
    print(name, 'kept', kept, 'iterations', last_state['iterations'], 'voxels', int(got.sum()), 'reads', last_state['reads'])
    assert kept == c['kept'] and last_state['iterations'] == [c['iterations']] and last_state['kept'] == [c['kept']]
    assert int(got.sum()) == c['voxels'] and np.array_equal(got, want)
    assert np.array_equal(t.cpu().numpy(), x)                                   # the input is left as it was


@pytest.mark.parametrize('name', ['reject_n3_v11', 'smooth_0_1', 'smooth_2_3', 'speckle', 'plateau', 'minpeak_lt'])
def test_the_batch_size_does_not_change_the_result(name):
    from rsuper_amd.baselines.pseudo_labels import extract_lesion_candidates, last_state
    c = CALLS[name]
    x, want = _expected(c)
    t = torch.from_numpy(x).to(DEV)
    reads = {}
    for batch in (1, 7, 64):
        mask, kept = extract_lesion_candidates(t, c['n_lesions'], batch=batch, **_params(c))
        assert np.array_equal(mask.cpu().numpy(), want) and kept == c['kept'] and last_state['iterations'] == [c['iterations']], batch
        assert last_state['batch'] == batch
        reads[batch] = last_state['reads'][0]
    print(name, 'reads per batch size', reads)
    assert reads[1] >= reads[7] >= reads[64] == 1
    assert reads[1] <= c['iterations'] + 1


def test_iterations_enqueued_after_the_end_touch_nothing():
    """`ties` is finished after one iteration: one iteration and 64 enqueued iterations leave byte-identical out and work, and 64 more on the finished
    state leave out, work and every state word as they are."""
    c = CALLS['ties']
    x, want = _expected(c)
    w1, o1, s1, _ = _abi(x, [1], [1], fill='ff')
    w64, o64, s64, ws = _abi(x, [1], [64], fill='ff')
    assert torch.equal(o1, o64) and torch.equal(w1.view(torch.int32), w64.view(torch.int32))
    assert np.array_equal(o1.cpu().numpy()[0], want)
    left = x.copy()
    left[want > 0] = 0
    assert np.array_equal(w1.cpu().numpy()[0].view(np.int32), left.view(np.int32))
    a, b = s1.cpu().numpy()[0], s64.cpu().numpy()[0]
    assert a[:2].tolist() == [1, 1] == b[:2].tolist() and b[2] == 1             # kept, iterations; the longer run has also seen the end
    from rsuper_amd.hip import lib
    before = (w64.clone(), o64.clone(), s64.clone())
    lib.check(lib.lib().rsuper_lesion_candidates_run(w64.data_ptr(), o64.data_ptr(), 1, *x.shape, 0.40, 11, 0.01, s64.data_ptr(), ws.data_ptr(), 64,
                                                     torch.cuda.current_stream().cuda_stream), 'run')
    torch.cuda.synchronize()
    assert torch.equal(before[0].view(torch.int32), w64.view(torch.int32)) and torch.equal(before[1], o64) and torch.equal(before[2], s64)


def _embed(v, shape):
    out = np.zeros(shape, np.float32)
    out[tuple(slice(0, n) for n in v.shape)] = v
    return out


@pytest.fixture(scope='module')
def five_planes():
    """Five planes of one shape with different content and counts: a serpentine, rejected components, two plateaus, n = 0, a stop at min_peak."""
    shape = (17, 18, 70)
    planes = [pr.snake_volume(), _embed(pr.reject_volume(), shape), _embed(pr.plateau_volume(), shape), _embed(pr.ties_volume(), shape),
              _embed(pr.minpeak_volume(True), shape)]
    counts = [1, 3, 2, 0, 1]
    ref = [pr.candidates(v, n) for v, n in zip(planes, counts)]
    assert [r[1] for r in ref] == [1, 2, 2, 0, 0] and [r[2] for r in ref] == [1, 3, 2, 0, 0]
    return np.stack(planes), counts, ref


def test_planes_of_one_call_equal_their_single_calls(five_planes):
    from rsuper_amd.baselines.pseudo_labels import extract_lesion_candidates, last_state
    x, counts, ref = five_planes
    t = torch.from_numpy(x).to(DEV)
    masks, kept = extract_lesion_candidates(t, counts)
    its = list(last_state['iterations'])
    assert masks.shape == t.shape and kept == [r[1] for r in ref] and its == [r[2] for r in ref]
    assert last_state['reads'][3] == 0
    for p in range(len(counts)):
        m1, k1 = extract_lesion_candidates(t[p], counts[p])
        assert torch.equal(m1, masks[p]) and k1 == kept[p] and last_state['iterations'] == [its[p]], p
        assert np.array_equal(m1.cpu().numpy(), ref[p][0]), p
    assert np.array_equal(t.cpu().numpy(), x)


@pytest.mark.parametrize('fill', ['ff', 'nan'])
def test_prefilled_buffers_and_a_reused_workspace_give_the_same_result(five_planes, fill):
    x, counts, ref = five_planes
    want = np.stack([r[0] for r in ref])
    w, o, s, ws = _abi(x, counts, [4], fill=fill)
    first = (w.clone(), o.clone(), s.clone())
    assert np.array_equal(o.cpu().numpy(), want)
    sh = s.cpu().numpy()
    assert sh[:, 0].tolist() == [r[1] for r in ref] and sh[:, 1].tolist() == [r[2] for r in ref] and sh[:, 3].tolist() == counts
    w2, o2, s2, _ = _abi(x, counts, [2, 2], bufs=(o, s, ws))                    # the same buffers as the first call left them
    assert torch.equal(o2, first[1]) and torch.equal(s2, first[2]) and torch.equal(w2.view(torch.int32), first[0].view(torch.int32))


def test_refine_case_on_the_case_fixture():
    from rsuper_amd.baselines.pseudo_labels import refine_case
    case = J['case']
    raw = torch.from_numpy(G['case_raw']).to(DEV)
    for f in case['folders']:
        row = None if f['row'] is None else {k: (float('nan') if v == 'NaN' else v) for k, v in f['row'].items()}
        r = torch.stack([raw, 1.0 - raw], dim=-1) if f['four_d'] else raw
        included, masks = refine_case(r, case['classes'], row)
        assert included == f['included'] and sorted(masks) == f['masks'], f['id']
        for name, m in masks.items():
            want = np.unpackbits(G['case_%s_%s' % (f['id'], name)])[:m.numel()].reshape(case['shape'])
            assert m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), want), (f['id'], name)


def test_merge_pseudo_labels_equals_its_numpy_form():
    from rsuper_amd.baselines.pseudo_labels import merge_pseudo_labels
    r = np.random.default_rng(5)
    shape = (5, 7, 19)
    organ_names = ['spleen', 'liver', 'kidney_left', 'aorta']                    # not sorted: planes are taken by name
    organs = (r.random((4,) + shape) < 0.4).astype(np.int8)
    labels = ['liver_lesion', 'aorta', 'kidney_lesion', 'liver', 'pancreatic_lesion', 'spleen', 'kidney_left', 'colon_lesion', 'bladder_lesion']
    masks = {k: (r.random(shape) < 0.3).astype(np.uint8) for k in ('liver_lesion', 'pancreatic_lesion')}
    want = pr.merge_numpy(organs, organ_names, masks, labels)
    dev_masks = {k: torch.from_numpy(v).to(DEV) for k, v in masks.items()}
    got = merge_pseudo_labels(torch.from_numpy(organs).to(DEV), organ_names, dev_masks, labels)
    assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    packed = merge_pseudo_labels(torch.from_numpy(organs).to(DEV), organ_names, dev_masks, labels, packed=True)
    assert packed.C == len(labels) and np.array_equal(packed.packed[0].cpu().numpy(), np.packbits(want, axis=0))
    with pytest.raises(AssertionError):
        merge_pseudo_labels(torch.from_numpy(organs).to(DEV), organ_names, dev_masks, labels + ['stomach'])


def test_a_ct_sized_crop_equals_the_scipy_restatement():
    from scipy import ndimage
    from rsuper_amd.baselines.pseudo_labels import extract_lesion_candidates, last_state
    shape = (96, 128, 128)
    coarse = np.random.default_rng(11).standard_normal((7, 9, 9))
    v = ndimage.zoom(coarse, [s / c for s, c in zip(shape, coarse.shape)], order=1)
    assert v.shape == shape
    x = (1.0 / (1.0 + np.exp(-(3.0 * v - 2.0)))).astype(np.float32)
    want, kept, its = pr.candidates(x, 3)
    assert kept == 3 and 0 < want.sum() < want.size
    mask, k = extract_lesion_candidates(torch.from_numpy(x).to(DEV), 3)
    print('96x128x128: kept', k, 'iterations', last_state['iterations'], 'voxels', int(want.sum()))
    assert k == kept and last_state['iterations'] == [its] and np.array_equal(mask.cpu().numpy(), want)


def test_the_tool_end_to_end_on_the_case_fixture(tmp_path):
    """The folders of the case-level fixture as .npy files, the rows as a CSV: kept / skipped lists, masks and merged training labels."""
    import yaml
    from rsuper_amd.tools import refine_pseudo_labels as tool
    case = J['case']
    classes, raw = case['classes'], G['case_raw']
    cols = sorted({k for f in case['folders'] if f['row'] for k in f['row']})
    lines = ['BDMAP_ID,' + ','.join(cols)]
    root, organs_dir = tmp_path / 'in', tmp_path / 'organs'
    (organs_dir / 'list').mkdir(parents=True)
    organ_names = ['liver', 'kidney_left']
    organs = (np.random.default_rng(2).random((2,) + tuple(case['shape'])) < 0.5).astype(np.int8)
    (organs_dir / 'list' / 'label_names.yaml').write_text(yaml.safe_dump(organ_names))
    labels = ['liver_lesion', 'liver', 'kidney_lesion', 'kidney_left', 'pancreatic_lesion', 'colon_lesion']
    (tmp_path / 'labels.yaml').write_text(yaml.safe_dump(labels))
    for f in case['folders']:
        d = root / (f['id'] + '.npz') / 'predictions_raw'
        d.mkdir(parents=True)
        for c, name in enumerate(classes):
            np.save(d / (name + '.npy'), np.stack([raw[c], 1.0 - raw[c]], axis=-1) if f['four_d'] else raw[c])
        if f['row'] is not None:
            lines.append(f['id'] + ',' + ','.join('' if f['row'].get(k, '') == 'NaN' else str(f['row'].get(k, '')) for k in cols))
        np.savez_compressed(organs_dir / (f['id'] + '_gt.npz'), organs[[1, 0]])                # stored in sorted-name order
        np.savez_compressed(organs_dir / (f['id'] + '.npz'), np.zeros(case['shape'], np.float32))
    (tmp_path / 'meta.csv').write_text('\n'.join(lines) + '\n')
    out, tgt = tmp_path / 'out', tmp_path / 'tgt'
    kept, skipped = tool.main(['--input_dir', str(root), '--metadata', str(tmp_path / 'meta.csv'), '--out_npz_dir', str(out),
                               '--label_list', str(tmp_path / 'labels.yaml'), '--organs_path', str(organs_dir), '--tgt_path', str(tgt)])
    # a missing column is an empty cell in a CSV: NaN, excluded all the same
    assert kept == [f['id'] for f in case['folders'] if f['included']] and skipped == [f['id'] for f in case['folders'] if not f['included']]
    for f in case['folders']:
        written = sorted(p.name[:-4] for p in (out / f['id']).iterdir()) if (out / f['id']).exists() else []
        assert written == f['masks'], f['id']
        masks = {}
        for name in written:
            m = np.load(out / f['id'] / (name + '.npz'))['mask']
            masks[name] = m
            assert m.dtype == np.uint8 and np.array_equal(m, np.unpackbits(G['case_%s_%s' % (f['id'], name)])[:m.size].reshape(case['shape']))
        if f['included']:
            want = pr.merge_numpy(organs[[1, 0]], sorted(organ_names), masks, labels)
            assert np.array_equal(np.load(tgt / (f['id'] + '_gt.npz'))['arr_0'], want) and (tgt / (f['id'] + '.npz')).exists()
        else:
            assert not (tgt / (f['id'] + '_gt.npz')).exists()
    assert yaml.safe_load((tgt / 'list' / 'label_names.yaml').read_text()) == sorted(labels)


def _nan_planes():
    """ties with: a positive NaN, a negative NaN, only NaN, +inf on the second block, and untouched."""
    base = pr.ties_volume()
    pos, neg, allnan, inf = base.copy(), base.copy(), np.full_like(base, np.nan), base.copy()
    pos[4, 4, 20] = np.nan
    neg[4, 4, 20] = -np.nan
    assert not np.signbit(pos[4, 4, 20]) and np.signbit(neg[4, 4, 20])
    inf[7, 7, 31] = np.inf
    return np.stack([pos, neg, allnan, inf, base])


def test_a_nan_plane_is_ended_and_the_call_returns():
    """NaN is the caller's error and the result unspecified, but every plane ends: a NaN peak sets `done` with no iteration, a negative NaN orders
    below everything and never enters a mask, +inf is a peak like any other.  The planes next to them are exact."""
    from rsuper_amd.baselines.pseudo_labels import extract_lesion_candidates, last_state
    x = _nan_planes()
    counts = [2, 2, 1, 1, 2]
    w, o, s, _ = _abi(x, counts, [4], fill='ff')
    sh, out = s.cpu().numpy(), o.cpu().numpy()
    print('state (kept, iterations, done):', sh[:, :3].tolist())
    want, kept, its = pr.candidates(x[4], 2)
    assert sh[0, :3].tolist() == [0, 0, 1] and not out[0].any()                              # positive NaN: ended before the first pass
    assert sh[2, :3].tolist() == [0, 0, 1] and not out[2].any()
    assert sh[1, :2].tolist() == [kept, its] and np.array_equal(out[1], want)                # negative NaN: as if it were not there
    assert sh[4, :2].tolist() == [kept, its] and np.array_equal(out[4], want)
    winf, kinf, iinf = pr.candidates(x[3], 1)                                                # thr = inf: the inf voxel alone, rejected; then the first block
    assert (kinf, iinf) == (1, 2) and winf.sum() == 12 and winf[7, 7, 31] == 0
    assert sh[3, :2].tolist() == [kinf, iinf] and np.array_equal(out[3], winf)
    assert np.array_equal(w.cpu().numpy()[0].view(np.int32), x[0].view(np.int32))            # the NaN plane's work is untouched
    masks, k = extract_lesion_candidates(torch.from_numpy(x).to(DEV), counts, batch=1)
    assert k == sh[:, 0].tolist() and last_state['iterations'] == sh[:, 1].tolist() and np.array_equal(masks.cpu().numpy(), out)
    assert max(last_state['reads']) <= its + 1


def test_more_planes_than_one_launch_group_takes():
    """65 planes run as a group of 64 and a group of one, each with its own workspace: per plane the single call's result, iterations and reads."""
    from rsuper_amd.baselines.pseudo_labels import extract_lesion_candidates, last_state
    base = [pr.reject_volume(), _embed(pr.ties_volume(), (9, 10, 36)), _embed(pr.bridge_volume(), (9, 10, 36))]
    params = [(3, 11), (1, 11), (0, 11)]
    ref = [pr.candidates(v, n) for v, (n, _) in zip(base, params)]
    x = np.stack([base[p % 3] for p in range(64)] + [base[0]])
    counts = [params[p % 3][0] for p in range(64)] + [2]                                     # the last group's only plane: reject with n = 2
    ref64 = pr.candidates(base[0], 2)
    masks, kept = extract_lesion_candidates(torch.from_numpy(x).to(DEV), counts, batch=2)
    got = masks.cpu().numpy()
    for p in range(65):
        r = ref64 if p == 64 else ref[p % 3]
        assert kept[p] == r[1] and last_state['iterations'][p] == r[2] and np.array_equal(got[p], r[0]), p
    reads = last_state['reads']
    assert reads[0] == 2 and reads[1] == 1 and reads[2] == 0 and reads[63] == reads[0] and reads[64] == 2 and len(reads) == 65


# a voxel and its backward neighbour (dz, dy, dx) on either side of a corner of the 8 x 8 x 32 labelling tile of a (9, 9, 33) volume
TILE_CORNER_PAIRS = {(-1, -1, -1): ((8, 8, 32), (7, 7, 31)), (-1, 1, 1): ((8, 7, 31), (7, 8, 32)), (0, -1, 1): ((4, 8, 31), (4, 7, 32))}


@pytest.mark.parametrize('d', sorted(TILE_CORNER_PAIRS))
def test_a_diagonal_pair_across_a_tile_corner_is_one_component(d):
    """26-connectivity at a tile corner: two equal peak voxels that touch only diagonally, in tiles that share no face, are one component of size 2,
    kept in the first iteration with min_voxels = 2; a lower three-voxel run across the x = 31 | 32 tile face stays out of it."""
    from rsuper_amd.baselines.pseudo_labels import extract_lesion_candidates, last_state
    a, b = TILE_CORNER_PAIRS[d]
    assert tuple(p - q for p, q in zip(b, a)) == d
    v = np.zeros((9, 9, 33), np.float32)
    v[a] = v[b] = 0.9
    v[2, 2, 30:33] = 0.5                                                        # inside the mask (thr = 0.36), not adjacent to the pair
    want = np.zeros(v.shape, np.uint8)
    want[a] = want[b] = 1
    ref = pr.candidates(v, 1, min_voxels=2)
    assert np.array_equal(ref[0], want) and ref[1:] == (1, 1)
    mask, kept = extract_lesion_candidates(torch.from_numpy(v).to(DEV), 1, min_voxels=2)
    assert np.array_equal(mask.cpu().numpy(), ref[0]) and kept == ref[1] and last_state['iterations'] == [ref[2]]
