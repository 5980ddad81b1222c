"""MI355X tests of the device DEFLATE encoder (csrc/deflate.hip, inference/npz_writer.py).  For every input and both code tables: zlib inflates the device
stream to the input, the stream equals the bytes of the pure-Python restatement tests/deflate_ref.py, the CRC-32 equals zlib's, the length respects
rsuper_deflate_bound, and a second call gives the same bytes.  Then the file writers and the --device_compress flag of predict_abdomenatlas end to end."""
import gzip
import os
import sys
import zipfile
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import deflate_ref as R  # noqa: E402
import resample_ref as rr  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TABLES = ('fixed', 'mask')
S, C = R.SEG, R.CHUNK
DIST_BASES = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)


def ball40():
    z, y, x = np.mgrid[:40, :40, :40]
    return ((z - 20) ** 2 + (y - 19) ** 2 + (x - 21) ** 2 < 15 ** 2).astype(np.uint8)


def runs_1_to_600():
    """Runs of every length 1..600, the value alternating: every length code and every extra-bit value of the length alphabet."""
    return np.concatenate([np.full(k, k & 1, np.uint8) for k in range(1, 601)])


def every_length():
    """One segment per match length 3..258: 0 / 1 alternating, then L + 1 equal bytes up to the end of the segment -- a match of exactly L, whatever the
    segment boundaries do to the ladder above."""
    segs = []
    for L in range(3, 259):
        f = S - (L + 1)
        segs.append(np.concatenate([((np.arange(f) + f + 1) & 1).astype(np.uint8), np.ones(L + 1, np.uint8)]))  # the filler ends in 0
    return np.concatenate(segs)


def fit(a, n):
    """The first n bytes of `a` repeated."""
    a = np.asarray(a, np.uint8).ravel()
    return np.resize(a, n) if n else np.zeros(0, np.uint8)


def contents(n, seed=0):
    """The eight content classes at n bytes."""
    r = np.random.default_rng(seed + n)
    return [np.zeros(n, np.uint8), np.ones(n, np.uint8), np.full(n, 255, np.uint8), (np.arange(n) & 1).astype(np.uint8),
            r.integers(0, 256, n, dtype=np.uint8), fit(runs_1_to_600(), n), fit(ball40(), n), fit(np.packbits(ball40().ravel()), n)]


def lib():
    from rsuper_amd.hip import lib as _l
    return _l.lib()


def check(planes, pitch, table):
    """planes: equally long uint8 arrays, one device call (and a second one)."""
    from rsuper_amd.inference import deflate_device
    n = len(planes[0])
    stack = torch.from_numpy(np.stack(planes)).to(DEV)
    streams, crcs = deflate_device(stack, pitch=pitch, table=table)
    again, crcs2 = deflate_device(stack, pitch=pitch, table=table)
    assert len(streams) == len(planes)
    bound = lib().rsuper_deflate_bound(n)
    for k, x in enumerate(planes):
        raw = x.tobytes()
        assert zlib.decompress(streams[k], wbits=-15) == raw, f'plane {k}: the device stream does not inflate to the input'
        assert streams[k] == R.stream(raw, pitch, table), f'plane {k}: the device stream is not the restatement\'s'
        assert crcs[k] == zlib.crc32(raw), f'plane {k}: CRC'
        assert len(streams[k]) <= bound, f'plane {k}: {len(streams[k])} bytes > bound {bound}'
    assert again == streams and crcs2 == crcs, 'a second call gave other bytes'
    return streams


def test_geometry_and_bound():
    L = lib()
    assert L.rsuper_deflate_chunk_bytes() == C and L.rsuper_deflate_segment_bytes() == S and C % S == 0
    for n in (0, 1, 1000, C, C + 1, 10 * C, (1 << 32) - 1):
        assert L.rsuper_deflate_bound(n) <= n + n // 1024 + 64
    assert L.rsuper_deflate_bound(0) == 5


SIZES = (0, 1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 516, 517, S - 1, S, S + 1, C - 1, C, C + 1, 2 * C + 17)


@pytest.mark.parametrize('table', TABLES)
@pytest.mark.parametrize('n', sorted(set(SIZES)))
def test_sizes(n, table):
    """Every size of the list with every content class, eight planes in one call; rows of 40 bytes (the ball's)."""
    check(contents(n), 40, table)


@pytest.mark.parametrize('table', TABLES)
def test_contents_at_their_own_size(table):
    """The run ladder (180300 bytes), one segment per match length (every length code and extra-bit value, in coded chunks), the ball with its rows and the
    bit-packed ball with its rows."""
    runs = runs_1_to_600()
    s = check([runs], 0, table)
    each = every_length()
    assert {t[1] for t in R.tokens(each.tobytes(), 0) if t[0] == 'match'} == set(range(3, 259))
    for lo in range(0, len(each), C):
        assert len(R.stream(each[lo:lo + C].tobytes(), 0, table)) < len(each[lo:lo + C])       # coded, not stored: the match codes reach the stream
    check([each], 0, table)
    ball = ball40()
    check([ball.ravel()], 40, table)
    check([np.packbits(ball.ravel())], 5, table)
    check([np.packbits(ball, axis=0).ravel()], 40, table)
    assert len(s[0]) < len(runs) // 8


@pytest.mark.parametrize('table', TABLES)
def test_incompressible_planes_are_stored(table):
    """Alternating 0 / 1 under the fixed code (no match of 3, 8 bits a literal) and random bytes under either fall back to stored blocks."""
    n = C + 100
    alt, rnd = (np.arange(n) & 1).astype(np.uint8), np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8)
    s = check([alt, rnd], 0, table)
    stored = n + 5 * 2 + 5
    assert len(s[1]) == stored
    if table == 'fixed':
        assert len(s[0]) == stored
    else:
        assert len(s[0]) < n // 2                                  # 2 bits a literal


@pytest.mark.parametrize('table', TABLES)
@pytest.mark.parametrize('pitch', DIST_BASES + (32768,))
def test_pitch_at_every_distance_code(pitch, table):
    """Three identical rows and 7 bytes of a fourth: rows 2 and 3 are matches at distance `pitch`, the base of each distance code and the largest
    extra-bit value."""
    row = np.random.default_rng(pitch).integers(0, 256, pitch, dtype=np.uint8)
    x = fit(row, 3 * pitch + 7)
    check([x], pitch, table)
    if pitch >= 3:
        assert any(t[0] == 'match' and t[2] == pitch for t in R.tokens(x.tobytes(), pitch))


def test_pitch_above_the_window_is_refused():
    from rsuper_amd.inference import deflate_device, npz_writer as nw
    x = torch.zeros((1, 100), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        deflate_device(x, pitch=32769)
    t = nw.fixed_table()
    words, header = nw._device_table(t, x.device)
    out = torch.zeros(256, dtype=torch.uint8, device=DEV)
    meta = torch.zeros((3, 1), dtype=torch.int64, device=DEV)
    ws = torch.zeros(lib().rsuper_deflate_workspace_bytes(1, 100), dtype=torch.uint8, device=DEV)
    args = lambda pitch: (x.data_ptr(), 100, 100, 1, pitch, words.data_ptr(), header.data_ptr(), 3, out.data_ptr(), meta[0].data_ptr(),  # noqa: E731
                          meta[1].data_ptr(), meta[2].data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert lib().rsuper_deflate_planes(*args(32769)) == 1          # RSUPER_ERR_ARG, nothing launched
    assert lib().rsuper_deflate_planes(*args(-1)) == 1
    assert lib().rsuper_deflate_planes(*args(32768)) == 0
    torch.cuda.synchronize()
    with pytest.raises(Exception):
        deflate_device(torch.zeros((1, 100), dtype=torch.uint8))      # a host tensor reaches no kernel
    with pytest.raises(Exception):
        torch.ops.rsuper.deflate_planes(torch.zeros(100, dtype=torch.uint8), 100, 100, 1, 0, words.cpu(), header.cpu(), 3)


@pytest.mark.parametrize('table', TABLES)
def test_rows_across_chunks_first_row_and_short_plane(table):
    """Rows whose row above lies in the chunk before (and a row that straddles the chunk boundary); a first row, which has no row above; a plane shorter
    than one row."""
    r = np.random.default_rng(9)
    for pitch in (1000, 4096, 20000):
        rows = (C + 3 * pitch) // pitch + 1
        row = r.integers(0, 2, pitch, dtype=np.uint8)
        x = np.tile(row, rows)
        x[pitch * (rows // 2) + 3] ^= 1                            # one row differs from its neighbours at one place
        s = check([x], pitch, table)
        assert len(s[0]) <= pitch + 5 + len(x) // 64 + 256         # the first row at 8 bits a byte or less, 26 bits or less per 258 bytes after it
        cut = [t for t in R.tokens(x[:C + 2 * pitch].tobytes(), pitch) if t[0] == 'match' and t[2] == pitch]
        assert cut
    check([r.integers(0, 2, 777, dtype=np.uint8)], 777, table)     # exactly one row
    check([r.integers(0, 2, 30, dtype=np.uint8)], 40, table)       # shorter than a row
    check([np.zeros(30, np.uint8)], 32768, table)


@pytest.mark.parametrize('table', TABLES)
@pytest.mark.parametrize('off', (1, 2, 3))
def test_batch_with_unaligned_source_and_stride(off, table):
    """Three planes in one call -- all zero, random (stored between two coded planes), the ball -- from a view that starts `off` bytes after a 16-byte
    boundary, the planes n + 13 bytes apart."""
    from rsuper_amd.inference import npz_writer as nw
    n, stride = 64000, 64013
    planes = [np.zeros(n, np.uint8), np.random.default_rng(off).integers(0, 256, n, dtype=np.uint8), ball40().ravel()]
    host = np.full(16 + 3 * stride, 0xA5, np.uint8)
    for k, x in enumerate(planes):
        host[off + k * stride: off + k * stride + n] = x
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off: off + 2 * stride + n]
    streams, crcs = nw.deflate_strided(view, n, stride, 3, 40, table)
    again, _ = nw.deflate_strided(view, n, stride, 3, 40, table)
    for k, x in enumerate(planes):
        assert zlib.decompress(streams[k], wbits=-15) == x.tobytes()
        assert streams[k] == R.stream(x.tobytes(), 40, table)
        assert crcs[k] == zlib.crc32(x.tobytes())
    assert again == streams
    assert len(streams[1]) == n + 5 * 2 + 5 and len(streams[0]) < 1000 and len(streams[2]) < n // 8


def test_all_equal_plane_size_under_the_fixed_code():
    """13 bits per 258-byte match: an all-equal plane of n >= 64 KiB gives at most n / 128 + 256 bytes."""
    from rsuper_amd.inference import deflate_device
    for n, v in ((65536, 0), (2 * C + 17, 1), (200000, 255)):
        (s,), _ = deflate_device(torch.full((1, n), v, dtype=torch.uint8, device=DEV), table='fixed')
        assert zlib.decompress(s, wbits=-15) == bytes([v]) * n
        assert len(s) <= n // 128 + 256, (n, len(s))


# ------------------------------------------------------------------------------------------------ files
@pytest.mark.parametrize('table', TABLES)
def test_savez_compressed_device_equals_numpy(tmp_path, table):
    from rsuper_amd.inference import savez_compressed_device, save_planes_npz, gzip_device
    r = np.random.default_rng(3)
    stack = (r.random((5, 12, 10, 14)) < 0.3).astype(np.uint8)
    stack[1] = 0
    names = np.array(['liver', 'pancreas'])
    dev = torch.from_numpy(stack).to(DEV)
    a, b = str(tmp_path / 'host.npz'), str(tmp_path / 'dev')
    np.savez_compressed(a, stack, stack[2].astype(bool), classes=names, mask=stack[3])
    savez_compressed_device(b, dev, dev[2].bool(), table=table, classes=names, mask=dev[3])
    assert os.path.exists(b + '.npz') and zipfile.ZipFile(b + '.npz').testzip() is None
    with np.load(a) as za, np.load(b + '.npz') as zb:
        assert sorted(za.files) == sorted(zb.files) == ['arr_0', 'arr_1', 'classes', 'mask']
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and np.array_equal(za[k], zb[k]), k
    paths = [str(tmp_path / f'plane{k}.npz') for k in range(5)]
    save_planes_npz(paths, dev, key='mask', table=table)
    for k, p in enumerate(paths):
        with np.load(p) as z:
            assert z.files == ['mask'] and z['mask'].dtype == np.uint8 and np.array_equal(z['mask'], stack[k])
    assert gzip.decompress(gzip_device(dev, table=table)) == stack.tobytes()
    assert gzip.decompress(gzip_device(dev[0, 0, 0, :0], table=table)) == b''
    with pytest.raises(Exception):
        savez_compressed_device(str(tmp_path / 'f32'), dev.float())


CLASSES = ['kidney_left', 'kidney_lesion', 'kidney_right', 'liver', 'liver_lesion', 'pancreas', 'pancreatic_lesion']
SHAPES = {'BDMAP_00000001': (40, 36, 44), 'BDMAP_00000002': (38, 36, 42)}


@pytest.fixture(scope='module')
def flow_dir(tmp_path_factory):
    """A tiny UNet checkpoint, its config and two synthetic cases."""
    from rsuper_amd.model.dim3.unet import UNet
    d = str(tmp_path_factory.mktemp('deflate_flow'))
    os.makedirs(os.path.join(d, 'img'))
    os.makedirs(os.path.join(d, 'run7'))
    with open(os.path.join(d, 'classes.yaml'), 'w') as f:
        f.write('[' + ', '.join(CLASSES) + ']\n')
    with open(os.path.join(d, 'unet8.yaml'), 'w') as f:
        f.write('in_chan: 1\nbase_chan: 8\ndown_scale: [[2,2,2], [2,2,2], [2,2,2], [2,2,2]]\nkernel_size: [[3,3,3], [3,3,3], [3,3,3], [3,3,3], [3,3,3]]\n'
                'block: BasicBlock\nnorm: in\ncompute_dtype: f32\ntraining_size: [32, 32, 32]\n')
    net = UNet(1, 8, num_classes=len(CLASSES), block='BasicBlock', norm='in', compute_dtype='f32')
    sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 7)
    torch.save({'epoch': 1, 'model_state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, os.path.join(d, 'run7', 'latest.pth'))
    for k, (case, shape) in enumerate(SHAPES.items()):
        np.savez(os.path.join(d, 'img', case + '.npz'), rr.ct_volume(shape, -200.0, 400.0, 40 + k, np.int16))
    return d


def load_tree(root):
    """{relative path: {key: array}} of every .npz under root."""
    out = {}
    for base, _, files in os.walk(root):
        for f in files:
            if f.endswith('.npz'):
                with np.load(os.path.join(base, f)) as z:
                    out[os.path.relpath(os.path.join(base, f), root)] = {k: z[k] for k in z.files}
    return out


@pytest.mark.parametrize('packed', (False, True), ids=('per_class', 'packed'))
def test_predict_with_device_compress_writes_the_same_trees(flow_dir, packed):
    from rsuper_amd import predict_abdomenatlas as P
    d = flow_dir
    trees = {}
    for flag in (False, True):
        save = f'res_{int(packed)}_{int(flag)}'
        argv = ['--load', os.path.join(d, 'run7', 'latest.pth'), '--img_path', os.path.join(d, 'img'), '--class_list', os.path.join(d, 'classes.yaml'),
                '--config', os.path.join(d, 'unet8.yaml'), '--save_path', os.path.join(d, save), '--dataset', 'synthetic', '--organ_mask_on_lesion']
        argv += (['--packed'] if packed else []) + (['--device_compress'] if flag else [])
        done, _ = P.main(argv)
        assert done == sorted(SHAPES)
        trees[flag] = load_tree(os.path.join(d, save))
    host, dev = trees[False], trees[True]
    assert sorted(host) == sorted(dev) and len(host) == (len(SHAPES) if packed else len(SHAPES) * len(CLASSES))
    some = 0
    for path in host:
        assert sorted(host[path]) == sorted(dev[path]), path
        for k in host[path]:
            a, b = host[path][k], dev[path][k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (path, k)
            some += int(a.dtype == np.uint8 and a.any())
    assert some > 0, 'every saved mask is empty: the comparison shows nothing'


def test_refine_pseudo_labels_with_device_compress_writes_the_same_trees(tmp_path):
    """The pseudo-label tool on the case fixture of tests/golden/pseudo_labels.npz, with and without the flag: the `mask` files and the merged `_gt.npz`
    (key arr_0) load to the same arrays."""
    import json
    import yaml
    from rsuper_amd.tools import refine_pseudo_labels as tool
    G = np.load(os.path.join(ROOT, 'tests', 'golden', 'pseudo_labels.npz'))
    case = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'pseudo_labels.json')))['case']
    classes, raw = case['classes'], G['case_raw']
    cols = sorted({k for f in case['folders'] if f['row'] for k in f['row']})
    lines = ['BDMAP_ID,' + ','.join(cols)]
    root, organs_dir = tmp_path / 'in', tmp_path / 'organs'
    (organs_dir / 'list').mkdir(parents=True)
    organs = (np.random.default_rng(2).random((2,) + tuple(case['shape'])) < 0.5).astype(np.int8)
    (organs_dir / 'list' / 'label_names.yaml').write_text(yaml.safe_dump(['liver', 'kidney_left']))
    (tmp_path / 'labels.yaml').write_text(yaml.safe_dump(['liver_lesion', 'liver', 'kidney_lesion', 'kidney_left', 'pancreatic_lesion', 'colon_lesion']))
    for f in case['folders']:
        d = root / (f['id'] + '.npz') / 'predictions_raw'
        d.mkdir(parents=True)
        for c, name in enumerate(classes):
            np.save(d / (name + '.npy'), raw[c])
        if f['row'] is not None:
            lines.append(f['id'] + ',' + ','.join('' if f['row'].get(k, '') == 'NaN' else str(f['row'].get(k, '')) for k in cols))
        np.savez_compressed(organs_dir / (f['id'] + '_gt.npz'), organs[[1, 0]])
        np.savez_compressed(organs_dir / (f['id'] + '.npz'), np.zeros(case['shape'], np.float32))
    (tmp_path / 'meta.csv').write_text('\n'.join(lines) + '\n')
    trees, lists = {}, {}
    for flag in (False, True):
        out, tgt = tmp_path / f'out{int(flag)}', tmp_path / f'tgt{int(flag)}'
        lists[flag] = tool.main(['--input_dir', str(root), '--metadata', str(tmp_path / 'meta.csv'), '--out_npz_dir', str(out), '--label_list',
                                 str(tmp_path / 'labels.yaml'), '--organs_path', str(organs_dir), '--tgt_path', str(tgt)] + (['--device_compress'] if flag else []))
        trees[flag] = (load_tree(str(out)), {k: v for k, v in load_tree(str(tgt)).items() if k.endswith('_gt.npz')})
    assert lists[True] == lists[False] and lists[True][0]
    for host, dev in zip(trees[False], trees[True]):
        assert sorted(host) == sorted(dev) and host
        for path in host:
            assert sorted(host[path]) == sorted(dev[path]) and sorted(host[path]) in (['mask'], ['arr_0']), path
            for k in host[path]:
                assert host[path][k].dtype == dev[path][k].dtype and np.array_equal(host[path][k], dev[path][k]), (path, k)
