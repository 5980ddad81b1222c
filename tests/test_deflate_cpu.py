"""The host side of the device DEFLATE path (inference/npz_writer.py) and the restatement tests/deflate_ref.py that the GPU tests compare the device
bytes with.  zlib's inflater, np.load and zipfile are the oracles.  No GPU needed."""
import io
import os
import sys
import zipfile
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import deflate_ref as R  # noqa: E402
from rsuper_amd.inference import npz_writer as nw  # noqa: E402

TABLES = ('fixed', 'mask')
S, C = R.SEG, R.CHUNK


def ball40():
    z, y, x = np.mgrid[:40, :40, :40]
    return ((z - 20) ** 2 + (y - 19) ** 2 + (x - 21) ** 2 < 15 ** 2).astype(np.uint8)


def content_classes():
    r = np.random.default_rng(1)
    n = C + 1000
    ball = ball40()
    return {'zeros': (np.zeros(n, np.uint8), 0), 'ones': (np.ones(n, np.uint8), 0), 'ff': (np.full(n, 255, np.uint8), 0),
            'alternating': ((np.arange(n) & 1).astype(np.uint8), 0), 'random': (r.integers(0, 256, n, dtype=np.uint8), 0),
            'runs': (np.concatenate([np.full(k, k & 1, np.uint8) for k in range(1, 601)]), 0),
            'ball': (ball.ravel(), 40), 'ball_packed': (np.packbits(ball.ravel()), 5), 'empty': (np.zeros(0, np.uint8), 0)}


@pytest.mark.parametrize('table', TABLES)
@pytest.mark.parametrize('name', sorted(content_classes()))
def test_restatement_round_trips_through_zlib(name, table):
    x, pitch = content_classes()[name]
    for p in sorted({0, pitch}):
        s = R.stream(x.tobytes(), p, table)
        assert zlib.decompress(s, wbits=-15) == x.tobytes()
        assert len(s) <= nw.deflate_bound(len(x), C)
        assert s.endswith(nw.CLOSING_BLOCK)


def test_parse_rule():
    """The longer candidate wins, distance 1 on a tie; 1 or 2 bytes left are literals; matches stop at segment boundaries; no row above in the first row."""
    assert R.tokens(b'\x07' * 10) == [('lit', 7), ('match', 9, 1)]
    assert R.tokens(b'\x07' * 3) == [('lit', 7), ('lit', 7), ('lit', 7)]                    # two bytes left after the first
    assert R.tokens(b'\x07' * 4) == [('lit', 7), ('match', 3, 1)]
    assert R.tokens(b'\x07' * 260) == [('lit', 7), ('match', 258, 1), ('lit', 7)]
    row = bytes(range(8))
    assert R.tokens(row * 3, 8) == [('lit', b) for b in row] + [('match', 16, 8)]
    assert R.tokens(bytes(8) * 2, 8) == [('lit', 0), ('match', 15, 1)]                      # tie -> distance 1
    assert R.tokens(row[:5], 8) == [('lit', b) for b in row[:5]]                            # shorter than a row
    t = R.tokens(bytes(S + 10))
    assert t == [('lit', 0), ('match', 258, 1), ('match', 257, 1), ('match', 10, 1)]        # cut at the segment, and a match may start a segment
    assert R.tokens(bytes(C + 4))[-1] == ('match', 4, 1)                                    # ... and a chunk


def test_zip_writer_round_trips_through_numpy_and_zipfile(tmp_path):
    ball = ball40()
    names = np.array(['liver', 'pancreas'])
    path = str(tmp_path / 'two.npz')
    members = []
    for key, a, pitch in (('arr_0', ball, 40), ('mask', ball[3].astype(bool), 40), ('empty', np.zeros((0, 4), np.uint8), 4)):
        raw = a.tobytes()
        members.append((key + '.npy',) + nw.npy_member(a.shape, a.dtype, R.stream(raw, pitch, 'mask'), zlib.crc32(raw), len(raw)))
    members.append(('classes.npy',) + nw.host_member(names))
    nw.write_zip(path, members)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None and z.namelist() == ['arr_0.npy', 'mask.npy', 'empty.npy', 'classes.npy']
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())
    with np.load(path) as z:
        assert np.array_equal(z['arr_0'], ball) and z['arr_0'].dtype == np.uint8
        assert np.array_equal(z['mask'], ball[3].astype(bool)) and z['mask'].dtype == np.bool_
        assert z['empty'].shape == (0, 4) and list(z['classes']) == ['liver', 'pancreas']
    single = io.BytesIO()
    nw.write_zip(single, members[:1])
    assert np.array_equal(np.load(io.BytesIO(single.getvalue()))['arr_0'], ball)
    with pytest.raises(ValueError):
        nw.write_zip(io.BytesIO(), [('big.npy', b'', 0, 1 << 32)])                          # 4 GiB needs ZIP64


def test_npy_header_block_is_what_numpy_writes():
    for shape, dt in (((5, 12, 10, 14), np.uint8), ((0,), np.bool_), ((3,), np.int8)):
        f = io.BytesIO()
        np.save(f, np.zeros(shape, dt))
        head = nw.npy_header(shape, dt)
        assert f.getvalue()[:len(head)] == head and len(f.getvalue()) == len(head) + int(np.prod(shape))
        blk = nw.stored_block(head)
        assert blk[0] == 0 and zlib.decompress(blk + nw.CLOSING_BLOCK, wbits=-15) == head


def test_crc_combine():
    r = np.random.default_rng(2)
    data = r.integers(0, 256, 3 * C + 77, dtype=np.uint8).tobytes()
    for chunks in ([data[:C], data[C:2 * C], data[2 * C:3 * C], data[3 * C:]], [data[:5], b'', data[5:9]], [b''], [], [b'', data[:1]]):
        whole = b''.join(chunks)
        assert nw.crc32_of_chunks([zlib.crc32(c) for c in chunks], [len(c) for c in chunks]) == zlib.crc32(whole)
    head = b'\x93NUMPY header'
    assert nw.crc32_combine(zlib.crc32(head), 0, 0) == zlib.crc32(head)                     # an empty payload
    assert nw.crc32_combine(zlib.crc32(head), zlib.crc32(data), len(data)) == zlib.crc32(head + data)
    assert nw.crc32_combine(0, zlib.crc32(data), len(data)) == zlib.crc32(data)


@pytest.mark.parametrize('pitch', (0, 1, 2, 40, 192, 193, 32768))
def test_tables(pitch):
    """Both tables code all 286 + 30 symbols; the mask table's lengths are complete codes (Kraft sum exactly 1) and its header inflates."""
    for t in (nw.fixed_table(), nw.mask_table(pitch)):
        assert len(t.ll_lengths) == 286 and len(t.d_lengths) == 30 and min(t.ll_lengths + t.d_lengths) >= 1 and max(t.ll_lengths + t.d_lengths) <= 15
        w = t.words()
        assert w.dtype == np.uint32 and w.shape == (316,) and ((w >> 24) == np.array(t.ll_lengths + t.d_lengths)).all()
        for lens, codes in ((t.ll_lengths, t.ll_codes), (t.d_lengths, t.d_codes)):          # prefix-free: canonical codes of distinct symbols differ
            assert len({(b, c) for b, c in zip(lens, codes)}) == len(lens) and all(c < (1 << b) for b, c in zip(lens, codes))
        # the header, the end-of-block code and the closing block alone are a valid stream of no bytes
        assert zlib.decompress(R.coded_fragment([], t) + nw.CLOSING_BLOCK, wbits=-15) == b''
        every = bytes(range(256)) * 2
        assert zlib.decompress(R.coded_fragment([('lit', b) for b in every], t) + nw.CLOSING_BLOCK, wbits=-15) == every
    m = nw.mask_table(pitch)
    assert sum(1 << (15 - b) for b in m.ll_lengths) == 1 << 15 and sum(1 << (15 - b) for b in m.d_lengths) == 1 << 15
    assert m.ll_lengths[0] <= 2 and m.ll_lengths[1] <= 2 and m.ll_lengths[285] <= 2 and m.d_lengths[0] == 1
    if pitch >= 2:
        assert m.d_lengths[nw.distance_symbol(pitch)[0]] <= 2
    assert m.header_bits <= 4096 and m.header_words().shape == ((m.header_bits + 31) // 32,)


def test_a_symbol_without_a_code_is_refused():
    f = nw.fixed_table()
    ll = list(f.ll_lengths)
    ll[200] = 0
    with pytest.raises(ValueError):
        nw.DeflateTable('holes', ll, f.d_lengths, 0b010, 3)
    with pytest.raises(ValueError):
        nw.DeflateTable('short', f.ll_lengths[:285], f.d_lengths, 0b010, 3)
    with pytest.raises(ValueError):
        nw.mask_table(32769)
    with pytest.raises(ValueError):
        nw.make_table('dynamic')
    with pytest.raises(ValueError):
        nw.length_symbol(259)
    with pytest.raises(ValueError):
        nw.distance_symbol(32769)
    assert [nw.length_symbol(v) for v in (3, 10, 11, 257, 258)] == [(257, 0, 0), (264, 0, 0), (265, 1, 0), (284, 5, 30), (285, 0, 0)]
    assert [nw.distance_symbol(v) for v in (1, 4, 5, 24577, 32768)] == [(0, 0, 0), (3, 0, 0), (4, 1, 0), (29, 13, 0), (29, 13, 8191)]


def test_bound():
    """rsuper_deflate_bound(n) <= n + n / 1024 + 64 for every n: five bytes per chunk and five to close; the library and the host restatement agree."""
    from rsuper_amd.hip import lib
    L = lib.lib()
    assert L.rsuper_deflate_chunk_bytes() == C and L.rsuper_deflate_segment_bytes() == S
    ns = list(range(0, 3000)) + [k * C + d for k in (1, 2, 3, 100, 4097, 130055) for d in (-1, 0, 1)] + [(1 << 32) - 1, 1 << 31]
    for n in ns:
        b = L.rsuper_deflate_bound(n)
        assert b == nw.deflate_bound(n, C) and b <= n + n // 1024 + 64, n
    # exact for the worst input: one stored block per chunk
    x = np.random.default_rng(4).integers(0, 256, 2 * C + 9, dtype=np.uint8).tobytes()
    assert len(R.stream(x, 0, 'fixed')) == L.rsuper_deflate_bound(len(x))
    assert L.rsuper_deflate_workspace_bytes(3, 2 * C + 9) >= 3 * 3 * (C + 5)


def test_new_symbols_are_declared_and_bound():
    import re
    from rsuper_amd.hip import lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read(), flags=re.S)
    for name, arity in {'rsuper_deflate_bound': 1, 'rsuper_deflate_workspace_bytes': 2, 'rsuper_deflate_chunk_bytes': 0, 'rsuper_deflate_segment_bytes': 0,
                        'rsuper_deflate_planes': 14}.items():
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/rsuper_hip.h'
        assert len([p for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']) == arity == len(lib._SIGS[name][1]), name
        assert hasattr(lib.lib(), name)


def test_device_entry_points_refuse_host_tensors():
    import torch
    from rsuper_amd.inference import deflate_device, savez_compressed_device, save_planes_npz, gzip_device  # noqa: F401  (re-exported)
    with pytest.raises(Exception):
        deflate_device(torch.zeros((2, 8), dtype=torch.uint8))
    with pytest.raises(Exception):
        gzip_device(torch.zeros((2, 8), dtype=torch.uint8))
