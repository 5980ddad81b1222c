"""np.savez_compressed with the DEFLATE pass on the device (csrc/deflate.hip): the masks are compressed where they are and only the compressed bytes
are read back.  The files are what the reference writes and reads -- a ZIP of `.npy` members that `np.load(path)['arr_0']` opens.

A member is one raw DEFLATE stream:
    host    one stored block with the `.npy` header (np.lib.format.write_array_header_1_0): 00, LEN, ~LEN, the header bytes
    device  the stream of the payload (torch.ops.rsuper.deflate_planes): one byte-aligned fragment per chunk, then 01 00 00 FF FF
The CRC-32 of the member is folded from the header's (zlib.crc32) and the payload's (computed on the device) with crc32_combine.
The ZIP container is written with struct (zipfile cannot take compressed bytes): local header, data, central directory, end record; method 8, no ZIP64.

Everything but deflate_device's launch is host code and runs without a device: the code tables, the block header serialiser, crc32_combine, the `.npy`
header block and the ZIP writer."""
import heapq
import io
import struct
import zlib

import numpy as np

MAX_MEMBER = (1 << 32) - 1            # no ZIP64: sizes and offsets are 32-bit
MAX_PITCH = 32768

_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258 (RFC 1951 3.2.5)."""
    if not 3 <= length <= 258:
        raise ValueError(f'match length {length}')
    k = max(i for i, b in enumerate(_LEN_BASE) if b <= length)
    return 257 + k, _LEN_EXTRA[k], length - _LEN_BASE[k]


def distance_symbol(dist):
    """(symbol, extra bits, extra value) of a match distance 1..32768."""
    if not 1 <= dist <= 32768:
        raise ValueError(f'match distance {dist}')
    k = max(i for i, b in enumerate(_DIST_BASE) if b <= dist)
    return k, _DIST_EXTRA[k], dist - _DIST_BASE[k]


# ---- CRC-32 of a concatenation (zlib.crc32_combine, which Python 3.10 does not expose)
_POLY = 0xEDB88320


def _mulmod(a, b):
    """a(x) * b(x) modulo the CRC-32 polynomial, reflected bit order (bit 31 = x^0)."""
    p = 0
    for k in range(32):
        if a & (0x80000000 >> k):
            p ^= b
        b = (b >> 1) ^ _POLY if b & 1 else b >> 1
    return p


def _x2n_table():
    t, p = [], 0x40000000
    for _ in range(32):
        t.append(p)
        p = _mulmod(p, p)
    return t


_X2N = _x2n_table()
_SHIFT_OPS = {}


def crc_shift_operator(nbytes):
    """x^(8 * nbytes) modulo the polynomial: the operator that moves a CRC past nbytes more bytes (kept per length: chunk lengths repeat)."""
    op = _SHIFT_OPS.get(nbytes)
    if op is None:
        op, n, k = 0x80000000, nbytes, 3
        while n:
            if n & 1:
                op = _mulmod(_X2N[k & 31], op)
            n >>= 1
            k += 1
        if len(_SHIFT_OPS) < 64:
            _SHIFT_OPS[nbytes] = op
    return op


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B)."""
    return _mulmod(crc_shift_operator(len_b), crc_a & 0xFFFFFFFF) ^ (crc_b & 0xFFFFFFFF)


def crc32_of_chunks(crcs, lengths):
    crc = 0
    for c, n in zip(crcs, lengths):
        crc = crc32_combine(crc, c, n)
    return crc


# ---- Huffman code tables
def canonical_codes(lengths):
    """RFC 1951 3.2.2: the codes of a list of code lengths (0 = the symbol has no code)."""
    maxb = max(lengths)
    count = [0] * (maxb + 2)
    for b in lengths:
        if b:
            count[b] += 1
    code, nxt = 0, [0] * (maxb + 2)
    for b in range(1, maxb + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for b in lengths:
        out.append(nxt[b] if b else 0)
        if b:
            nxt[b] += 1
    return out


def huffman_lengths(weights, limit):
    """Code lengths of a Huffman code for positive integer weights, every symbol coded, no length above `limit`: the weights are halved (kept >= 1) until the
    tree is shallow enough.  Ties are broken by the lowest symbol in the subtree, so the result is a function of the weights."""
    w = list(weights)
    if len(w) < 2 or min(w) < 1:
        raise ValueError('huffman_lengths needs two or more symbols with positive weights')
    while True:
        heap = [(x, i, (i,)) for i, x in enumerate(w)]
        heapq.heapify(heap)
        lens = [0] * len(w)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(lens) <= limit:
            return lens
        w = [max(1, x // 2) for x in w]


def _reverse(code, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


class _BitSink:
    """LSB-first bit string as a Python int."""

    def __init__(self):
        self.value, self.bits = 0, 0

    def put(self, v, n):
        self.value |= (v & ((1 << n) - 1)) << self.bits
        self.bits += n

    def put_code(self, code, n):
        self.put(_reverse(code, n), n)


class DeflateTable:
    """The encoder's argument: code lengths and codes of the 286 literal/length and 30 distance symbols, and the bits that open a block."""

    def __init__(self, name, ll_lengths, d_lengths, header_value, header_bits):
        if len(ll_lengths) != 286 or len(d_lengths) != 30:
            raise ValueError('a table has 286 literal/length and 30 distance symbols')
        if min(ll_lengths) < 1 or min(d_lengths) < 1 or max(ll_lengths) > 15 or max(d_lengths) > 15:
            raise ValueError('every symbol needs a code of 1..15 bits: the encoder may meet any byte and any length')
        self.name = name
        self.ll_lengths, self.d_lengths = tuple(ll_lengths), tuple(d_lengths)
        self.header_value, self.header_bits = header_value, header_bits

    def set_codes(self, ll_codes, d_codes):
        self.ll_codes, self.d_codes = tuple(ll_codes), tuple(d_codes)
        return self

    def words(self):
        """316 uint32: (bits << 24) | bit-reversed code, as csrc/deflate.hip reads them."""
        w = [(b << 24) | _reverse(c, b) for c, b in zip(self.ll_codes + self.d_codes, self.ll_lengths + self.d_lengths)]
        return np.array(w, dtype=np.uint32)

    def header_words(self):
        n = (self.header_bits + 31) // 32
        return np.array([(self.header_value >> (32 * k)) & 0xFFFFFFFF for k in range(n)], dtype=np.uint32)


def fixed_table():
    """BTYPE 01: the fixed code of RFC 1951 3.2.6 (its 286 / 30 usable symbols); the header is BFINAL = 0, BTYPE = 01."""
    ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    d = [5] * 32
    t = DeflateTable('fixed', ll[:286], d[:30], 0b010, 3)
    return t.set_codes(canonical_codes(ll)[:286], canonical_codes(d)[:30])


def _code_length_runs(lengths):
    """The code-length sequence with symbol 16 ("repeat the previous length 3..6 times"); every length is > 0, so 17 and 18 never apply."""
    out, i = [], 0
    while i < len(lengths):
        v = lengths[i]
        out.append((v, 0, 0))
        j = i + 1
        while j < len(lengths) and lengths[j] == v:
            j += 1
        run = j - i - 1
        while run >= 3:
            r = min(run, 6)
            out.append((16, 2, r - 3))
            run -= r
        out.extend([(v, 0, 0)] * run)
        i = j
    return out


def dynamic_header(ll_lengths, d_lengths):
    """(value, bits) of BFINAL = 0, BTYPE = 10 and the code lengths of RFC 1951 3.2.7 for the two alphabets."""
    seq = _code_length_runs(list(ll_lengths) + list(d_lengths))
    freq = [0] * 19
    for s, _, _ in seq:
        freq[s] += 1
    used = [s for s in range(19) if freq[s]]
    if len(used) < 2:
        raise ValueError('a dynamic header needs two or more distinct code lengths')
    cl = [0] * 19
    for s, b in zip(used, huffman_lengths([freq[s] for s in used], 7)):
        cl[s] = b
    cl_codes = canonical_codes(cl)
    hclen = max(k for k, s in enumerate(_CL_ORDER) if cl[s]) + 1
    o = _BitSink()
    o.put(0, 1)
    o.put(2, 2)
    o.put(len(ll_lengths) - 257, 5)
    o.put(len(d_lengths) - 1, 5)
    o.put(max(hclen, 4) - 4, 4)
    for s in _CL_ORDER[:max(hclen, 4)]:
        o.put(cl[s], 3)
    for s, eb, ev in seq:
        o.put_code(cl_codes[s], cl[s])
        o.put(ev, eb)
    return o.value, o.bits


def mask_table(pitch=0):
    """BTYPE 10 with one static code made for 0 / 1 bytes in runs and repeated rows: two bits each for the literals 0 and 1 and for length 258, one bit for
    distance 1 and two for the distance symbol of `pitch`; the other lengths next, the other literals and distances long.  The lengths come from a Huffman
    construction over fixed weights, so the code is complete (Kraft sum 1) by construction."""
    if not 0 <= pitch <= MAX_PITCH:
        raise ValueError(f'pitch {pitch} is outside 0..{MAX_PITCH}')
    wl = [16] * 286
    wl[0] = wl[1] = wl[285] = 8192
    for s in range(257, 285):
        wl[s] = 128
    wd = [16] * 30
    wd[0] = 8192
    if pitch >= 2:
        wd[distance_symbol(pitch)[0]] = max(wd[distance_symbol(pitch)[0]], 4096)
    ll, d = huffman_lengths(wl, 15), huffman_lengths(wd, 15)
    t = DeflateTable('mask', ll, d, *dynamic_header(ll, d))
    return t.set_codes(canonical_codes(ll), canonical_codes(d))


def make_table(table, pitch=0):
    if isinstance(table, DeflateTable):
        return table
    if table == 'fixed':
        return fixed_table()
    if table == 'mask':
        return mask_table(pitch)
    raise ValueError(f"table must be 'fixed', 'mask' or a DeflateTable, got {table!r}")


# ---- the host's share of a member and the containers
def stored_block(data, final=False):
    """One stored block; it starts and ends on a byte boundary."""
    if len(data) > 65535:
        raise ValueError('a stored block holds up to 65535 bytes')
    return bytes([1 if final else 0]) + struct.pack('<HH', len(data), len(data) ^ 0xFFFF) + bytes(data)


CLOSING_BLOCK = stored_block(b'', final=True)


def deflate_bound(n, chunk):
    """rsuper_deflate_bound on the host: every chunk stored (five bytes each) and the closing block."""
    return n + 5 * ((n + chunk - 1) // chunk) + 5


def npy_header(shape, dtype):
    """The bytes np.save writes in front of the data of a C-ordered array (format version 1.0)."""
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, {'descr': np.lib.format.dtype_to_descr(np.dtype(dtype)), 'fortran_order': False, 'shape': tuple(shape)})
    return f.getvalue()


def npy_member(shape, dtype, stream, payload_crc, payload_bytes):
    """(compressed bytes, CRC-32, uncompressed size) of a `.npy` member whose payload stream (closing block included) came from the device."""
    head = npy_header(shape, dtype)
    return stored_block(head) + stream, crc32_combine(zlib.crc32(head), payload_crc, payload_bytes), len(head) + payload_bytes


def host_member(array):
    """The same for a host array, deflated by zlib (small members: class names, ids)."""
    f = io.BytesIO()
    np.lib.format.write_array(f, np.asanyarray(array), allow_pickle=False)
    raw = f.getvalue()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(raw) + c.flush(), zlib.crc32(raw), len(raw)


def write_zip(file, members):
    """members: [(name, compressed bytes, CRC-32, uncompressed size)], all method 8 (raw DEFLATE).  `file`: a path or a binary file object."""
    own = isinstance(file, (str, bytes)) or hasattr(file, '__fspath__')
    f = open(file, 'wb') if own else file
    try:
        central, pos = [], 0
        for name, data, crc, usize in members:
            nm = name.encode('utf-8')
            if max(len(data), usize, pos) > MAX_MEMBER:
                raise ValueError(f'{name}: a member or archive of 4 GiB or more needs ZIP64, which this writer does not produce')
            flags = 0x800 if any(b > 127 for b in nm) else 0
            f.write(struct.pack('<IHHHHHIIIHH', 0x04034B50, 20, flags, 8, 0, 0x21, crc, len(data), usize, len(nm), 0) + nm)
            f.write(data)
            central.append(struct.pack('<IHHHHHHIIIHHHHHII', 0x02014B50, 20, 20, flags, 8, 0, 0x21, crc, len(data), usize, len(nm), 0, 0, 0, 0, 0, pos) + nm)
            pos += 30 + len(nm) + len(data)
        if pos > MAX_MEMBER or len(members) > 65535:
            raise ValueError('the archive needs ZIP64, which this writer does not produce')
        cd = b''.join(central)
        f.write(cd)
        f.write(struct.pack('<IHHHHIIH', 0x06054B50, 0, 0, len(members), len(members), len(cd), pos, 0))
    finally:
        if own:
            f.close()


def _npz_path(path):
    path = str(path)
    return path if path.endswith('.npz') else path + '.npz'


# ---- the device call
_DEVICE_TABLES = {}
_OP = None


def _deflate_planes_impl(src, n, plane_stride, planes, pitch, table, header, header_bits):
    """The C ABI call: src one-byte device storage holding `planes` planes of n bytes plane_stride apart -> (out bytes, meta (3, planes) int64: offsets, sizes
    and CRCs (as uint32 pairs in the third row))."""
    import torch
    from ..hip import lib as _l
    if not src.is_cuda or not table.is_cuda or not header.is_cuda:
        raise _l.RSuperHipError('deflate_planes needs device tensors (no CPU fallback)')
    if src.element_size() != 1 or not src.is_contiguous() or planes < 1 or n < 0 or plane_stride < n or (planes - 1) * plane_stride + n > src.numel():
        raise ValueError('deflate_planes: src must be contiguous one-byte storage that holds `planes` planes of n bytes plane_stride apart')
    if table.numel() != 316 or table.element_size() != 4 or header.element_size() != 4 or header.numel() * 32 < header_bits:
        raise ValueError('deflate_planes: the table has 316 words and the header holds header_bits bits')
    L = _l.lib()
    out = torch.empty(planes * L.rsuper_deflate_bound(n), device=src.device, dtype=torch.uint8)
    meta = torch.zeros((3, planes), device=src.device, dtype=torch.int64)
    ws = torch.empty(max(L.rsuper_deflate_workspace_bytes(planes, n), 16), device=src.device, dtype=torch.uint8)
    with torch.cuda.device(src.device):
        _l.check(L.rsuper_deflate_planes(src.data_ptr(), plane_stride, n, planes, pitch, table.data_ptr(), header.data_ptr(), header_bits, out.data_ptr(),
                                         meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(), ws.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), 'deflate_planes')
    return out, meta


def _op():
    global _OP
    if _OP is None:
        from ..hip import ops as _ops          # noqa: F401  (hip/ops.py pulls in hip/library.py; this order avoids the import cycle)
        from ..hip import library as _library
        _OP = _library.install_deflate_ops(_deflate_planes_impl)
    return _OP


def _device_table(t, device):
    import torch
    key = (t.name, t.ll_lengths, t.d_lengths, t.header_value, str(device))
    got = _DEVICE_TABLES.get(key)
    if got is None:
        got = (torch.from_numpy(t.words().view(np.int32)).to(device), torch.from_numpy(t.header_words().view(np.int32)).to(device))
        if len(_DEVICE_TABLES) < 32:
            _DEVICE_TABLES[key] = got
    return got


def _as_planes(stack):
    """(one-byte contiguous device tensor, planes, bytes per plane) of a bool / uint8 / int8 stack whose first axis counts the planes."""
    import torch
    from ..hip import lib as _l
    if not isinstance(stack, torch.Tensor) or not stack.is_cuda:
        raise _l.RSuperHipError('the device encoder needs a device tensor (no CPU fallback)')
    if stack.dtype not in (torch.uint8, torch.bool, torch.int8) or stack.dim() < 1:
        raise ValueError(f'the device encoder takes bool / uint8 / int8 tensors, got {stack.dtype}')
    v = stack.contiguous()
    if v.dtype != torch.uint8:
        v = v.view(torch.uint8)
    planes = v.shape[0]
    n = v[0].numel() if planes else 0
    if n > MAX_MEMBER:
        raise ValueError('a plane of 4 GiB or more does not fit a ZIP member without ZIP64')
    return v, planes, n


def deflate_strided(storage, n, plane_stride, planes, pitch=0, table='fixed', timings=None):
    """deflate_device for planes that lie plane_stride >= n bytes apart in a flat one-byte device tensor (any alignment): plane p = storage[p * plane_stride:
    p * plane_stride + n].  1 <= planes <= 65535."""
    import time
    import torch
    if not 0 <= pitch <= MAX_PITCH:
        raise ValueError(f'pitch {pitch} is outside 0..{MAX_PITCH}')
    t = make_table(table, pitch)
    words, header = _device_table(t, storage.device)
    t0 = time.perf_counter()
    out, meta = _op()(storage, n, plane_stride, planes, pitch, words, header, t.header_bits)
    if timings is not None:
        torch.cuda.synchronize(storage.device)
        timings['kernel'] = timings.get('kernel', 0.0) + time.perf_counter() - t0
        t0 = time.perf_counter()
    m = meta.cpu().numpy()                                         # read 1: offsets, sizes, CRCs
    off, size, crc = m[0], m[1], m[2].view(np.uint32)[:planes]
    host = out[:int(off[-1] + size[-1])].cpu().numpy().tobytes()   # read 2: the compressed bytes
    if timings is not None:
        timings['readback'] = timings.get('readback', 0.0) + time.perf_counter() - t0
    return [host[int(o):int(o + k)] for o, k in zip(off, size)], [int(c) for c in crc]


def deflate_device(stack_u8, pitch=None, table='fixed', timings=None):
    """One raw DEFLATE stream per plane stack_u8[p] (closing block included, the host's `.npy` header block not) and the CRC-32 of every plane:
    (list of bytes, list of int).  pitch: the row length for "same as the row above" matches, None = the last axis of a stack with two or more axes per
    plane, 0 = runs only.  table: 'fixed', 'mask' or a DeflateTable.  Two device-to-host reads: sizes and CRCs, then the compressed bytes.
    timings: a dict that receives the seconds of the 'kernel' and 'readback' stages (one extra synchronisation)."""
    v, planes, n = _as_planes(stack_u8)
    if pitch is None:
        pitch = _row_pitch(v[0]) if planes else 0
    streams, crcs = [], []
    for p0 in range(0, planes, 65535):
        part = v[p0:p0 + 65535]
        s, c = deflate_strided(part.reshape(-1), n, n, part.shape[0], pitch, table, timings)
        streams += s
        crcs += c
    return streams, crcs


def _row_pitch(a):
    """The row length of an array with two or more axes, 0 (runs only) otherwise or when a row is longer than a match can reach."""
    return a.shape[-1] if a.dim() >= 2 and a.shape[-1] <= MAX_PITCH else 0


def _is_device_tensor(a):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(a, torch.Tensor) and a.is_cuda


def _np_dtype(t):
    import torch
    return {torch.uint8: np.uint8, torch.bool: np.bool_, torch.int8: np.int8}[t.dtype]


def savez_compressed_device(path, *arrays, table='fixed', **named):
    """np.savez_compressed(path, *arrays, **named) where device bool / uint8 / int8 tensors are deflated on the device (rows = the last axis) and host
    arrays by zlib.  The file loads with np.load.  A tensor of 4 GiB or more raises ValueError (no ZIP64): keep np.savez_compressed for those."""
    items = [('arr_%d' % k, a) for k, a in enumerate(arrays)]
    for k, a in named.items():
        if k in dict(items):
            raise ValueError(f'Cannot use un-named variables and keyword {k}')
        items.append((k, a))
    members = []
    for key, a in items:
        if _is_device_tensor(a):
            if a.numel() > MAX_MEMBER:
                raise ValueError(f'{key}: a tensor of 4 GiB or more does not fit a ZIP member without ZIP64')
            (stream,), (crc,) = deflate_device(a.reshape((1,) + tuple(a.shape)), pitch=_row_pitch(a), table=table)
            members.append((key + '.npy',) + npy_member(tuple(a.shape), _np_dtype(a), stream, crc, a.numel()))
        else:
            members.append((key + '.npy',) + host_member(a))
    write_zip(_npz_path(path), members)


def save_planes_npz(paths, stack, key='arr_0', table='fixed', timings=None):
    """One `.npz` per plane of the device stack (P, ...), member `<key>.npy` = stack[p], from one device call."""
    import time
    v, planes, n = _as_planes(stack)
    if len(paths) != planes:
        raise ValueError(f'{len(paths)} paths for {planes} planes')
    streams, crcs = deflate_device(stack, table=table, timings=timings)
    t0 = time.perf_counter()
    for path, stream, crc in zip(paths, streams, crcs):
        write_zip(_npz_path(path), [(key + '.npy',) + npy_member(tuple(stack.shape[1:]), _np_dtype(stack), stream, crc, n)])
    if timings is not None:
        timings['file'] = timings.get('file', 0.0) + time.perf_counter() - t0


def gzip_member(stream, crc, size):
    """The bytes of a .gz file around a raw DEFLATE stream of `size` bytes with CRC-32 `crc`: 10-byte header, the stream, CRC-32 and size."""
    return b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff' + stream + struct.pack('<II', crc, size & 0xFFFFFFFF)


def gzip_device(tensor, table='fixed'):
    """The bytes of a .gz file of the tensor's bytes (gzip.decompress gives them back): 10-byte header, the device stream, CRC-32 and size."""
    (stream,), (crc,) = deflate_device(tensor.reshape((1,) + tuple(tensor.shape)), pitch=_row_pitch(tensor), table=table)
    return gzip_member(stream, crc, tensor.numel())


def gzip_planes_device(storage, n, plane_stride, planes, pitch=0, table='fixed'):
    """gzip_device for `planes` byte planes of n bytes lying plane_stride apart in flat one-byte device storage: one .gz file's bytes per plane from one
    device call (deflate_strided)."""
    streams, crcs = deflate_strided(storage, n, plane_stride, planes, pitch, table)
    return [gzip_member(s, c, n) for s, c in zip(streams, crcs)]
