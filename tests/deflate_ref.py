"""Pure-Python restatement of the device DEFLATE encoder (r-super_amd/csrc/deflate.hip): the same chunks, segments, greedy parse and code tables, so that a
test can pin WHICH valid stream the device produces.  Whether a stream is valid is zlib's inflater's to say, not this module's.

    stream(x, pitch, table)  the bytes rsuper_deflate_planes gives for the plane x (closing block included)
    tokens(x, pitch)         the parse alone: ('lit', byte) / ('match', length, distance)

CHUNK and SEG are the geometry the C ABI reports (rsuper_deflate_chunk_bytes / rsuper_deflate_segment_bytes); test_gpu_deflate.py checks that they agree."""
import numpy as np

from rsuper_amd.inference import npz_writer as nw

SEG = 516
CHUNK = 64 * SEG


def _run_lengths(x, d):
    """r[i] = number of k >= 0 with x[i + k] == x[i + k - d] for all positions up to k (0 for i < d), unbounded."""
    n = len(x)
    r = np.zeros(n, dtype=np.int64)
    if d < 1 or n <= d:
        return r
    eq = x[d:] == x[:-d]
    idx = np.arange(len(eq))
    stop = np.where(eq, len(eq), idx)
    stop = np.minimum.accumulate(stop[::-1])[::-1]          # the next position at or after j where the bytes differ
    r[d:] = stop - idx
    return r


def tokens_of_range(x, r1, rp, pitch, lo, hi):
    """The greedy parse of the segment [lo, hi) of the plane x."""
    out, i = [], lo
    while i < hi:
        lim = min(hi - i, 258)
        l1 = min(int(r1[i]), lim)
        lp = min(int(rp[i]), lim) if pitch >= 2 else 0
        L = max(l1, lp)
        if L >= 3:
            out.append(('match', L, 1 if l1 >= lp else pitch))
            i += L
        else:
            out.append(('lit', int(x[i])))
            i += 1
    return out


def tokens(x, pitch=0):
    x = np.frombuffer(bytes(x), dtype=np.uint8)
    r1, rp = _run_lengths(x, 1), _run_lengths(x, pitch if pitch >= 2 else 0)
    out = []
    for lo in range(0, len(x), CHUNK):
        for s in range(lo, min(lo + CHUNK, len(x)), SEG):
            out += tokens_of_range(x, r1, rp, pitch, s, min(s + SEG, lo + CHUNK, len(x)))
    return out


def _rev(code, bits):
    return int(format(code, '0%db' % bits)[::-1], 2) if bits else 0


def _pack(values, nbits):
    """LSB-first concatenation of values[k] in nbits[k] bits -> (bytes padded with zero bits, number of bits)."""
    v = np.array(values, dtype=np.uint64)
    nb = np.array(nbits, dtype=np.int64)
    k = np.arange(64, dtype=np.uint64)
    bits = ((v[:, None] >> k[None, :]) & np.uint64(1)).astype(np.uint8)
    keep = k[None, :].astype(np.int64) < nb[:, None]
    flat = bits[keep]
    return np.packbits(flat, bitorder='little').tobytes(), int(nb.sum())


def coded_fragment(toks, table):
    """Header bits, tokens, end-of-block code; then the empty stored block that returns to a byte boundary."""
    values, nbits = [], []
    hv, hb = table.header_value, table.header_bits
    while hb > 0:
        values.append(hv & 0xFFFFFFFF)
        nbits.append(min(hb, 32))
        hv >>= 32
        hb -= 32
    for t in toks:
        if t[0] == 'lit':
            b = table.ll_lengths[t[1]]
            values.append(_rev(table.ll_codes[t[1]], b))
            nbits.append(b)
        else:
            ls, leb, lev = nw.length_symbol(t[1])
            ds, deb, dev = nw.distance_symbol(t[2])
            lb, db = table.ll_lengths[ls], table.d_lengths[ds]
            v = _rev(table.ll_codes[ls], lb) | (lev << lb)
            v |= (_rev(table.d_codes[ds], db) | (dev << db)) << (lb + leb)
            values.append(v)
            nbits.append(lb + leb + db + deb)
    values.append(_rev(table.ll_codes[256], table.ll_lengths[256]))
    nbits.append(table.ll_lengths[256])
    values.append(0)
    nbits.append(3)
    body, _ = _pack(values, nbits)
    return body + b'\x00\x00\xff\xff'


def stream(x, pitch=0, table='fixed'):
    x = bytes(x)
    table = nw.make_table(table, pitch)
    a = np.frombuffer(x, dtype=np.uint8)
    r1, rp = _run_lengths(a, 1), _run_lengths(a, pitch if pitch >= 2 else 0)
    out = []
    for lo in range(0, len(x), CHUNK):
        hi = min(lo + CHUNK, len(x))
        toks = []
        for s in range(lo, hi, SEG):
            toks += tokens_of_range(a, r1, rp, pitch, s, min(s + SEG, hi))
        coded = coded_fragment(toks, table)
        stored = nw.stored_block(x[lo:hi])
        out.append(coded if len(coded) <= len(stored) else stored)
    out.append(nw.CLOSING_BLOCK)
    return b''.join(out)
