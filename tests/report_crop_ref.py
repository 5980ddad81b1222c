"""numpy-only restatement of the report-annotated crop's device work (csrc/crop_report.hip): no scipy, so that it runs wherever the tests do.

    union(packed, C, cset)              the voxels where any class of the 64-bit set is on, from an np.packbits(axis=0) label
    union_plain(lab, cset)              the same from a (C, D, H, W) label of 0 / non-zero bytes
    count_bbox(mask, add)               (count, [min z, y, x, max z, y, x]); no voxel: min = shape, max = -1 (what rsuper_union_bbox writes)
    to_bits(mask) / from_bits(bits, nx) (nz, ny, nx) <-> (nz, ny, ceil(nx / 64)) uint64 words, bit i of word k = voxel 64 k + i
    erode / dilate / opening            scipy's binary_erosion / binary_dilation with the default cross and border_value = 0, iterated; opening =
                                        dilate(erode(m, r), r) & m
    denoise_mask(mask, r, cc)           the reference's denoise_mask (training/augmentation.py:746): opening, then the largest component, ties to
                                        the first in C order; nothing left -> all zero
    remap(packed, C_in, C_out, masks, ones)   one remapped volume: class j = (the voxel's classes & masks[j]) != 0 or bit j of ones, np.packbits again
"""
import numpy as np

import postprocess_ref as PR


def unpack(packed, C):
    return np.unpackbits(np.asarray(packed), axis=0)[:C].astype(bool)


def union(packed, C, cset):
    lab = unpack(packed, C)
    m = np.zeros(lab.shape[1:], bool)
    for c in range(C):
        if cset >> c & 1:
            m |= lab[c]
    return m


def union_plain(lab, cset):
    m = np.zeros(lab.shape[1:], bool)
    for c in range(lab.shape[0]):
        if cset >> c & 1:
            m |= lab[c] != 0
    return m


def count_bbox(mask, add=(0, 0, 0)):
    mask = np.asarray(mask) != 0
    n = int(mask.sum())
    if n == 0:
        return 0, [s + a for s, a in zip(mask.shape, add)] + [a - 1 for a in add]
    idx = np.nonzero(mask)
    return n, [int(i.min()) + a for i, a in zip(idx, add)] + [int(i.max()) + a for i, a in zip(idx, add)]


def to_bits(mask):
    mask = np.asarray(mask) != 0
    nz, ny, nx = mask.shape
    nw = (nx + 63) // 64
    padded = np.zeros((nz, ny, nw * 64), np.uint8)
    padded[:, :, :nx] = mask
    return np.packbits(padded.reshape(nz, ny, nw, 64), axis=-1, bitorder='little').view('<u8').reshape(nz, ny, nw)


def from_bits(bits, nx):
    bits = np.ascontiguousarray(bits).view(np.uint64)
    nz, ny, nw = bits.shape
    b = np.unpackbits(bits.astype('<u8').view(np.uint8).reshape(nz, ny, nw * 8), axis=-1, bitorder='little')
    assert not b[:, :, nx:].any(), 'bits past nx must be zero'
    return b[:, :, :nx].astype(bool)


def _shifted(m, ax, step):
    """m moved by `step` along ax, zero filled."""
    out = np.zeros_like(m)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[ax], dst[ax] = slice(0, -1), slice(1, None)
    else:
        src[ax], dst[ax] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = m[tuple(src)]
    return out


def erode(m, r=1):
    m = np.asarray(m) != 0
    for _ in range(r):
        e = m.copy()
        for ax in range(3):
            e &= _shifted(m, ax, 1) & _shifted(m, ax, -1)
        m = e
    return m


def dilate(m, r=1):
    m = np.asarray(m) != 0
    for _ in range(r):
        d = m.copy()
        for ax in range(3):
            d |= _shifted(m, ax, 1) | _shifted(m, ax, -1)
        m = d
    return m


def opening(m, r):
    m = np.asarray(m) != 0
    return dilate(erode(m, r), r) & m


def denoise_mask(mask, iterations=2, connected_component=True):
    final = opening(mask, iterations)
    if not connected_component or not final.any():
        return final
    return PR.largest_component(final).astype(bool)


def remap(packed, C_in, C_out, masks, ones):
    lab = unpack(packed, C_in)
    out = np.zeros((C_out,) + lab.shape[1:], bool)
    for j in range(C_out):
        if ones >> j & 1:
            out[j] = True
        for c in range(C_in):
            if masks[j] >> c & 1:
                out[j] |= lab[c]
    return np.packbits(out, axis=0)
