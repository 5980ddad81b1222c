#!/usr/bin/env python3
"""Device times of the NIfTI -> packed-case conversion (dataset_conversion/nii_dataset.py, csrc/nii_dataset.hip) on a synthetic hospital case made in
memory from a seed: a 512 x 512 x 300 int16 CT at 0.8 x 0.8 x 2.5 mm with 26 uint8 masks, resampled to 1 mm -> a (750, 410, 410) box, four byte planes.

    image                 load_nifti_device + rsuper_ct_stats + rsuper_ct_normalize_pop of the CT (device events; includes the allocations)
    upload_group          the raw bytes of one group of eight masks, pageable host memory -> device (host clock + synchronise)
    gather_identity       one rsuper_label_gather_pack launch: eight masks stored in the CT's voxel order (unit stride = canonical x)
    gather_permuted       the same masks stored with the axes permuted (unit stride = canonical z): the strided read, not tiled through LDS
    gather_label_map      label-map mode: one int16 map, a 35-value table, all four planes in one launch
    background            rsuper_label_background over the box
    pack_bits             the existing rsuper_pack_bits on an unpacked (8, Do, Ho, Wo) volume of the SAME output volume, in the same call: the
                          comparable streaming kernel (reads 8 V, writes V)
    gunzip_host           gzip.decompress of one mask file's bytes on one host thread, and that time x 26 (host clock): expected to bound a case
    numpy_restatement     tests/nii_dataset_ref.py on eight of the masks (reorient, three nearest tables, stack, pad, astype(bool), packbits), the
                          per-class gathers on a pool of 16 threads; wall time, and that time scaled linearly to 26 classes (host clock)

Achieved bytes/s of a gather = (source bytes touched + packed bytes written) / median time, both computed from the shapes and the tables by
`gather_bytes`: a source voxel is touched when its index occurs in all three tables.  One JSON line per stage: median, min and max of --reps repetitions
after warm-up.  The first gather's output is compared with the numpy restatement bit for bit.

    python tools/bench_nii_dataset.py [--reps 10] [--out profiles/nii_dataset_bench.json] [--shape 512 512 300] [--skip-host]"""
import argparse
import gzip
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_COPY_GBPS = 6290.0
LINES = []


def _events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return [float(np.median(ts)), float(min(ts)), float(max(ts))]


def _host(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(ts)), float(min(ts)), float(max(ts))]


def _line(stage, case, ms, nbytes=None, clock='device events', **extra):
    out = {'metric': f'{stage}: (median, min, max) ms', 'unit': 'ms', 'clock': clock, 'case': case, 'ms': ms}
    if nbytes is not None:
        gbps = nbytes / (ms[0] * 1e-3) / 1e9
        out.update({'algorithmic_bytes': int(nbytes), 'GBps': gbps, 'share_of_measured_copy_6.29TBps': gbps / HBM_COPY_GBPS})
    out.update(extra)
    LINES.append(out)
    print(json.dumps(out), flush=True)


def gather_bytes(tables, esz, nclass, V, planes=1):
    """(source bytes touched, packed bytes written): a source voxel is read when its index occurs in all three tables."""
    touched = 1
    for t in tables:
        touched *= len(np.unique(t[t >= 0]))
    return touched * esz * nclass, V * planes


def blob(shape_zyx, k):
    """An ellipsoid whose centre and radii depend on k: a mask with long runs, as organs are."""
    Z, Y, X = shape_zyx
    zz = (np.arange(Z, dtype=np.float32)[:, None, None] - Z * (0.3 + 0.05 * (k % 8))) / (Z * (0.15 + 0.02 * (k % 5)))
    yy = (np.arange(Y, dtype=np.float32)[None, :, None] - Y * (0.35 + 0.04 * (k % 7))) / (Y * (0.12 + 0.03 * (k % 4)))
    xx = (np.arange(X, dtype=np.float32)[None, None, :] - X * (0.4 + 0.03 * (k % 6))) / (X * (0.10 + 0.04 * (k % 3)))
    return (zz * zz + yy * yy + xx * xx < 1.0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--shape', type=int, nargs=3, default=[512, 512, 300], help='ni nj nk of the CT')
    ap.add_argument('--classes', type=int, default=26)
    ap.add_argument('--skip-host', action='store_true', help='leave out the gunzip and numpy lines (a profiler run)')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'nii_dataset_bench.json'))
    a = ap.parse_args()
    import nifti_ref as R
    import nii_dataset_ref as ndr
    from rsuper_amd.hip import lib
    from rsuper_amd.dataset_conversion import nii_dataset as nd
    from rsuper_amd.inference import nifti as N
    from rsuper_amd.inference import nifti_device as D
    lib.require_device()
    ni, nj, nk = a.shape
    pix = tuple(float(np.float32(v)) for v in (0.8, 0.8, 2.5))
    rng = np.random.default_rng(0)
    nvox = ni * nj * nk
    flat = (rng.normal(0.0, 30.0, size=nvox) + np.repeat(rng.choice([-1000.0, 40.0, 900.0], size=nvox // 64 + 1), 64)[:nvox])
    flat = np.clip(flat, -1024, 3071).astype(np.int16)
    ident = ((0, 1, 2), (False, False, False))
    vol = N.NiftiVolume(path='<synthetic>', data=flat, shape=(ni, nj, nk), pixdim=pix, qfac=1.0, datatype=4, vox_offset=352, scl_slope=1.0, scl_inter=0.0,
                        qform_code=0, sform_code=1, quatern=(0.0, 0.0, 0.0), qoffset=(0.0, 0.0, 0.0), srow=R.affine_for(ident[0], ident[1], pix)[:3].copy())
    geom = D.geometry_of(vol)
    X, Y, Z = geom.size
    tables = nd.nearest_tables(geom.size, geom.spacing, (1.0, 1.0, 1.0))
    box = (len(tables[2]), len(tables[1]), len(tables[0]))
    shape, offset = nd.pad_geometry(box)
    V = int(np.prod(shape))
    C = a.classes
    P = (C + 7) // 8
    case = {'ct_shape_ijk': [ni, nj, nk], 'pixdim': list(pix), 'classes': C, 'mask_dtype': 'uint8', 'box_zyx': list(box), 'padded_zyx': list(shape), 'planes': P}

    def image():
        hu, _ = D.load_nifti_device(vol, (1.0, 1.0, 1.0))
        return torch.ops.rsuper.ct_normalize_pop(hu, nd.CLIP[0], nd.CLIP[1], list(shape), list(offset), None)
    _line('image', case, _events(image, a.reps), launches=5, note='load (2 launches) + resample + ct_stats + ct_normalize_pop; allocations included')
    torch.cuda.empty_cache()

    canon = [blob((Z, Y, X), k) for k in range(8)]                   # eight distinct masks; the groups of a case differ only in content
    perm_orient = ((2, 0, 1), (False, True, False))                  # file i runs along canonical z: the unit stride is not canonical x
    ix, iy, iz = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).cuda() for t in tables)
    packed = torch.empty((P,) + shape, device='cuda', dtype=torch.uint8)
    gather = torch.ops.rsuper.label_gather_pack
    src_b, dst_b = gather_bytes(tables, 1, 8, V)
    results = {}
    for tag, orient in (('gather_identity', ident), ('gather_permuted', perm_orient)):
        files = [R.file_order(R.inverse_reorient(m, orient[0], orient[1])) for m in canon]
        shape_ijk = R.inverse_reorient(canon[0], orient[0], orient[1]).shape
        size, stride, off, _ = N.canonical_layout(shape_ijk, orient[0], orient[1])
        assert tuple(size) == (X, Y, Z)
        raw_host = torch.from_numpy(np.concatenate(files))
        if tag == 'gather_identity':
            _line('upload_group', case, _host(lambda: raw_host.to('cuda'), max(3, a.reps // 2)), raw_host.numel(), clock='host clock + synchronise',
                  note='eight masks, pageable host memory; the rate is the bus, not the HBM')
        raw = raw_host.cuda()
        desc = torch.tensor([[k * nvox, 0, stride[2], stride[1], stride[0], off, nvox, 0] for k in range(8)], dtype=torch.int64, device='cuda')
        ms = _events(lambda: gather(raw, desc, 8, None, ix, iy, iz, [Z, Y, X], packed, 0, list(offset)), a.reps)
        _line(tag, dict(case, orientation=[list(orient[0]), [bool(f) for f in orient[1]]], strides_zyx=[int(stride[2]), int(stride[1]), int(stride[0])]),
              ms, src_b + dst_b, launches=1, source_bytes_touched=int(src_b), packed_bytes_written=int(dst_b),
              note='one byte plane = eight classes; a case of 26 classes makes four such launches')
        results[tag] = packed[0].cpu().numpy()
        del raw, raw_host, files
    assert np.array_equal(results['gather_identity'], results['gather_permuted']), 'the two storage orders give different bits'

    table = {'c%02d' % v: v for v in range(1, C + 1)}
    names = sorted(table)
    lut = torch.from_numpy(nd.build_lut(names, table)).cuda()
    lm = np.zeros((Z, Y, X), np.int16)
    for k in range(8):
        lm[canon[k] != 0] = 1 + (3 * k) % C
    raw = torch.from_numpy(R.file_order(R.inverse_reorient(lm, ident[0], ident[1])).view(np.uint8).copy()).cuda()
    desc = torch.tensor([[0, 2, X * Y, X, 1, 0, nvox, 0]], dtype=torch.int64, device='cuda')
    src_lm, dst_lm = gather_bytes(tables, 2, 1, V, P)
    _line('gather_label_map', dict(case, map_dtype='int16', n_values=int(lut.shape[0])),
          _events(lambda: gather(raw, desc, 1, lut, ix, iy, iz, [Z, Y, X], packed, 0, list(offset)), a.reps), src_lm + dst_lm, launches=1,
          source_bytes_touched=int(src_lm), packed_bytes_written=int(dst_lm))
    del raw
    nbox = int(np.prod(box))
    _line('background', case, _events(lambda: torch.ops.rsuper.label_background(packed, 0, list(offset), list(box)), a.reps), nbox * (P + 1), launches=1,
          note='reads the P bytes of a box voxel, writes one')
    del packed
    torch.cuda.empty_cache()

    unpacked = torch.zeros((1, 8) + shape, device='cuda', dtype=torch.uint8)
    unpacked[0, :, offset[0]:offset[0] + box[0]:3, :, offset[2]:offset[2] + box[2]] = 1
    out = torch.empty((1, 1) + shape, device='cuda', dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    L = lib.lib()
    _line('pack_bits', dict(case, note_volume='(8, Do, Ho, Wo) uint8, the output volume of one gather'),
          _events(lambda: lib.check(L.rsuper_pack_bits(unpacked.data_ptr(), out.data_ptr(), 1, 8, V, V, V, st), 'pack_bits'), a.reps), 9 * V, launches=1,
          note='the comparable streaming kernel: reads 8 V, writes V')
    del unpacked, out
    torch.cuda.empty_cache()

    if not a.skip_host:
        gz = gzip.compress(canon[0].tobytes(), 6)
        ms = _host(lambda: gzip.decompress(gz), 3, warm=0)
        _line('gunzip_host', case, ms, clock='host clock, one thread', compressed_bytes=len(gz), raw_bytes=int(nvox), files_per_case=C,
              ms_for_all_files_one_thread=ms[0] * C, note='a blob mask compresses far better than a real one reads; the inflate rate is what counts')
        masks = {'c%d' % k: (R.inverse_reorient(canon[k], ident[0], ident[1]), ident[0], ident[1]) for k in range(8)}
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as pool:
            planes = list(pool.map(lambda k: ndr.gather_nearest((R.reorient(*masks['c%d' % k]) != 0).astype(np.int8), geom.size, geom.spacing,
                                                                (1.0, 1.0, 1.0)), range(8)))
        want = ndr.packed_labels(np.stack(planes, axis=0), nd.MIN_SIZE)
        host_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(want[0], results['gather_identity']), 'the device plane differs from the numpy restatement'
        _line('numpy_restatement', case, [host_ms] * 3, clock='host clock, 16 threads for the per-class gathers', classes_measured=8,
              ms_scaled_to_all_classes=host_ms * C / 8, device_plane_equals_restatement=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for line in LINES:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
