#!/usr/bin/env python3
"""Device times of the NIfTI front and back end (inference/nifti_device.py, csrc/nifti.hip) on a synthetic hospital CT: 512 x 512 x 300 int16
voxels at 0.78 x 0.78 x 2.5 mm, stored 'LAS' (one flipped axis), resampled to 1 mm -> (750, 399, 399).

    upload           the file's voxel buffer, pageable host memory -> device (host clock around the copy and a synchronise)
    load_prefilter   rsuper_nifti_load_prefilter with prefilter: strided, scaled read -> x pass -> y pass in place (two launches)
    load_only        the same entry point without prefilter (the same-spacing path): one launch
    resample         rsuper_bspline_resample through the host's tables
    reorient_store   rsuper_reorient_store of --classes uint8 planes behind their 352 header bytes
    save_nifti_masks the whole back end: stack, headers, reorient_store, device DEFLATE, read-back of the compressed bytes, file writes (host clock)
    scipy_host       scipy.ndimage.spline_filter + map_coordinates on --host-slices source slices of the same case (float64, one thread), and
                     that time scaled linearly to the 300 slices -- the arithmetic of the reference's SimpleITK front end, which is not installed

One JSON line per stage: median and min of --reps repetitions after warm-up (device events unless the line says host clock), the algorithmic
bytes of DESIGN.md 6p, the resulting GB/s and its share of what a float4 copy reaches on this part (6.29 TB/s, MI355X microarchitecture notes).
The lines are printed and written to --out.

    python tools/bench_nifti.py [--reps 10] [--classes 4] [--host-slices 12] [--out profiles/nifti_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

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
    return [float(np.median(ts)), float(min(ts))]


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
    return [float(np.median(ts)), float(min(ts))]


def _line(stage, case, ms, nbytes=None, clock='device events', **extra):
    out = {'metric': f'{stage}: (median, min) ms', 'unit': 'ms', 'clock': clock, 'case': case, 'ms': ms}
    if nbytes is not None:
        gbps = nbytes / (ms[0] * 1e-3) / 1e9
        out.update({'algorithmic_bytes': int(nbytes), 'GBps': gbps, 'share_of_measured_copy_6.29TBps': gbps / HBM_COPY_GBPS})
    out.update(extra)
    LINES.append(out)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--classes', type=int, default=4)
    ap.add_argument('--host-slices', type=int, default=12)
    ap.add_argument('--shape', type=int, nargs=3, default=[512, 512, 300], help='ni nj nk')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'nifti_bench.json'))
    a = ap.parse_args()
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import nifti as N
    from rsuper_amd.inference import nifti_device as D
    import nifti_ref as R
    lib.require_device()
    ni, nj, nk = a.shape
    pix = (0.78, 0.78, 2.5)
    perm, flip = (0, 1, 2), (False, True, False)                     # 'LAS'
    rng = np.random.default_rng(0)
    # a smooth body with sharp edges and noise, in file order
    flat = (rng.normal(0.0, 30.0, size=ni * nj * nk) + np.repeat(rng.choice([-1000.0, 40.0, 900.0], size=ni * nj * nk // 64 + 1), 64)[:ni * nj * nk])
    flat = np.clip(flat, -1024, 3071).astype(np.int16)
    A = R.affine_for(perm, flip, pix)
    vol = N.NiftiVolume(path='<synthetic>', data=flat, shape=(ni, nj, nk), pixdim=tuple(float(np.float32(v)) for v in pix), qfac=1.0, datatype=4,
                        vox_offset=352, scl_slope=1.0, scl_inter=0.0, qform_code=0, sform_code=1, quatern=(0.0, 0.0, 0.0), qoffset=(0.0, 0.0, 0.0),
                        srow=A[:3].copy())
    geom = D.geometry_of(vol)
    size, stride, offset, _ = N.canonical_layout(vol.shape, geom.perm, geom.flip)
    X, Y, Z = size
    nvox = X * Y * Z
    case = {'shape_ijk': [ni, nj, nk], 'pixdim': list(pix), 'orientation': 'LAS', 'dtype': 'int16'}

    host_bytes = torch.from_numpy(flat.view(np.uint8))
    _line('upload', case, _host(lambda: host_bytes.to('cuda'), a.reps), flat.nbytes, clock='host clock + synchronise',
          note='pageable host memory; the rate is the bus, not the HBM')
    raw = host_bytes.to('cuda')
    load = torch.ops.rsuper.nifti_load_prefilter
    args = (raw, 2, [Z, Y, X], list(stride[::-1]), offset, 1.0, 0.0)
    _line('load_prefilter', case, _events(lambda: load(*args, True), a.reps), nvox * (2 + 4 + 4 + 4), launches=2,
          note='pass 1 reads int16 and writes f32, pass 2 reads and writes f32 in place; the time includes the output allocation')
    _line('load_only', case, _events(lambda: load(*args, False), a.reps), nvox * (2 + 4), launches=1)
    coef = load(*args, True)
    tabs = D.resample_tables(geom.size, geom.spacing, (1.0, 1.0, 1.0), 'cuda')
    out = torch.ops.rsuper.bspline_resample(coef, *tabs, 0.0)
    case_r = dict(case, out_zyx=list(out.shape))
    _line('resample', case_r, _events(lambda: torch.ops.rsuper.bspline_resample(coef, *tabs, 0.0), a.reps), 4 * nvox + 4 * out.numel(), launches=1,
          note='every coefficient read once, every output written once; the time includes the output allocation')

    # correctness of what was timed, on a few slices against scipy (also the host's time for the same arithmetic)
    from scipy import ndimage
    canon = R.reorient(flat.reshape(nk, nj, ni).transpose(2, 1, 0), perm, flip)
    px, inx = R.positions(X, geom.spacing[0], 1.0)
    py, iny = R.positions(Y, geom.spacing[1], 1.0)
    zt = R.nearest_table(Z, geom.spacing[2], 1.0)
    coords = np.stack(np.meshgrid(py, px, indexing='ij'))
    ns = max(1, min(a.host_slices, Z))
    t0 = time.perf_counter()
    host = {}
    for zs in np.linspace(0, Z - 1, ns).astype(int):
        host[int(zs)] = ndimage.map_coordinates(ndimage.spline_filter(canon[zs].astype(np.float64), order=3, mode='mirror'), coords, order=3,
                                                mode='mirror', prefilter=False)
    host_s = time.perf_counter() - t0
    worst = 0.0
    plane_in = iny[:, None] & inx[None, :]
    for zs, ref in host.items():
        zo = int(np.nonzero(zt == zs)[0][0])
        worst = max(worst, float(np.abs(out[zo].cpu().numpy()[plane_in] - ref[plane_in]).max()))
    assert worst <= 0.02, f'the device result is {worst} HU from scipy'
    _line('scipy_host', case_r, [host_s * 1e3 / len(host) * Z] * 2, clock='host clock, one thread', slices_measured=len(host),
          measured_ms=host_s * 1e3, note=f'spline_filter + map_coordinates of {len(host)} source slices, scaled linearly to {Z}; nearest-z copies not charged',
          max_abs_difference_to_device_HU=worst)
    del coef, out, raw
    torch.cuda.empty_cache()

    # ---- the way back
    C = a.classes
    gen = torch.Generator(device='cuda').manual_seed(1)
    zz = torch.arange(Z, device='cuda')[:, None, None]
    yy = torch.arange(Y, device='cuda')[None, :, None]
    xx = torch.arange(X, device='cuda')[None, None, :]
    stack = torch.stack([(((zz - Z // 2) * 2.5) ** 2 + (yy - Y // 2 + 20 * c) ** 2 + (xx - X // 2) ** 2 < (60 + 10 * c) ** 2).to(torch.uint8)
                         for c in range(C)])
    header = N.nifti1_header(geom.shape_ijk, geom.pixdim, geom.affine, 2)
    plane = len(header) + nvox
    buf = torch.zeros((C * plane,), device='cuda', dtype=torch.uint8)
    cstride = (1, X, X * Y)
    st = [(-cstride[geom.perm[k]] if geom.flip[k] else cstride[geom.perm[k]]) for k in range(3)]
    off = sum((geom.shape_ijk[k] - 1) * cstride[geom.perm[k]] for k in range(3) if geom.flip[k])
    case_s = dict(case, classes=C, dtype='uint8 blobs')
    _line('reorient_store', case_s, _events(lambda: torch.ops.rsuper.reorient_store(stack, buf, len(header), plane, list(geom.shape_ijk), st, off),
                                            a.reps), 2 * C * nvox, launches=1)
    pred = {f'class_{c}': stack[c] for c in range(C)}
    with tempfile.TemporaryDirectory() as d:
        ms = _host(lambda: D.save_nifti_masks(d, pred, list(pred), geom), max(2, a.reps // 3))
        size_on_disk = sum(os.path.getsize(os.path.join(d, 'predictions', f)) for f in os.listdir(os.path.join(d, 'predictions')))
        h, arr = R.read_nifti_gz(os.path.join(d, 'predictions', 'class_0.nii.gz'))
        assert np.array_equal(arr, R.inverse_reorient(stack[0].cpu().numpy(), perm, flip)), 'the saved mask differs'
    _line('save_nifti_masks', case_s, ms, clock='host clock + synchronise', compressed_bytes=int(size_on_disk), raw_bytes=int(C * plane),
          note='stack + headers + reorient_store + device DEFLATE + read-back of the compressed bytes + file writes')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for line in LINES:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
