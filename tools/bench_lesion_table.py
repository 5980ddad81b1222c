#!/usr/bin/env python3
"""Times of the lesion table (rsuper_amd.inference.lesion_table, csrc/lesion_table.hip) on one synthetic whole-CT case -- 512 x 512 x 400 voxels,
four lesion planes, each with a dozen ellipsoid blobs plus salt noise -- next to the scipy / numpy restatement the tests use
(tests/lesion_table_ref.py: scipy.ndimage.label per plane, brute-force diameters) on the same masks on the host.  The device time is the wall time of
the whole call with the label volume, after a warm-up call; the host time is one run of the restatement, the masks already in host memory (the
transfer a host implementation would also pay is reported apart).  Results are compared.  Prints one JSON line and writes it to --out (default
profiles/lesion_table_bench.json).  Nothing here asserts a speed-up.

    python tools/bench_lesion_table.py [--depth 400] [--side 512] [--planes 4] [--reps 5] [--no-cpu] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def synthetic_planes(P, D, H, W, seed, blobs=12, salt=2e-5):
    """(P, D, H, W) uint8: per plane `blobs` ellipsoids with semi-axes of 2..9 voxels at random places and salt noise of density `salt`."""
    r = np.random.default_rng(seed)
    out = np.zeros((P, D, H, W), np.uint8)
    for p in range(P):
        for _ in range(blobs):
            rad = r.integers(2, 10, 3)
            c = [int(r.integers(rad[i] + 1, s - rad[i] - 1)) for i, s in enumerate((D, H, W))]
            g = np.ogrid[tuple(slice(-int(v), int(v) + 1) for v in rad)]
            e = sum((g[i] / float(rad[i])) ** 2 for i in range(3)) <= 1.0
            box = tuple(slice(c[i] - int(rad[i]), c[i] + int(rad[i]) + 1) for i in range(3))
            out[p][box] |= e.astype(np.uint8)
        n = int(salt * D * H * W)
        out[p].reshape(-1)[r.integers(0, D * H * W, n)] = 1
    return out


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=400)
    ap.add_argument('--side', type=int, default=512)
    ap.add_argument('--planes', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max_lesions', type=int, default=64)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lesion_table_bench.json'))
    a = ap.parse_args()
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import lesion_table
    lib.require_device()
    P, D, H, W = a.planes, a.depth, a.side, a.side
    spacing = (2.5, 0.8, 0.8)
    host = synthetic_planes(P, D, H, W, 0)
    t0 = time.perf_counter()
    masks = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    call = lambda: lesion_table(masks, spacing=spacing, conn=26, max_lesions=a.max_lesions, return_labels=True)      # noqa: E731
    out = {'metric': 'lesion table of one whole-CT case: wall ms of one call on the device (median, min), seconds of the scipy / numpy restatement '
                     'on the host', 'shape': [D, H, W], 'planes': P, 'spacing': list(spacing), 'conn': 26, 'max_lesions': a.max_lesions,
           'foreground_voxels': int(host.sum()), 'launches_per_call': int(lib.lib().rsuper_lesion_table_launches()),
           'workspace_bytes': int(lib.lib().rsuper_lesion_table_workspace_bytes(P, D, H, W, a.max_lesions))}
    out['device_ms'] = _time(call, a.reps)
    t = call()
    ri, rf, totals = t.host()
    out.update(components=[int(v) for v in totals[:, 0]], rows=[int(v) for v in totals[:, 3]], capped_rows=int((ri[..., 15] != 0).sum()),
               largest_voxels=[int(v) for v in ri[:, 0, 1]])
    t0 = time.perf_counter()
    t.labels.cpu()
    out['labels_to_host_s'] = time.perf_counter() - t0
    out['masks_to_device_s'] = upload_s
    if not a.no_cpu:
        import lesion_table_ref as R
        t0 = time.perf_counter()
        want = R.tables(host, spacing=spacing, conn=26, max_lesions=a.max_lesions)
        out['host_scipy_s'] = time.perf_counter() - t0
        b, wb = rf[..., 2], want['rows_f'][..., 2]
        out['equal_to_host'] = bool(np.array_equal(ri, want['rows_i']) and np.array_equal(totals, want['totals'])
                                    and np.array_equal(rf[..., [0, 1, 3]], want['rows_f'][..., [0, 1, 3]]) and (np.abs(b - wb) <= 1e-9 * np.abs(wb)).all()
                                    and np.array_equal(t.labels.cpu().numpy(), want['labels']))
        out['host_over_device'] = out['host_scipy_s'] / (out['device_ms'][0] * 1e-3)
        out['host'] = {'threads': int(os.environ.get('OMP_NUM_THREADS', '0') or 0), 'note': 'single-process scipy.ndimage.label + numpy brute force'}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
