#!/usr/bin/env python3
"""Times of the report-guided pseudo-label refinement (rsuper_amd.baselines.pseudo_labels.extract_lesion_candidates, csrc/pseudo_label.hip) on a
CT-sized smooth probability volume, next to the scipy restatement of the reference's loop (tests/pseudo_labels_ref.py) on the same input:
one plane with n_lesions = 1, 3, 10, and one 8-plane case (n = 1, 2, 3, 1, 2, 3, 1, 2) in a single call.  The device time is the wall time of the
whole call -- the copy of the input, every launch and every read of the state block -- after a warm-up call; the host time is one run of the
restatement (per plane, summed, for the 8-plane case).  Results are compared for equality.  Prints one JSON line and writes it to --out
(default profiles/pseudo_labels_bench.json).

    python tools/bench_pseudo_labels.py [--depth 256] [--side 256] [--reps 5] [--batch K] [--no-cpu] [--out FILE]"""
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


def _synthetic_planes(P, D, H, W, seed):
    """Smooth per-plane probability volumes on the device: a coarse random grid, trilinear up-sampling, a sigmoid."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    coarse = torch.randn((1, P, max(2, D // 24), max(2, H // 24), max(2, W // 24)), generator=g, device='cuda')
    x = torch.nn.functional.interpolate(coarse, size=(D, H, W), mode='trilinear', align_corners=True)[0]
    return torch.sigmoid(3.0 * x - 2.0).contiguous()


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
    ap.add_argument('--depth', type=int, default=256)
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=None, help='iterations enqueued per state read (default: DEFAULT_BATCH)')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pseudo_labels_bench.json'))
    a = ap.parse_args()
    from rsuper_amd.baselines.pseudo_labels import DEFAULT_BATCH, extract_lesion_candidates, last_state
    from rsuper_amd.hip import lib
    lib.require_device()
    K = DEFAULT_BATCH if a.batch is None else a.batch
    D, H, W = a.depth, a.side, a.side
    planes = _synthetic_planes(8, D, H, W, 0)
    counts8 = [1, 2, 3, 1, 2, 3, 1, 2]
    cases = [('1_plane_n%d' % n, planes[0], n) for n in (1, 3, 10)] + [('8_planes', planes, counts8)]
    cpu = None
    if not a.no_cpu:
        try:
            import pseudo_labels_ref as pr
            import scipy  # noqa: F401
            cpu = pr
        except ImportError:
            cpu = None
    out = {'metric': 'report-guided pseudo-label refinement: wall ms of one call (median, min) on the device, seconds of the scipy loop on the host',
           'shape': [D, H, W], 'voxels_per_plane': D * H * W, 'batch_K': K, 'launches_per_iteration': 5, 'cases': {}}
    for name, x, n in cases:
        res = {}
        res['device_ms'] = _time(lambda: extract_lesion_candidates(x, n, batch=K), a.reps)
        mask, kept = extract_lesion_candidates(x, n, batch=K)
        res.update(n_lesions=n, kept=kept, iterations=list(last_state['iterations']), state_reads=list(last_state['reads']),
                   voxels=int(mask.sum()))
        res['device_ms_per_iteration'] = res['device_ms'][0] / max(1, max(last_state['iterations']))
        if cpu is not None:
            xs = x.cpu().numpy()
            xs, ns = (xs[None], [n]) if xs.ndim == 3 else (xs, n)
            t0 = time.perf_counter()
            ref = [cpu.candidates(v, k) for v, k in zip(xs, ns)]
            res['host_scipy_s'] = time.perf_counter() - t0
            got = mask.cpu().numpy()
            got = got[None] if got.ndim == 3 else got
            res['equal_to_host'] = bool(all(np.array_equal(g, r[0]) for g, r in zip(got, ref))
                                        and [r[1] for r in ref] == ([kept] if isinstance(kept, int) else kept)
                                        and [r[2] for r in ref] == res['iterations'])
            res['host_over_device'] = res['host_scipy_s'] / (res['device_ms'][0] * 1e-3)
        out['cases'][name] = res
    if cpu is not None:
        out['host'] = {'threads': int(os.environ.get('OMP_NUM_THREADS', '0') or 0), 'note': 'single-process numpy + scipy.ndimage.label, as the reference runs it'}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
