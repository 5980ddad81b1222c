#!/usr/bin/env python3
"""Host time per call of the C-ABI entry points of the bandwidth-bound glue kernels (InstanceNorm backward tail, max pool, subsample, trilinear
up-sampling) on small tensors, where the GPU work is negligible: what remains is ctypes + argument checks + the dispatch of csrc/glue_plan.hpp + the
launch.  --root TREE measures another checkout's library with the same calls.  Usage: python tools/glue_host_cost.py [--root TREE] [--calls N]"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--calls', type=int, default=2000)
a = ap.parse_args()
sys.path.insert(0, a.root)
import torch  # noqa: E402
from rsuper_amd.hip import lib, ops  # noqa: E402

lib.require_device()
L, dev, dt = ops._L(), 'cuda', torch.bfloat16
N, C, I, O = 2, 64, (6, 6, 6), (12, 12, 12)
d, st = ops._DT[dt], ops._stream()
lo, hi = torch.randn((N,) + I + (C,), device=dev).to(dt), torch.randn((N,) + O + (C,), device=dev).to(dt)
lo2, hi2 = torch.empty_like(lo), torch.empty_like(hi)
mr, gm = torch.ones((N, C, 2), device=dev), torch.zeros((N, C, 2), device=dev)
blocks = ops._stat_blocks(6 ** 3)
part = torch.empty((N, max(blocks, ops._stat_blocks(12 ** 3)), C, 2), device=dev)
p = ops._ptr
rows = [
    ('rsuper_in_bwd_finalize', lambda: L.rsuper_in_bwd_finalize(d, p(hi), C, p(hi), C, p(mr), p(gm), None, C, None, C, p(hi2), C, N, 12 ** 3, C, st)),
    ('rsuper_maxpool2_fwd', lambda: L.rsuper_maxpool2_fwd(d, p(hi), C, p(lo2), C, p(part), blocks, N, *O, C, st)),
    ('rsuper_maxpool2_bwd', lambda: L.rsuper_maxpool2_bwd(d, p(hi), C, p(lo), C, p(hi2), C, N, *O, C, st)),
    ('rsuper_subsample2_fwd', lambda: L.rsuper_subsample2_fwd(d, p(hi), C, p(lo2), C, p(part), blocks, N, *O, C, st)),
    ('rsuper_subsample2_bwd', lambda: L.rsuper_subsample2_bwd(d, p(lo), C, p(hi2), C, N, *O, C, st)),
    ('rsuper_upsample_fwd', lambda: L.rsuper_upsample_fwd(d, p(lo), C, p(hi2), C, p(part), ops._stat_blocks(12 ** 3), N, *I, *O, C, st)),
    ('rsuper_upsample_bwd', lambda: L.rsuper_upsample_bwd(d, p(hi), C, p(lo2), C, N, *I, *O, C, st)),
]
for name, fn in rows:
    for _ in range(50):
        assert fn() == 0, name
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(5):                                           # best of five batches: the launch queue and the clock settle
        t0 = time.perf_counter()
        for _ in range(a.calls // 5):
            fn()
        best = min(best, (time.perf_counter() - t0) / (a.calls // 5) * 1e6)
        torch.cuda.synchronize()
    print(f'{name:26s} {best:6.2f} us of host time per call')
