#!/usr/bin/env python3
"""Host time per call of the operators of MedFormer's attention stages (hip/ops.py over csrc/pointwise.hip, depthwise.hip, instnorm.hip) on small tensors,
where the GPU work is negligible: what remains is torch's allocations, ctypes, the queries, the argument checks, the dispatch of csrc/mf_plan.hpp and
the launches.  --root TREE measures another checkout with the same calls.  Usage: python tools/mf_host_cost.py [--root TREE] [--calls N]"""
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
dev, bf = 'cuda', torch.bfloat16
xs, xl = torch.randn((2, 6, 6, 6, 64), device=dev), torch.randn((2, 12, 12, 12, 64), device=dev)
w3 = torch.randn((64, 1, 3, 3, 3), device=dev)
x2, dy2, w = torch.randn((432, 64), device=dev), torch.randn((432, 128), device=dev), torch.randn((128, 64), device=dev)
se = [torch.randn(s, device=dev) for s in ((16, 64, 1, 1, 1), (16,), (64, 16, 1, 1, 1), (64,))]


def norm_bwd(x):
    xr = x.clone().requires_grad_(True)
    y = ops.ChannelNormFn.apply(xr, 1e-5, True)
    return lambda: torch.autograd.grad(y, xr, x, retain_graph=True)


rows = [
    ('ChannelNormFn fwd, 216 voxels', lambda: ops.ChannelNormFn.apply(xs, 1e-5, True)),
    ('ChannelNormFn fwd, 1728 voxels', lambda: ops.ChannelNormFn.apply(xl, 1e-5, True)),
    ('ChannelNormFn bwd, 216 voxels', norm_bwd(xs)),
    ('ChannelNormFn bwd, 1728 voxels', norm_bwd(xl)),
    ('pointwise_gemm 432 x 64 -> 128', lambda: ops.pointwise_gemm(x2, w, None, 0, bf)),
    ('pointwise_wgrad 432 x 128 x 64', lambda: ops.pointwise_wgrad(dy2, x2, True, bf)),
    ('DepthwiseConvFn fwd, 12^3 x 64', lambda: ops.DepthwiseConvFn.apply(xl, w3)),
    ('SqueezeExciteFn fwd, 12^3 x 64', lambda: ops.SqueezeExciteFn.apply(xl, *se)),
]
with torch.no_grad():
    for name, fn in rows:
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        best = float('inf')
        for _ in range(5):                                       # best of five batches: the launch queue and the clock settle
            t0 = time.perf_counter()
            for _ in range(a.calls // 5):
                fn()
            best = min(best, (time.perf_counter() - t0) / (a.calls // 5) * 1e6)
            torch.cuda.synchronize()
        print(f'{name:32s} {best:6.2f} us of host time per call')
