#!/usr/bin/env python3
"""Times of the tail of MedFormer's ClassificationBranch (reducer -> transformer block -> token mean -> head; model/dim3/medformer.py), fused
(torch.ops.rsuper.cls_tail, csrc/cls_branch.hip: 1 launch forward, 2 backward) against the unfused chain of existing operators
(RSUPER_MF_CLS_FUSED=0), for a batch of 2 at L = 27 tokens (96^3 crops) and L = 64 (128^3), Nc = 3 (multi-task head) and 768 (CLIP head):

    fwd      the forward of the tail
    fwd_bwd  forward + gradients of the input and the 15 parameters (torch.autograd.grad: no accumulation kernels)

Per case and path: `device_ms` = device events around the call, `host_ms` = host wall clock until the device has finished, each as [median, min] over
--reps repetitions after warm-up.  MedFormer's step is host-bound, so `host_ms` is the figure that bears on the step.

    python tools/bench_cls_branch.py [--reps 20] [--batch 2] [--out profiles/cls_branch_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _device_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return [float(np.median(ts)), float(min(ts))]


def _host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return [float(np.median(ts)), float(min(ts))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cls_branch_bench.json'))
    a = ap.parse_args()
    import rsuper_amd  # noqa: F401
    from rsuper_amd.hip import lib
    from rsuper_amd.model.dim3 import medformer as M
    lib.require_device()
    res = dict(tool='bench_cls_branch', batch=a.batch, reps=a.reps, device=torch.cuda.get_device_name(0), cases=[])
    for L in (27, 64):
        for nc in (3, 768):
            torch.manual_seed(0)
            br = M.ClassificationBranch(num_classes=nc).cuda()
            x = torch.randn(a.batch, L, 1, 1, 160, device='cuda', requires_grad=True)
            go = torch.randn(a.batch, nc, device='cuda')
            inputs = [x] + list(br.parameters())             # no extra layer: every parameter belongs to the tail
            case = dict(L=L, Nc=nc)
            for path, fused in (('fused', True), ('unfused', False)):
                M.CLS_FUSED = fused

                def fwd():
                    with torch.no_grad():
                        return br.tail(x)

                def fwd_bwd():
                    return torch.autograd.grad(br.tail(x), inputs, go)
                for name, fn in (('fwd', fwd), ('fwd_bwd', fwd_bwd)):
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    case[f'{path}_{name}'] = dict(device_ms=_device_ms(fn, a.reps), host_ms=_host_ms(fn, a.reps))
            M.CLS_FUSED = True
            for name in ('fwd', 'fwd_bwd'):
                case[f'speedup_{name}_host'] = case[f'unfused_{name}']['host_ms'][0] / case[f'fused_{name}']['host_ms'][0]
                case[f'speedup_{name}_device'] = case[f'unfused_{name}']['device_ms'][0] / case[f'fused_{name}']['device_ms'][0]
            res['cases'].append(case)
            print(json.dumps(case))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
