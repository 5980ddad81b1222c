#!/usr/bin/env python3
"""Device times of the intensity augmentation (training/augmentation.py intensity_augment_batch, kernel csrc/augment_intensity.hip) for a batch of
2 volumes at 116 x 136 x 136 (the large crop of --aug_device gpu) and 96^3 (the training size), for three plans applied to every sample:

    all six       multiply, additive, gamma, contrast, blur (sigma 1.5: radius 5), noise from the in-kernel generator     3 launches
    blur only     sigma 1.5                                                                                             1 launch
    pointwise     multiply, additive, noise                                                                             1 launch

and the time the six CPU functions of training/augmentation.py take for ONE sample of the same plan, called in online_intensity_augmentation's order
with their draws forced to the plan's values, on the box's 16 CPUs (torch.set_num_threads(16)) -- what a DataLoader worker spends per sample.

Prints one JSON line per shape: median / min device time, launch count and traffic model of each plan, and the CPU times.  Traffic model, bytes per
voxel: a stats pass reads 4; the apply pass reads 4 * halo and writes 4, halo = staged voxels per output voxel of an 8 x 8 x 32 brick ((8 + 2 r)^2 *
16-byte groups covering 32 + 2 r, / 2048; 1 without blur); the explicit-noise variant would read 4 more.

    python tools/bench_intensity.py [--reps 20] [--batch 2]"""
import argparse
import json
import os
import sys
import time
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(116, 136, 136), (96, 96, 96)]
PLANS = {'all_six': dict(multiply=1.2, additive=-0.05, gamma=1.3, contrast=1.2, sigma=1.5, noise_std=0.1),
         'blur_only': dict(sigma=1.5),
         'pointwise_only': dict(multiply=1.2, additive=-0.05, noise_std=0.1)}


def _time(fn, reps):
    for _ in range(3):
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
    return float(np.median(ts)), float(min(ts))


def _cpu_ms(A, x, plan, reps=3):
    """One sample through the CPU functions with the plan's parameters: torch.rand returns 0, so a range (v, v + 1) yields exactly v."""
    on = lambda k: plan.flags[0] >> k & 1

    def zeros(*a, **kw):
        return torch.zeros(kw['size'] if 'size' in kw else a)

    def chain(v):
        if on(0):
            v = A.brightness_multiply(v, multiply_range=(plan.multiply[0], plan.multiply[0] + 1))
        if on(1):
            v = A.brightness_additive(v, std=0.1)
        if on(2):
            v = A.gamma(v, gamma_range=(plan.gamma[0], plan.gamma[0] + 1))
        if on(3):
            v = A.contrast(v, contrast_range=(plan.contrast[0], plan.contrast[0] + 1))
        if on(4):
            v = A.gaussian_blur(v, sigma_range=(plan.sigma[0], plan.sigma[0] + 1))
        if on(5):
            v = A.gaussian_noise(v, std=plan.noise_std[0])      # draws its own field: that is part of the cost
        return v
    ts = []
    with mock.patch.object(torch, 'rand', zeros), \
            mock.patch.object(torch, 'normal', lambda *a, **kw: torch.full(kw['size'], plan.additive[0], dtype=torch.float32)):
        for _ in range(reps + 1):
            t = time.perf_counter()
            chain(x)
            ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=2)
    a = ap.parse_args()
    from rsuper_amd.hip import lib
    from rsuper_amd.training import augmentation as A
    lib.require_device()
    torch.set_num_threads(16)
    B = a.batch
    for shape in SHAPES:
        img = torch.randn((B, 1) + shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))
        host = img[:1].cpu()
        vox = B * int(np.prod(shape))
        out = {'metric': 'intensity augmentation device times (median, min) ms', 'unit': 'ms', 'case': {'batch': B, 'shape': list(shape), 'voxels': vox},
               'times': {}, 'launches': {}, 'traffic_model_bytes_per_voxel': {}, 'rates_GBps': {}, 'cpu_16_threads_ms_per_sample': {}}
        for name, kw in PLANS.items():
            plan = A.make_intensity_plan(B, seed=list(range(1, B + 1)), **{k: [v] * B for k, v in kw.items()})
            r = plan.radius[0]
            halo = (8 + 2 * r) ** 2 * 4 * (((8 + 32 + r + 3) >> 2) - ((8 - r) >> 2)) / 2048.0 if 'sigma' in kw else 1.0
            n = A.intensity_launches(plan)
            passes = {'stats_read': 4 * (n - 1), 'apply_read': 4 * halo, 'apply_write': 4}
            med, mn = _time(lambda: A.intensity_augment_batch(img, plan), a.reps)
            out['times'][name] = [med, mn]
            out['launches'][name] = n
            out['traffic_model_bytes_per_voxel'][name] = passes
            out['rates_GBps'][name] = vox * sum(passes.values()) / (med * 1e-3) / 1e9
            out['cpu_16_threads_ms_per_sample'][name] = _cpu_ms(A, host, plan)
        print(json.dumps(out), flush=True)
        del img
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
