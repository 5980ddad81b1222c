#!/usr/bin/env python3
"""Device times of the spatial augmentation (training/augmentation.py affine_center_crop, kernel csrc/augment.hip) against the ATen composition
the reference runs (F.affine_grid + F.grid_sample, bilinear for the image and nearest for the float label planes, then the centre slice) on the
same GPU, B = 2 samples of 26 classes:

    116 x 136 x 136 -> 96^3    scale 0.3, rotate 45, translate 0.1   (the function's defaults)
    148 x 168 x 168 -> 128^3   scale 0,   rotate 30, translate 0     (the shipped MedFormer YAML)

The fused path reads the f32 image and the bit-packed label / unknown / segment volumes (4 bytes per voxel each) and writes only the crop; the
ATen path reads the image and 26 float planes per volume and writes the whole grid.  Prints one JSON line per case with both times (median,
min), the bytes of the traffic model -- image and packed bytes of the source voxels the crop touches, plus 16 bytes written per output voxel --
and the bytes per second that model gives at the measured time.

    python tools/bench_augment.py [--reps 20] [--batch 2] [--classes 26]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((116, 136, 136), (96, 96, 96), dict(scale=0.3, rotate=45, translate=0.1)),
         ((148, 168, 168), (128, 128, 128), dict(scale=0, rotate=30, translate=0))]


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


def _blobs(B, C, size, seed):
    """(B, C, D, H, W) 0/1 u8 on the device: a smooth random field per class, thresholded."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    coarse = torch.randn((B, C) + tuple(max(2, s // 12) for s in size), generator=g, device='cuda')
    return (F.interpolate(coarse, size=size, mode='trilinear', align_corners=True) > 0.8).to(torch.uint8)


def _pack(u8):
    """np.packbits(axis = class) on the device: (B, C, ...) 0/1 -> (B, ceil(C / 8), ...)."""
    B, C = u8.shape[:2]
    P = (C + 7) // 8
    pad = torch.zeros((B, P * 8 - C) + tuple(u8.shape[2:]), dtype=torch.uint8, device=u8.device)
    bits = torch.cat([u8, pad], 1).reshape((B, P, 8) + tuple(u8.shape[2:]))
    out = torch.zeros((B, P) + tuple(u8.shape[2:]), dtype=torch.uint8, device=u8.device)
    for k in range(8):
        out |= bits[:, :, k] << (7 - k)
    return out.contiguous()


def _touched_source_voxels(theta, size, crop, off):
    """Source voxels the crop reads (the 8 trilinear corners of every output voxel; the nearest voxel is one of them), per sample."""
    D, H, W = size
    n = []
    for t in theta.double().cuda():
        ax = [(-1 + 2 * torch.arange(o, o + c, device='cuda', dtype=torch.float64) / (N - 1)) for o, c, N in zip(off, crop, size)]
        z, y, x = torch.meshgrid(*ax, indexing='ij')
        src = [((t[r, 0] * x + t[r, 1] * y + t[r, 2] * z + t[r, 3]) + 1) / 2 * (N - 1) for r, N in zip(range(3), (W, H, D))]
        fl = [torch.floor(s).long() for s in src]
        hit = torch.zeros(D * H * W, dtype=torch.bool, device='cuda')
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    xx, yy, zz = fl[0] + dx, fl[1] + dy, fl[2] + dz
                    ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (zz >= 0) & (zz < D)
                    hit[((zz * H + yy) * W + xx)[ok]] = True
        n.append(int(hit.sum()))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--classes', type=int, default=26)
    a = ap.parse_args()
    from rsuper_amd.hip import lib
    from rsuper_amd.training import augmentation as A
    lib.require_device()
    B, C = a.batch, a.classes
    for size, crop, kw in CASES:
        np.random.seed(size[0])
        theta = torch.stack([A.draw_affine_3d(**kw) for _ in range(B)])
        theta_dev = theta.cuda()
        img = torch.randn((B, 1) + size, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))
        u8 = [_blobs(B, C, size, 1 + k) for k in range(3)]
        packed = [_pack(v) for v in u8]
        planes = [v.float() for v in u8]
        del u8
        off = A.crop_offsets(size, crop, 'center')
        sl = tuple(slice(o, o + c) for o, c in zip(off, crop))

        def fused(nvol):
            return A.affine_center_crop(img, tuple(packed[:nvol]), theta_dev, crop)

        def aten(nvol):
            grid = F.affine_grid(theta_dev, list(img.shape), align_corners=True)
            i = F.grid_sample(img, grid, mode='bilinear', padding_mode='zeros', align_corners=True)[(..., ) + sl].contiguous()
            vs = [F.grid_sample(p, grid, mode='nearest', padding_mode='zeros', align_corners=True)[(..., ) + sl].contiguous() for p in planes[:nvol]]
            return i, vs

        # the two paths compute the same thing: bytes differ only where an f32 coordinate rounds to the other neighbour
        fi, fv = fused(3)
        ai, av = aten(3)
        diff = [float((_pack(v.to(torch.uint8)) != f).float().mean()) for v, f in zip(av, fv)]
        img_diff = float((fi - ai).abs().max())
        del ai, av
        res = {}
        for nvol in (3, 1):
            res['fused_%dvol_ms' % nvol] = _time(lambda: fused(nvol), a.reps)
            res['aten_%dvol_ms' % nvol] = _time(lambda: aten(nvol), a.reps)
        P = packed[0].shape[1]
        vox_out = B * int(np.prod(crop))
        touched = sum(_touched_source_voxels(theta, size, crop, off))
        model = {n: touched * (4 + n * P) + vox_out * (4 + n * P) for n in (3, 1)}
        aten_bytes = {n: B * int(np.prod(size)) * (4 + 12 + (4 + 4) * (1 + n * C)) for n in (3, 1)}     # grid write + read, every plane read + written
        out = {'metric': 'spatial augmentation device times (median, min) ms', 'unit': 'ms',
               'case': {'batch': B, 'classes': C, 'packed_planes': P, 'source': list(size), 'crop': list(crop), 'args': kw,
                        'output_voxels': vox_out, 'source_voxels': B * int(np.prod(size)), 'source_voxels_touched': touched},
               'times': res,
               'traffic_model_bytes': {'fused_%dvol' % n: model[n] for n in model},
               'aten_minimum_bytes': {'aten_%dvol' % n: aten_bytes[n] for n in aten_bytes},
               'rates': {'fused_%dvol_GBps' % n: model[n] / (res['fused_%dvol_ms' % n][0] * 1e-3) / 1e9 for n in model},
               'speedup_over_aten': {'%dvol' % n: res['aten_%dvol_ms' % n][0] / res['fused_%dvol_ms' % n][0] for n in model},
               'agreement': {'byte_fraction_differing': diff, 'image_max_abs_diff': img_diff}}
        print(json.dumps(out), flush=True)
        del img, packed, planes
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
