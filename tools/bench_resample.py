#!/usr/bin/env python3
"""Device times of the whole-CT preprocessing (inference/preprocess.py, kernels rsuper_ct_stats / rsuper_ct_normalize) and of the class-stack
resampler (inference/resample.py, kernel rsuper_resample3d) at sizes a user runs, next to what a user of the previous commit runs on the same
device: the reference's literal ATen sequence, timed in the same call and alternated with the new path repetition by repetition.

    ct_normalize     (400, 512, 512) CT -> z-score (nothing is short of the training size, so neither side pads), from int16 and from float32
                     ATen: clip / mean / std / sub_ / div_ on the float32 volume (preprocess :347-352)
    ct_normalize_pad (80, 512, 512) CT with training size 96: z is short, so x is widened to 530 (the reference's axis quirk) -- ragged rows
                     ATen: the same plus F.pad(t, (9, 9, 0, 0, 0, 0))
    nearest_u8       26 uint8 label planes, the (334, 410, 410) box of a (338, 410, 410) prediction -> (400, 512, 512)
                     ATen: per plane unpad (slice) -> F.interpolate(mode='nearest')
    trilinear_thr    the same stack as float32 probabilities -> `> 0.5` as uint8, one launch
                     ATen: per plane unpad -> F.interpolate(mode='trilinear', align_corners=True) -> `> 0.5`
                     (the reference also copies every plane to the host and back; that round trip is NOT charged to the ATen side here)

Prints one JSON line per case: median / min device-event times of both sides over --reps repetitions after warm-up, their ratio, the algorithmic
bytes (every source voxel read once, every output voxel written once; the statistics pass reads the volume once more), the resulting GB/s and its
share of the HBM peak (8.0 TB/s specified; 6.29 TB/s is what a float4 copy reaches on this part, MI355X microarchitecture notes).

    python tools/bench_resample.py [--reps 20] [--planes 26]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
HBM_COPY_GBPS = 6290.0


def _time_pair(new, old, reps):
    """Alternate the two paths; returns ((median, min) new, (median, min) old) in ms."""
    for _ in range(3):
        new()
        old()
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(reps):
        for fn, ts in ((new, tn), (old, to)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
    return [float(np.median(tn)), float(min(tn))], [float(np.median(to)), float(min(to))]


def _line(name, case, new, old, nbytes, note=None):
    gbps = nbytes / (new[0] * 1e-3) / 1e9
    out = {'metric': f'{name}: device times (median, min) ms', 'unit': 'ms', 'case': case, 'new_ms': new, 'aten_ms': old,
           'aten_over_new': old[0] / new[0], 'algorithmic_bytes': int(nbytes), 'new_GBps': gbps, 'share_of_hbm_peak_8TBps': gbps / HBM_PEAK_GBPS,
           'share_of_measured_copy_6.29TBps': gbps / HBM_COPY_GBPS}
    if note:
        out['note'] = note
    print(json.dumps(out), flush=True)


def _aten_zscore(x, pad):
    t = torch.clip(x, -991, 500)
    mean = torch.mean(t)
    std = torch.std(t)
    t -= mean
    t /= std
    if pad:
        t = F.pad(t, (pad, pad, 0, 0, 0, 0))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--planes', type=int, default=26)
    a = ap.parse_args()
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import preprocess_array, resample_image_with_gpu, unpad_img
    from rsuper_amd.inference.preprocess import ct_stats_workspace
    lib.require_device()
    gen = torch.Generator(device='cuda').manual_seed(0)
    ws = ct_stats_workspace('cuda')

    # ---- z-score
    for name, shape, ts in (('ct_normalize', (400, 512, 512), (96, 96, 96)), ('ct_normalize_pad', (80, 512, 512), (96, 96, 96))):
        hu = (torch.randn(shape, device='cuda', generator=gen) * 400 - 200).round().clamp(-2000, 3000)
        hu16 = hu.to(torch.int16)
        args = argparse.Namespace(dimension='3d', training_size=list(ts))
        out, idx = preprocess_array(hu16, args, workspace=ws)
        pad = (out.shape[2] - shape[2]) // 2
        ref = _aten_zscore(hu, pad)
        assert out.shape == ref.shape and float((out - ref).abs().max()) < 1e-4, 'the two sides disagree'
        n, no = int(np.prod(shape)), out.numel()
        del out, ref
        for dt, x in (('int16', hu16), ('float32', hu)):
            new, old = _time_pair(lambda: preprocess_array(x, args, workspace=ws), lambda: _aten_zscore(hu, pad), a.reps)
            _line(name, {'shape': list(shape), 'out_shape': [shape[0], shape[1], shape[2] + 2 * pad], 'input': dt, 'launches': 2}, new, old,
                  2 * n * x.element_size() + 4 * no, 'the ATen side always starts from the float32 volume, as the reference uploads it')
        del hu, hu16
        torch.cuda.empty_cache()

    # ---- resampling
    C, pshape, box, out_zyx = a.planes, (338, 410, 410), [2, 336, 0, 410, 0, 410], (400, 512, 512)
    new_size = out_zyx[::-1]
    a3 = argparse.Namespace(dimension='3d')
    vin = C * 334 * 410 * 410
    vout = C * int(np.prod(out_zyx))
    note = None if C == 26 else f'{C} planes instead of 26'

    lab = (torch.rand((C,) + pshape, device='cuda', generator=gen) < 0.3).to(torch.uint8)

    def aten_nearest():
        return [F.interpolate(unpad_img(p, box, a3)[None, None], size=list(out_zyx), mode='nearest')[0, 0] for p in lab]

    got = resample_image_with_gpu(lab, new_size=new_size, interp='nearest', box=box)
    assert torch.equal(got[C - 1], aten_nearest()[C - 1]), 'the two sides disagree'
    del got
    new, old = _time_pair(lambda: resample_image_with_gpu(lab, new_size=new_size, interp='nearest', box=box), aten_nearest, a.reps)
    _line('nearest_u8', {'planes': C, 'padded': list(pshape), 'box': box, 'out': list(out_zyx), 'launches': 1}, new, old, vin + vout, note)
    del lab
    torch.cuda.empty_cache()

    prob = torch.rand((C,) + pshape, device='cuda', generator=gen)

    def aten_trilinear():
        return [(F.interpolate(unpad_img(p, box, a3)[None, None], size=list(out_zyx), mode='trilinear', align_corners=True)[0, 0] > 0.5) for p in prob]

    got = resample_image_with_gpu(prob, new_size=new_size, interp='trilinear', box=box, threshold=0.5)
    ref = aten_trilinear()[C - 1]
    differ = int((got[C - 1].bool() != ref).sum())
    assert differ <= 1e-5 * ref.numel(), f'{differ} voxels of the last plane differ'       # values within a rounding of 0.5 may fall either way
    del got, ref
    new, old = _time_pair(lambda: resample_image_with_gpu(prob, new_size=new_size, interp='trilinear', box=box, threshold=0.5), aten_trilinear,
                          a.reps)
    _line('trilinear_thr', {'planes': C, 'padded': list(pshape), 'box': box, 'out': list(out_zyx), 'launches': 1, 'voxels_differing_in_last_plane': differ},
          new, old, 4 * vin + vout, note)


if __name__ == '__main__':
    main()
