#!/usr/bin/env python3
"""Device times of the prediction post-processing (inference/detection.py, inference/postprocess.py) on a CT-sized synthetic case: 42 classes
predicted at 0.8 x 0.8 x 2.5 mm (D, H, W) = (160, 640, 640), i.e. 400 x 512 x 512 voxels after detection resamples a lesion plane to 1 mm.
Prints one JSON line.  Where scipy is importable (and without --no-cpu) it also times the reference's CPU forms on the same arrays: the
literal 9-threshold loop of eval_AUC.detection, postprocess_npz's binary_dilation masking, keep_largest_component as ndimage.label + the
largest-size pick (SimpleITK is not installed here; ndimage.label with the default structure gives the same face-connected components).

    python tools/bench_postprocess.py [--depth 160] [--side 640] [--reps 5] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

SPACING = (2.5, 0.8, 0.8)


def _synthetic_case(C, D, H, W, seed):
    """Smooth per-class probability volumes on the device: a coarse random grid, trilinear up-sampling, a sigmoid."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    coarse = torch.randn((1, C, max(2, D // 16), max(2, H // 32), max(2, W // 32)), generator=g, device='cuda')
    x = torch.nn.functional.interpolate(coarse, size=(D, H, W), mode='trilinear', align_corners=True)[0]
    return torch.sigmoid(3.0 * x - 2.0).contiguous()


def _time(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=160)
    ap.add_argument('--side', type=int, default=640)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    import synth
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import detection, keep_largest_component, zoom_shape
    lib.require_device()
    classes = synth.MASK42_CLASSES
    C, D, H, W = len(classes), a.depth, a.side, a.side
    pred = _synthetic_case(C, D, H, W, 0)
    lesions = [i for i, c in enumerate(classes) if 'lesion' in c]
    organ_idx = {c: i for i, c in enumerate(classes) if 'lesion' not in c}
    from rsuper_amd.inference.postprocess import organ_planes
    plan = [(i, [organ_idx[p] for p in organ_planes(classes[i], organ_idx)]) for i in lesions]
    les_i, oa, ob = [p[0] for p in plan], [p[1][0] for p in plan], [p[1][1] if len(p[1]) > 1 else -1 for p in plan]
    labels = (pred > 0.5).to(torch.uint8)
    plane = pred[lesions[0]].contiguous()
    lesion_planes = pred[lesions].contiguous()
    out_shape = zoom_shape((D, H, W), SPACING)
    vox_in, vox_out = D * H * W, int(np.prod(out_shape))
    ths = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
    mask = labels[lesions[0]].contiguous()

    res = {}
    res['detection_1_plane_ms'] = _time(lambda: torch.ops.rsuper.detection_volumes(plane[None], list(out_shape), ths, True), a.reps)
    res['detection_1_plane_plain_ms'] = _time(lambda: torch.ops.rsuper.detection_volumes(plane[None], list(out_shape), ths, False), a.reps)
    res[f'detection_{len(lesions)}_planes_ms'] = _time(lambda: torch.ops.rsuper.detection_volumes(lesion_planes, list(out_shape), ths, True), a.reps)
    iso = plane[:, :, :]
    res['detection_identity_1_plane_ms'] = _time(lambda: torch.ops.rsuper.detection_volumes(iso[None], [D, H, W], ths, True), a.reps)
    res[f'organ_mask_f32_{len(lesions)}_planes_ms'] = _time(lambda: torch.ops.rsuper.organ_mask(pred, les_i, oa, ob), a.reps)
    res[f'organ_mask_u8_{len(lesions)}_planes_ms'] = _time(lambda: torch.ops.rsuper.organ_mask(labels, les_i, oa, ob), a.reps)
    res['largest_component_ms'] = _time(lambda: keep_largest_component(mask), a.reps)
    rnd = (torch.rand((D, H, W), device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) < 0.31).to(torch.uint8)
    res['largest_component_density031_ms'] = _time(lambda: keep_largest_component(rnd), a.reps)
    vols, mprob = detection(plane, spacing=SPACING)
    out = {'metric': 'prediction post-processing device times (median, min) ms', 'unit': 'ms',
           'case': {'classes': C, 'lesion_planes': len(lesions), 'predicted_shape': [D, H, W], 'spacing_mm': list(SPACING),
                    'detection_shape_1mm': list(out_shape), 'voxels_in': vox_in, 'voxels_1mm': vox_out,
                    'lesion_voxels_first_plane': int(mask.sum()), 'density031_voxels': int(rnd.sum())},
           'times': res,
           'rates': {'detection_1mm_voxels_per_s': vox_out / (res['detection_1_plane_ms'][0] * 1e-3),
                     'detection_input_GBps': vox_in * 4 / (res['detection_1_plane_ms'][0] * 1e-3) / 1e9,
                     'organ_mask_f32_GBps': len(lesions) * vox_in * 4 * 4 / (res[f'organ_mask_f32_{len(lesions)}_planes_ms'][0] * 1e-3) / 1e9},
           'detection_first_plane': {'volumes': {str(k): v for k, v in vols.items()}, 'max_prob': mprob}}

    if not a.no_cpu:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            cpu = {'threads': int(os.environ.get('OMP_NUM_THREADS', '0') or 0), 'note': 'single-process scipy, as eval_AUC / predict call it'}
            x = plane.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            arr = ndimage.zoom(x, np.array(SPACING), order=1)
            cpu['zoom_s'] = time.perf_counter() - t0
            box = np.ones((3, 3, 3))
            t0 = time.perf_counter()
            cvols = {}
            for th in ths:
                b = arr > th
                e = ndimage.binary_erosion(b, structure=box, iterations=1)
                e = ndimage.binary_dilation(e, structure=box, iterations=2)
                e &= b
                cvols[th] = int(e.sum())
            cpu['detection_loop_s'] = time.perf_counter() - t0
            cpu['detection_total_s'] = cpu['zoom_s'] + cpu['detection_loop_s']
            cpu['detection_equal'] = cvols == vols and float(np.max(arr)) == mprob
            p = labels.cpu().numpy()
            t0 = time.perf_counter()
            for i, (o1, o2) in zip(les_i, zip(oa, ob)):
                org = p[o1] + p[o2] if o2 >= 0 else p[o1]
                org = ndimage.binary_dilation((org > 0.5).astype(np.uint8), structure=box).astype(p.dtype)
                _ = org * p[i]
            cpu[f'organ_mask_u8_{len(lesions)}_planes_s'] = time.perf_counter() - t0
            m = mask.cpu().numpy()
            t0 = time.perf_counter()
            cc, n = ndimage.label(m > 0)
            sizes = np.bincount(cc.ravel())
            sizes[0] = 0
            keep = (cc == int(np.argmax(sizes))) if n else np.ones_like(m, bool)
            cpu['largest_component_s'] = time.perf_counter() - t0
            cpu['largest_component_equal'] = bool(np.array_equal(keep.astype(np.uint8), keep_largest_component(mask).cpu().numpy()))
            cpu['speedup_detection'] = cpu['detection_total_s'] / (res['detection_1_plane_ms'][0] * 1e-3)
            cpu['speedup_largest_component'] = cpu['largest_component_s'] / (res['largest_component_ms'][0] * 1e-3)
            out['cpu_reference'] = cpu
    print(json.dumps(out))


if __name__ == '__main__':
    main()
