#!/usr/bin/env python3
"""Times `python -m rsuper_amd.predict_abdomenatlas` on synthetic cases, stage by stage (read, predict, post-process, measure, write), for a tiny
UNet (base 8, 7 classes, 32^3 window, 64^3 cases) and the config-2 UNet (base 32, 26 PanTS classes, 96^3 window, 192^3 cases, bf16), in three
output modes: `--score --not_save_binary` (nothing written but the CSV rows), one .npz per class, and `--packed`; with --device-compress the two
saving modes are taken again with the command's `--device_compress` (the DEFLATE pass on the device, inference/npz_writer.py).  Each mode runs twice with
--overwrite; the second run is reported (the first pays the module loads).  For comparison the reference's measurement as it stands
(test_with_reports.detection's steps in scipy, on host copies of the same lesion planes) is timed on the same box where scipy imports.
Writes profiles/predict_bench.json and prints it as one JSON line.

    python tools/bench_predict.py [--cases 3] [--no-config2] [--no-cpu] [--device-compress]"""
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
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

SPACING = (2.5, 0.8, 0.8)
TINY_CLASSES = ['kidney_left', 'kidney_lesion', 'kidney_right', 'liver', 'liver_lesion', 'pancreas', 'pancreatic_lesion']
YAML = ('in_chan: 1\nbase_chan: {base}\ndown_scale: [[2,2,2], [2,2,2], [2,2,2], [2,2,2]]\nkernel_size: [[3,3,3], [3,3,3], [3,3,3], [3,3,3], [3,3,3]]\n'
        'block: BasicBlock\nnorm: in\ncompute_dtype: {dtype}\ntraining_size: [{win}, {win}, {win}]\n')


def setup(d, name, classes, base, win, side, dtype, n_cases):
    from rsuper_amd.model.dim3.unet import UNet
    root = os.path.join(d, name)
    os.makedirs(os.path.join(root, 'img'))
    os.makedirs(os.path.join(root, 'ckpt'))
    open(os.path.join(root, 'classes.yaml'), 'w').write('[' + ', '.join(classes) + ']\n')
    open(os.path.join(root, 'cfg.yaml'), 'w').write(YAML.format(base=base, dtype=dtype, win=win))
    torch.manual_seed(0)
    net = UNet(1, base, num_classes=len(classes), block='BasicBlock', norm='in', compute_dtype=dtype)
    torch.save({'model_state_dict': net.state_dict()}, os.path.join(root, 'ckpt', 'latest.pth'))
    r = np.random.default_rng(1)
    with open(os.path.join(root, 'spacing.csv'), 'w') as f:
        f.write('BDMAP_ID,z,y,x\n')
        for k in range(n_cases):
            hu = (r.standard_normal((side, side, side)) * 300 - 100).astype(np.int16)
            np.save(os.path.join(root, 'img', f'BDMAP_{k:08d}.npy'), hu)
            f.write(f'BDMAP_{k:08d},{SPACING[0]},{SPACING[1]},{SPACING[2]}\n')
    return root


def run_mode(root, save, flags):
    from rsuper_amd import predict_abdomenatlas as P
    argv = ['--load', os.path.join(root, 'ckpt', 'latest.pth'), '--img_path', os.path.join(root, 'img'), '--class_list',
            os.path.join(root, 'classes.yaml'), '--config', os.path.join(root, 'cfg.yaml'), '--save_path', os.path.join(root, save),
            '--spacing_csv', os.path.join(root, 'spacing.csv'), '--organ_mask_on_lesion', '--overwrite'] + flags
    res = None
    for _ in range(2):
        t0 = time.perf_counter()
        done, times = P.main(argv)
        wall = time.perf_counter() - t0
        res = {'cases': len(done), 'wall_s': round(wall, 4), 'cases_per_s': round(len(done) / sum(times.values()), 3),
               'ms_per_case': {k: round(1e3 * v / len(done), 3) for k, v in times.items()}}
    return res


def cpu_measure(root, classes, win, n_cases):
    """The reference's measurement on host copies of the lesion planes one direct predict_case call returns: ms per case (all lesion planes)."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd.inference import detection_binary, predict_case
    argv = ['--load', os.path.join(root, 'ckpt', 'latest.pth'), '--img_path', os.path.join(root, 'img'), '--class_list',
            os.path.join(root, 'classes.yaml'), '--config', os.path.join(root, 'cfg.yaml'), '--organ_mask_on_lesion']
    args = P.get_parser(argv)
    args.class_list, args.classes = classes, len(classes)
    models = P.init_model(args, classes)
    pred, _ = predict_case(models, np.load(os.path.join(root, 'img', 'BDMAP_00000000.npy')), args, classes)
    lesions = [c for c in classes if c.endswith('_lesion')]
    box = np.ones((3, 3, 3))
    t0 = time.perf_counter()
    host = {c: pred[c].cpu().numpy() for c in lesions}
    vols = []
    for c in lesions:
        a = host[c].astype(np.float64) > 0.5
        a = ndimage.zoom(a, np.array(SPACING) / np.array((1, 1, 1)), order=0)
        o = a.copy()
        a = ndimage.binary_erosion(a, structure=box, iterations=1)
        a = ndimage.binary_dilation(a, structure=box, iterations=2)
        a *= o
        vols.append(int(a.sum()))
    ms = 1e3 * (time.perf_counter() - t0)
    dev = detection_binary(torch.stack([pred[c] for c in lesions]), SPACING)
    assert dev == vols, (dev, vols)
    return {'lesion_planes': len(lesions), 'scipy_ms_per_case': round(ms, 2), 'volumes_equal_the_device': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=3)
    ap.add_argument('--no-config2', action='store_true')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--device-compress', action='store_true', help='also time the two saving modes with --device_compress')
    a = ap.parse_args()
    import synth
    from rsuper_amd.hip import lib
    lib.require_device()
    out = {'device': torch.cuda.get_device_name(0), 'spacing': SPACING, 'note': 'second of two --overwrite runs; stage times are synchronised wall '
           'times per case; cases_per_s = cases / sum of the stage times'}
    nets = [('tiny', TINY_CLASSES, 8, 32, 64, 'f32')]
    if not a.no_config2:
        nets.append(('config2', synth.PANTS_CLASSES, 32, 96, 192, 'bf16'))
    with tempfile.TemporaryDirectory() as d:
        for name, classes, base, win, side, dtype in nets:
            root = setup(d, name, classes, base, win, side, dtype, a.cases)
            res = {'classes': len(classes), 'base': base, 'window': win, 'case': [side] * 3, 'dtype': dtype,
                   'score_not_save_binary': run_mode(root, 's', ['--score', '--not_save_binary']),
                   'per_class_files': run_mode(root, 'f', []),
                   'packed': run_mode(root, 'p', ['--packed']),
                   'score_and_per_class_files': run_mode(root, 'sf', ['--score'])}
            if a.device_compress:
                res['per_class_files_device_compress'] = run_mode(root, 'fd', ['--device_compress'])
                res['packed_device_compress'] = run_mode(root, 'pd', ['--packed', '--device_compress'])
            if not a.no_cpu:
                res['reference_measurement_on_host'] = cpu_measure(root, classes, win, a.cases)
            out[name] = res
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'predict_bench.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
