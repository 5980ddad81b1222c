#!/usr/bin/env python3
"""Times the write stage of a config-2 case (26 class planes of 192^3 uint8) on the host path (stack.cpu().numpy() + np.savez_compressed per class, and
the --packed form) and on the device path (inference/npz_writer.py, csrc/deflate.hip) under both code tables, in one process on one box, for two mask sets:

    noise   what tools/bench_predict.py saves: the masks of an untrained config-2 UNet on a noise volume (close to zlib's slowest input)
    blobs   ellipsoid organs and small spherical lesions, what a trained network produces

Per set and path: milliseconds per case (device path: kernel, read-back and file write apart), bytes on disk and the size against the host files (zlib
level 6).  Every device file is loaded with np.load and compared with the stack once.  The host path is slow (seconds per case), so it runs --host-reps
times and the device path --reps times after one warm-up; medians and minima are reported.  Writes profiles/deflate_bench.json, prints it as one JSON line.

    python tools/bench_deflate.py [--reps 5] [--host-reps 2] [--side 192] [--no-noise]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def noise_masks(d, classes, side):
    """The planes predict_abdomenatlas saves for bench_predict's config-2 setup: an untrained UNet on noise."""
    import bench_predict as bp
    from rsuper_amd import predict_abdomenatlas as P
    from rsuper_amd.inference import predict_case
    root = bp.setup(d, 'config2', classes, 32, 96, side, 'bf16', 1)
    argv = ['--load', os.path.join(root, 'ckpt', 'latest.pth'), '--img_path', os.path.join(root, 'img'), '--class_list',
            os.path.join(root, 'classes.yaml'), '--config', os.path.join(root, 'cfg.yaml'), '--organ_mask_on_lesion']
    args = P.get_parser(argv)
    args.class_list, args.classes = classes, len(classes)
    models = P.init_model(args, classes)
    pred, _ = predict_case(models, np.load(os.path.join(root, 'img', 'BDMAP_00000000.npy')), args, classes)
    stack = torch.stack([pred[c].to(torch.uint8) for c in classes])
    del models
    return stack


def blob_masks(planes, side, seed=0):
    """Organs: one ellipsoid per plane with radii of 6 .. 25 % of the side; every third plane a lesion class instead: 0 .. 3 spheres of radius 2 .. 6."""
    r = np.random.default_rng(seed)
    ax = torch.arange(side, device='cuda', dtype=torch.float32)
    z, y, x = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    out = torch.zeros((planes, side, side, side), dtype=torch.uint8, device='cuda')
    for p in range(planes):
        if p % 3 == 2:
            for _ in range(int(r.integers(0, 4))):
                c, rad = r.uniform(0.25, 0.75, 3) * side, float(r.uniform(2, 6))
                out[p] |= (((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) < rad * rad).to(torch.uint8)
        else:
            c, rad = r.uniform(0.3, 0.7, 3) * side, r.uniform(0.06, 0.25, 3) * side
            out[p] = ((((z - c[0]) / rad[0]) ** 2 + ((y - c[1]) / rad[1]) ** 2 + ((x - c[2]) / rad[2]) ** 2) < 1.0).to(torch.uint8)
    return out


def tree_bytes(paths):
    return sum(os.path.getsize(p) for p in paths)


def summary(ms):
    return {'median': round(statistics.median(ms), 3), 'min': round(min(ms), 3), 'runs': len(ms)}


def host_paths(stack, names, d, reps):
    """The parent's write_binary, per class and packed."""
    from rsuper_amd.training.dataset.packed import pack_bits_device
    per, packed = [], []
    files = [os.path.join(d, f'host_{n}.npz') for n in names]
    pfile = os.path.join(d, 'host_packed.npz')
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = stack.cpu().numpy()
        for k, f in enumerate(files):
            np.savez_compressed(f, host[k])
        per.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        bits = pack_bits_device(stack).packed[0].cpu().numpy()
        np.savez_compressed(pfile, arr_0=bits, classes=np.array(names))
        packed.append(1e3 * (time.perf_counter() - t0))
    return ({'ms_per_case': summary(per), 'bytes': tree_bytes(files)}, {'ms_per_case': summary(packed), 'bytes': os.path.getsize(pfile)})


def device_paths(stack, names, d, table, reps, host_bytes, host_packed_bytes):
    from rsuper_amd.inference.npz_writer import save_planes_npz, savez_compressed_device
    from rsuper_amd.training.dataset.packed import pack_bits_device
    files = [os.path.join(d, f'dev_{table}_{n}.npz') for n in names]
    pfile = os.path.join(d, f'dev_{table}_packed.npz')
    stages = {'total': [], 'kernel': [], 'readback': [], 'file': []}
    packed = []
    for rep in range(reps + 1):                                    # the first one warms up (code objects, allocator) and is dropped
        torch.cuda.synchronize()
        tm = {}
        t0 = time.perf_counter()
        save_planes_npz(files, stack, table=table, timings=tm)
        tm['total'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        bits = pack_bits_device(stack).packed[0]
        savez_compressed_device(pfile, table=table, arr_0=bits, classes=np.array(names))
        tp = time.perf_counter() - t0
        if rep:
            for k in stages:
                stages[k].append(1e3 * tm[k])
            packed.append(1e3 * tp)
    host = stack.cpu().numpy()
    for k, f in enumerate(files):
        with np.load(f) as z:
            assert np.array_equal(z['arr_0'], host[k]), f
    with np.load(pfile) as z:
        assert np.array_equal(z['arr_0'], np.packbits(host, axis=0)) and list(z['classes']) == list(names)
    nbytes, pbytes = tree_bytes(files), os.path.getsize(pfile)
    return ({'ms_per_case': {k: summary(v) for k, v in stages.items()}, 'bytes': nbytes, 'bytes_over_host_zlib6': round(nbytes / host_bytes, 3)},
            {'ms_per_case': summary(packed), 'bytes': pbytes, 'bytes_over_host_zlib6': round(pbytes / host_packed_bytes, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--side', type=int, default=192)
    ap.add_argument('--no-noise', action='store_true')
    a = ap.parse_args()
    import synth
    from rsuper_amd.hip import lib
    lib.require_device()
    classes = list(synth.PANTS_CLASSES)
    out = {'device': torch.cuda.get_device_name(0), 'planes': len(classes), 'case': [a.side] * 3,
           'note': 'wall times that end in a synchronise or in a finished file, ms per case; host = stack.cpu().numpy() + np.savez_compressed (zlib level 6); '
                   'device stages: kernel = launches to synchronise, readback = sizes, CRCs and compressed bytes to host, file = ZIP writes'}
    with tempfile.TemporaryDirectory() as d:
        sets = {}
        if not a.no_noise:
            sets['noise'] = noise_masks(d, classes, a.side)
        sets['blobs'] = blob_masks(len(classes), a.side)
        for name, stack in sets.items():
            res = {'raw_bytes': stack.numel(), 'voxels_set': round(float(stack.float().mean().item()), 4)}
            res['host_per_class'], res['host_packed'] = host_paths(stack, classes, d, a.host_reps)
            for table in ('fixed', 'mask'):
                res[f'device_{table}_per_class'], res[f'device_{table}_packed'] = device_paths(
                    stack, classes, d, table, a.reps, res['host_per_class']['bytes'], res['host_packed']['bytes'])
            out[name] = res
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'deflate_bench.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
