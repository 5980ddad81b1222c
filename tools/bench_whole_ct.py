#!/usr/bin/env python3
"""Training from whole CTs (training/dataset/whole_ct.py, dataset/packed.py upload_label, csrc/label_bits.hip pack_bits_kernel): what the path costs.

    pack / unpack   rsuper_pack_bits next to rsuper_unpack_bits on the same (C, D, H, W) volume, alternated repetition by repetition, device events.
                    Algorithmic bytes of both: C * V one-byte planes + ceil(C / 8) * V packed bytes.  GB/s and the share of the float4-copy rate
                    (6.29 TB/s on this part, the yardstick of DESIGN 6g).  Also the byte path of pack_bits (an unaligned destination offset).
    upload          upload_label of an unpacked int8 (C, D, H, W) host label for several chunk_bytes, and of the same label already packed: host
                    clock around a call that ends in a device synchronise (the staging copies are host work), median of --reps.
    loader          samples/s of WholeVolumeLoader over a synthetic tree (--volumes CTs of --size, labels stored packed / unpacked), prefetch on /
                    off, 0 / --workers DataLoader workers, batch 2, no compute between the batches: host clock over the whole pass, synchronised at the end.
    step            the config-2 training step (B = 2, 96^3, base 32, 26 classes, bf16, segmentation loss, fused optimiser) fed by the loader
                    (labels packed / unpacked, 0 / --workers DataLoader workers, prefetch on -- prefetch_next() after the step is queued, as
                    train_epoch does -- and off) against the same step fed from a resident batch.  Every step ends with the host reading the loss,
                    as train_epoch's meters do.  ms per step, host clock over --steps steps after warm-up, synchronised at the end.

Prints one JSON line per figure and writes them to --out.

    python tools/bench_whole_ct.py [--reps 10] [--steps 20] [--out profiles/whole_ct_bench.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_crop import HBM_COPY_GBPS, _time_pair, _time_one, synthetic_label  # noqa: E402

LINES = []


def emit(**kw):
    LINES.append(kw)
    print(json.dumps(kw), flush=True)


def class_names(C):
    """The benchmark's own 26 classes (tests/golden/synth.py); any other count: generic organs + the pancreas and its lesion class."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import synth
    if C == len(synth.PANTS_CLASSES):
        return sorted(synth.PANTS_CLASSES)
    return sorted(['organ_%02d' % i for i in range(C - 2)] + ['pancreas', 'pancreatic_lesion'])


def bench_kernels(C, size, reps):
    from rsuper_amd.hip import lib as _l
    from rsuper_amd.training.dataset import unpack_bits_device, pack_bits_device
    gen = torch.Generator(device='cuda').manual_seed(0)
    packed = synthetic_label(C, size, gen)[None]
    P, V = packed.shape[1], int(np.prod(size))
    plain = unpack_bits_device(packed, C)
    assert torch.equal(pack_bits_device(plain).packed, packed)
    L, st = _l.lib(), torch.cuda.current_stream().cuda_stream
    out_p, out_u = torch.empty_like(packed), torch.empty_like(plain)
    pk = lambda: _l.check(L.rsuper_pack_bits(plain.data_ptr(), out_p.data_ptr(), 1, C, V, V, V, st), 'pack_bits')
    un = lambda: _l.check(L.rsuper_unpack_bits(packed.data_ptr(), out_u.data_ptr(), 1, P, C, V, st), 'unpack_bits')
    tp, tu = _time_pair(pk, un, reps)
    nbytes = (C + P) * V
    for name, t in (('rsuper_pack_bits', tp), ('rsuper_unpack_bits', tu)):
        gbps = nbytes / (t[0] * 1e-3) / 1e9
        emit(metric=name + ': device time (median, min) ms', classes=C, size=list(size), ms=t, algorithmic_bytes=nbytes, GBps=gbps,
             share_of_measured_copy=gbps / HBM_COPY_GBPS)
    big = torch.empty(P * V + 64, dtype=torch.uint8, device='cuda')
    tb = _time_one(lambda: _l.check(L.rsuper_pack_bits(plain.data_ptr(), big.data_ptr() + 5, 1, C, V, V, V, st), 'pack_bits'), reps)
    emit(metric='rsuper_pack_bits, byte path (destination 5 bytes off alignment): device time (median, min) ms', classes=C, size=list(size), ms=tb,
         GBps=nbytes / (tb[0] * 1e-3) / 1e9)
    assert torch.equal(big[5:5 + P * V].view_as(packed), packed)


def bench_upload(C, size, reps):
    from rsuper_amd.training.dataset import upload_label
    gen = torch.Generator(device='cuda').manual_seed(1)
    packed = synthetic_label(C, size, gen)
    from rsuper_amd.training.dataset import unpack_bits_device
    lab = unpack_bits_device(packed[None], C)[0].cpu().numpy().view(np.int8)
    host_packed = packed.cpu().numpy()

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del r
        return [float(np.median(ts)), float(min(ts))]
    for mb in (8, 16, 32, 64, 128, 512):
        got = upload_label(lab, C, 'cuda', chunk_bytes=mb << 20)
        assert torch.equal(got.packed[0], packed)
        t = wall(lambda: upload_label(lab, C, 'cuda', chunk_bytes=mb << 20))
        emit(metric='upload_label, unpacked int8 label: host ms (median, min)', classes=C, size=list(size), chunk_MiB=mb, ms=t,
             host_GBps=lab.nbytes / (t[0] * 1e-3) / 1e9, unpacked_bytes=int(lab.nbytes))
    t = wall(lambda: upload_label(host_packed, C, 'cuda'))
    emit(metric='upload_label, packed label: host ms (median, min)', classes=C, size=list(size), ms=t, packed_bytes=int(host_packed.nbytes))
    reps = 2
    t = wall(lambda: torch.from_numpy(np.packbits(lab.astype(np.bool_), axis=0)).to('cuda'))
    emit(metric='np.packbits on the host + upload (what the loader would do without the kernel): host ms (median, min)', classes=C, size=list(size), ms=t)


def write_tree(base, n, C, size, form):
    root = os.path.join(base, form)
    os.makedirs(os.path.join(root, 'list'))
    names = class_names(C)
    with open(os.path.join(root, 'list', 'label_names.yaml'), 'w') as f:
        f.write(''.join('- %s\n' % c for c in names))
    from rsuper_amd.training.dataset import unpack_bits_device
    for i in range(n):
        gen = torch.Generator(device='cuda').manual_seed(10 + i)
        packed = synthetic_label(C, size, gen)
        img = (torch.rand(size, device='cuda', generator=gen) * 2 - 1).cpu().numpy()
        name = 'BDMAP_%08d' % (i + 1)
        np.save(os.path.join(root, name + '.npy'), img)
        np.save(os.path.join(root, name + '_gt.npy'), packed.cpu().numpy() if form == 'packed' else unpack_bits_device(packed[None], C)[0].cpu().numpy().view(np.int8))
    return root


def loader_for(root, ts, prefetch, order, batch=2, workers=0):
    from rsuper_amd.training.dataset.whole_ct import WholeVolumeDataset, WholeVolumeLoader
    a = argparse.Namespace(data_root=root, UFO_root=None, reports=None, ucsf_ids=None, training_size=[ts] * 3, scale=0.3, rotate=45, translate=0.1)
    ds = WholeVolumeDataset(a, all_train=True, crop_on_tumor=True, tumor_classes=['pancreas'])
    return WholeVolumeLoader(ds, batch_size=batch, sampler=[i % len(ds) for i in order], prefetch=prefetch, num_workers=workers)


def bench_loader(base, n, C, size, ts, passes, workers):
    roots = {form: write_tree(base, n, C, size, form) for form in ('packed', 'unpacked')}
    order = list(range(2 * n * passes))
    for form, root in roots.items():
        for prefetch, nw in ((True, 0), (False, 0), (True, workers), (False, workers)):
            np.random.seed(0), torch.manual_seed(0)
            ld = loader_for(root, ts, prefetch, order, workers=nw)
            for _ in ld:                       # warm-up pass: page cache, pinned allocations, the per-path totals
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            for b in ld:
                k += b['image'].shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            emit(metric='WholeVolumeLoader samples/s (no compute between batches)', labels=form, prefetch=prefetch, workers=nw, classes=C, size=list(size),
                 training_size=ts, samples=k, seconds=dt, samples_per_s=k / dt)
    return roots


def bench_step(roots, ts, steps, warmup, workers):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import bench
    from rsuper_amd.train_ddp import train_step
    from rsuper_amd.training.augmentation import intensity_augment_batch
    classes = class_names(26)
    a = argparse.Namespace(base=32, no_pool=False, unpacked_labels=False)
    leg = bench.Leg(a, 'bf16', False, 0, 1, 0, False, classes, 2, ts)

    res = {}
    n = 2 * (steps + warmup)
    feeds = [('resident batch', lambda: None)]
    for form in ('packed', 'unpacked'):
        for nw in (0, workers):
            for prefetch in (True, False):
                feeds.append(('loader, %s labels, %d workers, prefetch %s' % (form, nw, 'on' if prefetch else 'off'),
                              lambda form=form, nw=nw, prefetch=prefetch: loader_for(roots[form], ts, prefetch, range(n), workers=nw)))
    feeds.append(('resident batch (again)', lambda: None))
    for name, mk in feeds:
        np.random.seed(0), torch.manual_seed(0)
        ld = mk()
        if ld is not None:
            for _ in loader_for(ld.dataset.args.data_root, ts, False, range(2 * len(ld.dataset))):    # page cache
                pass
        it = iter(ld) if ld is not None else None          # one iterator serves warm-up and the timed window

        def run(n):
            for _ in range(n):
                batch = leg.batch
                if it is not None:
                    batch = next(it)
                    batch['image'] = intensity_augment_batch(batch['image'])
                loss, _ = train_step(leg.model, leg.ema, leg.opt, batch, leg.largs, classes, leg.step)
                if it is not None:
                    ld.prefetch_next()         # as train_epoch does once the step is queued
                float(loss['overall'])         # ... and then reads the loss for its meters: the host waits for the step here
                leg.step += 1
        run(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = dt / steps * 1e3
        del it, ld
        emit(metric='config-2 training step (B=2, %d^3, base 32, 26 classes, bf16): ms/step' % ts, feed=name, steps=steps, ms_per_step=res[name])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--classes', type=int, default=26)
    ap.add_argument('--kernel-size', type=int, nargs=3, default=[160, 512, 512])
    ap.add_argument('--size', type=int, nargs=3, default=[160, 320, 320], help='CTs of the loader tree')
    ap.add_argument('--volumes', type=int, default=4)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--workers', type=int, default=4, help='DataLoader workers of the legs that use workers')
    ap.add_argument('--training-size', type=int, default=96)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'whole_ct_bench.json'))
    a = ap.parse_args()
    from rsuper_amd.hip import lib as _l
    _l.require_device()
    for C in sorted({a.classes, 42}):
        bench_kernels(C, tuple(a.kernel_size), a.reps)
    bench_upload(a.classes, tuple(a.kernel_size), max(3, a.reps // 2))
    base = tempfile.mkdtemp(prefix='whole_ct_bench_')
    try:
        roots = bench_loader(base, a.volumes, a.classes, tuple(a.size), a.training_size, a.passes, a.workers)
        bench_step(roots, a.training_size, a.steps, a.warmup, a.workers)
    finally:
        shutil.rmtree(base, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(LINES, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
