#!/usr/bin/env python3
"""Device times of crop-on-tumour from a whole CT with a bit-packed label (training/augmentation.py class_counts / select_voxel / crop_box, kernels
of csrc/crop.hip) next to the reference's literal ATen sequence on the same device, timed in the same call and alternated repetition by repetition.

    whole_ct   (400, 512, 512) CT, 26 classes, crop (116, 136, 136) -- the large crop of a 96^3 training size
    small_ct   (90, 160, 160) CT: shorter than the crop in z, so the source counts as padded to (116, 160, 160)

    chain      class_counts -> the one read of the totals -> select_voxel -> crop_box (what tumor_crop runs once the draws are made)
               ATen: unpack the label ((packed >> shift) & 1, what np.unpackbits does on the host in the reference), [F.pad,] the per-class sums
               of the lesion planes, torch.nonzero of the chosen plane, index, .tolist(), slice + .contiguous() of image and label
    counts / select / crop   the three kernels on their own (no host read in between)

Both sides use the same class, rank and shift; the tool asserts that they cut the same box.  Prints (and writes to --out) one JSON line per case and
part: median / min device-event times over --reps repetitions after warm-up, the algorithmic bytes (the packed label read once for the totals; one
table column and the touched chunk for the selection; the crop read and written once), the resulting GB/s and its share of the float4-copy rate
(6.29 TB/s on this part, the yardstick of DESIGN 6g).

    python tools/bench_crop.py [--reps 20] [--out profiles/crop_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GBPS = 6290.0
LINES = []


def _time_one(fn, reps):
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
    return [float(np.median(ts)), float(min(ts))]


def _time_pair(new, old, reps):
    """Alternate the two paths; returns ((median, min) new, (median, min) old) in ms."""
    for _ in range(2):
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
    out = {'metric': f'{name}: device times (median, min) ms', 'unit': 'ms', 'case': case, 'new_ms': new, 'algorithmic_bytes': int(nbytes),
           'new_GBps': gbps, 'share_of_measured_copy_6.29TBps': gbps / HBM_COPY_GBPS}
    if old is not None:
        out['aten_ms'], out['aten_over_new'] = old, old[0] / new[0]
    if note:
        out['note'] = note
    LINES.append(out)
    print(json.dumps(out), flush=True)


def synthetic_label(C, size, gen):
    """Blocky organs (8^3 blocks of low-resolution noise), two small lesion classes at the end; packed on the device as np.packbits(axis=0) would."""
    D, H, W = size
    P = (C + 7) // 8
    packed = torch.zeros((P,) + tuple(size), dtype=torch.uint8, device='cuda')
    low = [-(-s // 8) for s in size]
    for c in range(C):
        p = 0.002 if c >= C - 2 else 0.04
        m = (torch.rand(low, device='cuda', generator=gen) < p).to(torch.uint8)
        m = m.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:D, :H, :W]
        packed[c >> 3] |= m << (7 - (c & 7))
    return packed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--classes', type=int, default=26)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'crop_bench.json'))
    a = ap.parse_args()
    from rsuper_amd.hip import lib
    from rsuper_amd.training import augmentation as A
    from rsuper_amd.training.dataset import PackedBits
    lib.require_device()
    gen = torch.Generator(device='cuda').manual_seed(0)
    C, crop = a.classes, (116, 136, 136)
    P = (C + 7) // 8
    shifts = torch.arange(7, -1, -1, device='cuda', dtype=torch.uint8).view(1, 8, 1, 1, 1)

    for name, size in (('whole_ct', (400, 512, 512)), ('small_ct', (90, 160, 160))):
        D, H, W = size
        V = D * H * W
        img = torch.randn((1, 1) + size, device='cuda', generator=gen)
        packed = synthetic_label(C, size, gen)
        lab = PackedBits(packed[None], C)
        full, lo = A.padded_size(size, crop)
        need_pad = list(size) != full
        counts = A.class_counts(lab)
        totals = counts.host(0)
        cls = C - 1
        assert totals[cls] > 0, 'the synthetic lesion class is empty'
        k, offs = totals[cls] // 2, [5, -7, 11]

        def chain():
            c = A.class_counts(lab)
            t = c.host(0)
            center = A.select_voxel(c, cls, k, t[cls], add=lo)
            return A.crop_box(img, (lab,), crop, pad=full, center=center, offset=offs)

        def aten():
            inflated = ((packed[:, None] >> shifts) & 1).reshape((P * 8,) + size)[:C][None]
            im, lb = img, inflated
            if need_pad:
                pads = []
                for i in (2, 1, 0):
                    t = full[i] - size[i]
                    pads += [t // 2, t - t // 2]
                im, lb = F.pad(im, pads), F.pad(lb, pads)
            tumor = lb[0][[C - 2, C - 1]]
            if tumor.sum() == 0:
                raise AssertionError
            positives = tumor.sum(dim=(-3, -2, -1)) > 0
            [i for i in range(positives.shape[0]) if positives[i]]
            vox = torch.nonzero(lb[0][cls])
            center = vox[k]
            o = [int(np.clip(int(c) - s // 2 + f, 0, n - s)) for c, s, f, n in zip(center, crop, offs, full)]
            sl = (slice(None), slice(None), slice(o[0], o[0] + crop[0]), slice(o[1], o[1] + crop[1]), slice(o[2], o[2] + crop[2]))
            return im[sl].contiguous(), lb[sl].contiguous(), o

        ci, (cl,), used = chain()
        ri, rl, ro = aten()
        assert used.cpu().tolist() == [ro] and torch.equal(ci, ri) and torch.equal(cl.unpack(), rl), 'the two sides disagree'
        del ri, rl
        torch.cuda.empty_cache()
        case = {'shape': list(size), 'padded': full, 'classes': C, 'crop': list(crop), 'class': cls, 'rank': k}
        nchunks = -(-V // A.CROP_CHUNK)
        b_counts = P * V
        b_select = nchunks * 4 + A.CROP_CHUNK
        b_crop = 2 * (4 + P) * crop[0] * crop[1] * crop[2]
        new, old = _time_pair(chain, aten, a.reps)
        _line(name + '/chain', dict(case, launches=4, host_reads=1), new, old, b_counts + b_select + b_crop,
              'the chain includes the device-to-host read of the totals; the ATen side includes its .tolist() of the chosen voxel')
        center = A.select_voxel(counts, cls, k, totals[cls], add=lo)
        _line(name + '/counts', dict(case, launches=2), _time_one(lambda: A.class_counts(lab), a.reps), None, b_counts)
        _line(name + '/select', dict(case, launches=1), _time_one(lambda: A.select_voxel(counts, cls, k, totals[cls], add=lo), a.reps), None, b_select)
        _line(name + '/crop', dict(case, launches=1), _time_one(lambda: A.crop_box(img, (lab,), crop, pad=full, center=center, offset=offs), a.reps),
              None, b_crop)
        del img, packed, lab, counts
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for ln in LINES:
            f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
