#!/usr/bin/env python3
"""Device times of the report-annotated crop from a whole CT with a bit-packed label (training/augmentation.py union_bbox / crop_foreground_3d /
label_remap, kernels of csrc/crop_report.hip) next to the reference's literal sequence as ATen calls on the same device, timed in the same
process and alternated repetition by repetition.

    pancreas_head   (400, 512, 512) CT, 28 classes_UFO -> 42 classes, crop (96, 96, 96): one pancreas segment, its box fits at once
    liver           the same CT, the 8 liver segments: an ellipsoid of 250 x 300 x 250 plus a speck and a spur (raw box 320 x 351 x 448), so the opening
                    (3 iterations) and the component step run and the answer is still 'mask does not fit crop size' -- what every liver crop at 96^3 goes through
    small_ct        (90, 160, 160) CT, pancreas head: the source counts as padded to (116, 160, 160)

    chain     union_bbox -> read -> [union_bits -> bits_open -> read -> largest_component -> union_bbox -> read ->] crop_box -> class_counts of the
              crop -> read -> label_remap (label, unknown map and chosen-segment mask in one launch); corner with rand=False on both sides
              ATen: unpack the label ((packed >> shift) & 1, np.unpackbits in the reference), stack and sum of the segment planes, binarise,
              .sum().item(), torch.nonzero and six .min() / .max().item(), slice + .contiguous(), and assign_labels' / get_chosen_segment_mask's
              plane-by-plane lists and torch.stack.  Where the box does not fit the ATen side ends after the six extrema: the reference's next step
              is scipy on the host, timed on its own (`scipy_open_s`: binary_erosion / binary_dilation with iterations=3 and ndimage.label over the
              whole CT, one run, time.perf_counter; skipped with --no-scipy or without scipy).
    bbox / bits / open / component / remap   the kernels on their own (no host read in between)

The tool asserts that both sides cut the same box and build the same three volumes.  Prints (and writes to --out) one JSON line per case and part:
median / min device-event times over --reps repetitions after warm-up, the algorithmic bytes (the byte planes the set touches read once; the box's
bit words read and written once per pass plus the u8 mask; the crop's planes read once and three volumes written), GB/s and its share of the
float4-copy rate (6.29 TB/s on this part, the yardstick of DESIGN 6g).

    python tools/bench_report_crop.py [--reps 20] [--no-scipy] [--out profiles/report_crop_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_crop import HBM_COPY_GBPS, _time_one, _time_pair  # noqa: E402

LINES = []
LIVER = ['liver_segment_%d' % i for i in range(1, 9)]
PANCREAS = ['pancreas_head', 'pancreas_body', 'pancreas_tail']
CLASSES_UFO = (['background'] + LIVER + PANCREAS + ['kidney_left', 'kidney_right', 'spleen', 'aorta', 'stomach', 'gall_bladder', 'postcava',
               'adrenal_gland_left', 'adrenal_gland_right', 'esophagus', 'duodenum', 'colon', 'bladder', 'prostate', 'lung_left', 'lung_right'])
CLASSES = CLASSES_UFO + ['liver', 'pancreas', 'liver_lesion', 'pancreatic_lesion', 'kidney_lesion', 'femur_left', 'femur_right', 'hepatic_vessel',
                         'portal_vein_and_splenic_vein', 'celiac_trunk', 'superior_mesenteric_artery', 'veins', 'intestine', 'rectum']
assert len(CLASSES_UFO) == 28 and len(CLASSES) == 42


def _line(name, case, new, old, nbytes, **extra):
    gbps = nbytes / (new[0] * 1e-3) / 1e9
    out = {'metric': f'{name}: device times (median, min) ms', 'unit': 'ms', 'case': case, 'new_ms': new, 'algorithmic_bytes': int(nbytes),
           'new_GBps': gbps, 'share_of_measured_copy_6.29TBps': gbps / HBM_COPY_GBPS}
    if old is not None:
        out['aten_ms'], out['aten_over_new'] = old, old[0] / new[0]
    out.update(extra)
    LINES.append(out)
    print(json.dumps(out), flush=True)


def ellipsoid(size, centre, radii):
    z, y, x = (torch.arange(s, device='cuda', dtype=torch.float32) for s in size)
    return (((z - centre[0]) / radii[0]) ** 2)[:, None, None] + (((y - centre[1]) / radii[1]) ** 2)[None, :, None] \
        + (((x - centre[2]) / radii[2]) ** 2)[None, None, :] < 1.0


def synthetic_label(size, gen):
    """An abdomen by ellipsoids, scaled to the volume: a liver of about 0.62 x 0.59 x 0.49 of the extents cut into 8 segments by octants, with a few
    specks and a thin spur the opening removes; a pancreas in three parts; blocky noise for the other organs.  Packed as np.packbits(axis=0) would."""
    D, H, W = size
    C = len(CLASSES_UFO)
    packed = torch.zeros(((C + 7) // 8,) + tuple(size), dtype=torch.uint8, device='cuda')

    def put(name, m):
        c = CLASSES_UFO.index(name)
        packed[c >> 3] |= m.to(torch.uint8) << (7 - (c & 7))

    lc = (D * 0.5, H * 0.4, W * 0.36)
    liver = ellipsoid(size, lc, (D * 0.3125, H * 0.293, W * 0.244))
    z, y, x = (torch.arange(s, device='cuda') for s in size)
    for i in range(8):
        half = ((z >= lc[0]) == bool(i & 4))[:, None, None] & ((y >= lc[1]) == bool(i & 2))[None, :, None] & ((x >= lc[2]) == bool(i & 1))[None, None, :]
        put(LIVER[i], liver & half)
    speck = torch.zeros(size, dtype=torch.bool, device='cuda')
    speck[D - 6:D - 4, 4:6, W - 8:W - 6] = True
    speck[int(lc[0]), int(lc[1]), int(lc[2]):W - 4] = True
    put(LIVER[0], speck)
    for k, name in enumerate(PANCREAS):
        put(name, ellipsoid(size, (D * 0.55, H * 0.62 + k * H * 0.05, W * 0.55 + k * W * 0.07), (D * 0.05, H * 0.045, W * 0.045)))
    low = [-(-s // 8) for s in size]
    for name in CLASSES_UFO[12:]:
        m = (torch.rand(low, device='cuda', generator=gen) < 0.03).repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:D, :H, :W]
        put(name, m)
    return packed


def rows_for(organ, location):
    return [{'Standardized Organ': organ, 'Standardized Location': location, 'Tumor Size (mm)': '14 x 9'}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-scipy', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'report_crop_bench.json'))
    a = ap.parse_args()
    from rsuper_amd.hip import lib
    from rsuper_amd.inference.postprocess import keep_largest_component
    from rsuper_amd.training import augmentation as A
    from rsuper_amd.training.dataset import PackedBits, reports
    from rsuper_amd.training.dataset.whole_volume import large_size
    lib.require_device()
    gen = torch.Generator(device='cuda').manual_seed(0)
    Cu, C = len(CLASSES_UFO), len(CLASSES)
    Pu, P = (Cu + 7) // 8, (C + 7) // 8
    shifts = torch.arange(7, -1, -1, device='cuda', dtype=torch.uint8).view(1, 8, 1, 1, 1)
    crop = (96, 96, 96)
    v = crop[0] * crop[1] * crop[2]

    for name, size, segment, rows in (('pancreas_head', (400, 512, 512), ['head'], rows_for('pancreas', 'head')),
                                      ('liver', (400, 512, 512), 'liver', rows_for('liver', 'liver')),
                                      ('small_ct', (90, 160, 160), ['head'], rows_for('pancreas', 'head'))):
        D, H, W = size
        V = D * H * W
        img = torch.randn((1, 1) + size, device='cuda', generator=gen)
        packed = synthetic_label(size, gen)
        lab = PackedBits(packed[None], Cu)
        pad = large_size(*crop)
        full, lo = A.padded_size(size, pad)
        cset = reports.segment_class_set(segment, CLASSES_UFO)
        idx = reports._bits(cset)
        planes_touched = len({c >> 3 for c in idx})
        (count, box), = A._read_count_box(A.union_bbox(lab, [cset]))
        ext = [box[3 + i] - box[i] + 1 for i in range(3)]
        fits = A.bbox_fits(A.bbox_with_margin([b + lo[i % 3] for i, b in enumerate(box)], full, 1), crop)
        case = {'shape': list(size), 'padded': full, 'classes_ufo': Cu, 'classes': C, 'crop': list(crop), 'segment': segment, 'voxels': count,
                'box': ext, 'fits': fits, 'planes_read': planes_touched}
        tables = {}

        def remap(cl):
            present = A.class_counts(cl).host(0)[:Cu]
            if 't' not in tables:                                # the tables are a few hundred host operations: built once, as a loader would cache them
                ml, ol, mu, ou, _ = reports.assign_labels_tables(CLASSES, CLASSES_UFO, rows, present)
                _, chosen = reports.chosen_segment_table(CLASSES, segment, CLASSES_UFO)
                mc = [0] * C
                for j, m in enumerate(chosen):
                    for c in reports._bits(m):
                        mc[j] |= ml[c]
                tables['t'] = ([[ml, mu, mc]], [[ol, ou, 0]])
            return A.label_remap(cl, C, *tables['t'])

        def chain():
            out = A.crop_foreground_3d(img, lab, cset, crop, rand=False, pad=pad)
            if isinstance(out, str):
                return out
            return out[0], remap(out[1])

        def aten():
            inflated = ((packed[:, None] >> shifts) & 1).reshape((Pu * 8,) + size)[:Cu]
            m = torch.stack([inflated[i] for i in idx], 0).sum(0)
            m[m > 0] = 1
            if m.sum().item() == 0:
                raise AssertionError
            coords = torch.nonzero(m)
            bb = [coords[:, i].min().item() for i in range(3)] + [coords[:, i].max().item() for i in range(3)]
            corner = A.plan_crop_foreground([b + lo[i % 3] for i, b in enumerate(bb)], full, crop, rand=False)
            if isinstance(corner, str):
                return corner                                    # denoise_mask on the host comes next in the reference: timed on its own
            im, lb = img, inflated[None]
            if list(size) != full:
                pads = []
                for i in (2, 1, 0):
                    t = full[i] - size[i]
                    pads += [t // 2, t - t // 2]
                im, lb = torch.nn.functional.pad(im, pads), torch.nn.functional.pad(lb, pads)
            sl = (slice(None), slice(None)) + tuple(slice(c, c + n) for c, n in zip(corner, crop))
            im, lb = im[sl].contiguous(), lb[sl].contiguous()[0]
            zero = torch.zeros_like(lb[0])
            label, unk = [], []
            for clss in CLASSES:                                 # assign_labels' lists (:1241-1292) for a crop with a tumour segment of `segment`'s organ
                if clss in CLASSES_UFO:
                    label.append(lb[CLASSES_UFO.index(clss)])
                    unk.append(torch.zeros_like(zero))
                elif clss in ('liver', 'pancreas'):
                    acc = torch.zeros_like(zero)
                    for part in (LIVER if clss == 'liver' else PANCREAS):
                        acc = torch.logical_or(acc, lb[CLASSES_UFO.index(part)])
                    label.append(acc)
                    unk.append(torch.zeros_like(zero))
                elif 'lesion' not in clss:
                    label.append(torch.zeros_like(zero))
                    unk.append(torch.ones_like(zero))
                else:
                    label.append(torch.zeros_like(zero))
                    u = torch.zeros_like(zero)
                    if 'pancreatic' in clss and lb[CLASSES_UFO.index('pancreas_head')].max() > 0:
                        u[lb[CLASSES_UFO.index('pancreas_head')] > 0] = 1
                    unk.append(u)
            label, unk = torch.stack(label, 0), torch.stack(unk, 0).type_as(label[0])
            seg = torch.stack([label[CLASSES.index('pancreas_head')]], 0).sum(0)
            seg[seg > 0] = 1
            mask = torch.stack([seg if 'pancreatic_lesion' in c else torch.zeros_like(zero) for c in CLASSES], 0)
            return im, (label, unk, mask)

        new_out, old_out = chain(), aten()
        if fits:
            assert torch.equal(new_out[0], old_out[0]), 'the two sides cut different boxes'
            for got, exp in zip(new_out[1], old_out[1]):
                assert torch.equal(got.unpack()[0], exp.to(torch.uint8)), 'the two sides build different volumes'
        else:
            assert new_out == old_out == A.NO_FIT
        del new_out, old_out
        torch.cuda.empty_cache()

        b_bbox = planes_touched * V
        nwords = ext[0] * ext[1] * ((ext[2] + 63) // 64)
        b_open = 6 * 2 * nwords * 8 + nwords * 8 + ext[0] * ext[1] * ext[2]
        b_crop = (4 + Pu) * 2 * v
        b_remap = (Pu + 3 * P) * v
        new, old = _time_pair(chain, aten, a.reps)
        if fits:
            _line(name + '/chain', dict(case, launches=6, host_reads=2), new, old, b_bbox + b_crop + Pu * v + b_remap)
        else:
            _line(name + '/chain', dict(case, launches=2 + 1 + 7 + 2, host_reads=3), new, old, b_bbox + planes_touched * nwords * 64 + b_open,
                  note='launch count without the launches inside rsuper_largest_component; the ATen side ends where the reference goes to scipy')
        _line(name + '/bbox', dict(case, launches=2), _time_one(lambda: A.union_bbox(lab, [cset]), a.reps), None, b_bbox)
        sub = [box[0], box[1], box[2]] + ext
        bits = A.union_bits(lab, cset, sub)
        _line(name + '/bits', dict(case, launches=1), _time_one(lambda: A.union_bits(lab, cset, sub), a.reps), None, planes_touched * nwords * 64 + nwords * 8)
        _, opened, _ = A.bits_open(bits, ext[2], 3)
        _line(name + '/open', dict(case, launches=7, iterations=3), _time_one(lambda: A.bits_open(bits, ext[2], 3), a.reps), None, b_open)
        _line(name + '/component', dict(case), _time_one(lambda: keep_largest_component(opened), a.reps), None, 2 * ext[0] * ext[1] * ext[2])
        if fits:
            cl = A.crop_foreground_3d(img, lab, cset, crop, rand=False, pad=pad)[1]
            _line(name + '/remap', dict(case, launches=1, volumes=3), _time_one(lambda: A.label_remap(cl, C, *tables['t']), a.reps), None, b_remap)
        elif not a.no_scipy:
            try:
                from scipy.ndimage import binary_dilation, binary_erosion, label
            except ImportError:
                label = None
            if label is not None:
                m = np.zeros(size, bool)
                inflated = ((packed[:, None] >> shifts) & 1).reshape((Pu * 8,) + size)
                for i in idx:
                    m |= inflated[i].cpu().numpy().astype(bool)
                del inflated
                t0 = time.perf_counter()
                final = binary_dilation(binary_erosion(m, iterations=3), iterations=3) & m
                labeled, n = label(final)
                if n > 1:
                    counts = np.bincount(labeled.ravel())
                    counts[0] = 0
                    final = labeled == np.argmax(counts)
                dt = time.perf_counter() - t0
                same = bool(np.array_equal(final[box[0]:box[3] + 1, box[1]:box[4] + 1, box[2]:box[5] + 1],
                                           keep_largest_component(opened).cpu().numpy().astype(bool)))
                out = {'metric': name + '/scipy_open_s: denoise_mask(iterations=3) on the host over the whole CT, one run', 'unit': 's', 'case': case,
                       'scipy_open_s': dt, 'equal_to_device': same}
                LINES.append(out)
                print(json.dumps(out), flush=True)
        del img, packed, lab, bits, opened
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for ln in LINES:
            f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
