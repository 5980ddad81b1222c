"""python -m rsuper_amd.tools.pack_dataset --src DIR --dst DIR

One-time conversion of a directory written by the reference's dataset_conversion/nii2npz.py (`<id>.npz` float32 image, `<id>_gt.npz` unpacked int8
(C, D, H, W) label, both savez_compressed, `list/label_names.yaml`) to files a DataLoader worker can memory-map: `<id>.npy` (the image, uncompressed)
and `<id>_gt.npy` (the label as np.packbits(axis=0), 1/8 of the bytes before compression).  The label is packed on the device (upload_label: z-slabs
through pinned staging buffers, rsuper_pack_bits) and read back.  `list/label_names.yaml` is copied.  The result is still a directory the reference's
dataset reads: it accepts .npy files and bit-packed labels (dataset_abdomenatlas_UFO.py:249-261, :465-470).  .npy inputs are converted the same way.
"""
import argparse
import os
import shutil
import sys

import numpy as np


def convert(src, dst, device='cuda', chunk_bytes=None, log=None):
    import torch
    from ..hip import lib as _l
    from ..training.dataset import packed, whole_ct
    _l.require_device()
    os.makedirs(os.path.join(dst, 'list'), exist_ok=True)
    shutil.copyfile(os.path.join(src, 'list', 'label_names.yaml'), os.path.join(dst, 'list', 'label_names.yaml'))
    C = len(whole_ct.read_label_names(src))
    done = []
    for name in whole_ct.scan_root(src):
        img_path, lab_path = whole_ct.case_paths(src, name)
        img = np.asarray(whole_ct.load_array(img_path))
        lab = packed.upload_label(whole_ct.load_array(lab_path), C, device, packed.UPLOAD_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        out = lab.packed[0].cpu().numpy()
        np.save(os.path.join(dst, name + '.npy'), img)
        np.save(os.path.join(dst, name + '_gt.npy'), out)
        done.append(name)
        if log:
            log('%s: image %s %s, label %s -> %s' % (name, img.dtype, img.shape, (C,) + img.shape, out.shape))
        del lab
    torch.cuda.synchronize()
    return done


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[1])
    p.add_argument('--src', required=True, help='directory written by nii2npz.py')
    p.add_argument('--dst', required=True, help='directory to write (created)')
    p.add_argument('--chunk_bytes', type=int, default=None, help='unpacked label bytes per staged z-slab (default: packed.UPLOAD_CHUNK_BYTES)')
    a = p.parse_args(argv)
    done = convert(a.src, a.dst, chunk_bytes=a.chunk_bytes, log=lambda m: print(m, file=sys.stderr, flush=True))
    print('converted %d cases into %s' % (len(done), a.dst))


if __name__ == '__main__':
    main()
