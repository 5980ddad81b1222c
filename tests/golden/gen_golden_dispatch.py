"""The 3x3x3 igemm dispatch table: block width and statistics rows of every launch shape the host queries answer for.

The queries are pure host functions (the library loads without a GPU; rsuper_conv3_set_workspace only stores the pointer, so a
dummy non-null pointer exercises the 6^3 split shape).  `table()` goes through functions that exist before and after the dispatch
became one plan function (ops.pick_bn and the exported C queries), so the committed dispatch_table.npz -- generated at the commit
it records -- pins the answers for every later tree: tests/test_dispatch_cpu.py recomputes it and requires equality row for row.

    python tests/golden/gen_golden_dispatch.py [commit]     # rewrites tests/golden/dispatch_table.npz from the current checkout
                                                            # (commit: for a tree exported without its .git)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

VARIANTS = (0, 1, 2, 3, 4, 6, 7, 8)
DTYPES = (torch.float32, torch.bfloat16)
DIMS = [(2, 96, 96, 96), (2, 48, 48, 48), (2, 24, 24, 24), (2, 12, 12, 12), (2, 6, 6, 6), (1, 96, 96, 96), (8, 24, 24, 24),
        (2, 5, 7, 19), (1, 3, 3, 3), (4, 6, 6, 6), (2, 64, 48, 80), (16, 12, 12, 12)]
COLS = [8, 24, 32, 40, 64, 96, 128, 160, 192, 256, 320, 512, 640]
# stride 2: full-resolution volumes, (Ca, Cb) source channels, columns
S2_DIMS = [(2, 96, 96, 96), (2, 48, 48, 48), (1, 24, 24, 24), (2, 13, 9, 21), (2, 6, 6, 6), (4, 12, 12, 12), (4, 162, 162, 162), (1, 2, 2, 4100)]
S2_SRC = [(32, 0), (16, 0), (24, 0), (8, 8), (64, 64), (32, 32), (48, 16), (520, 0), (1024, 1024)]
S2_COLS = [16, 32, 64, 128, 256, 640]
DUMMY_WS = 0x1000


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def table():
    """{'s1': (ws, variant, dtype, epi (-1: not given), mixed, volume index, columns, bn, rows(epi 0), rows(epi 1)),
        'nodims': (variant, dtype, columns, bn), 'notiles': (variant, dtype, epi, mixed, volume index, columns, bn) for pick_bn with the volume but no tile count,
        's2': (S2K on, S2D on, dtype, mode, Ca, Cb, volume index, columns, rows)} as int32 arrays.
    Leaves the library as it found it (variant, workspace, environment)."""
    from rsuper_amd.hip import lib, ops
    L = ops._L()                                  # on a GPU box this registers the real workspace first; restored below
    var0 = L.rsuper_conv3_variant(-1)
    env0 = {k: os.environ.get(k) for k in ('RSUPER_S2K', 'RSUPER_S2D')}
    s1, nodims, notiles, s2 = [], [], [], []
    try:
        for ws in (0, 1):
            L.rsuper_conv3_set_workspace(ctypes.c_void_p(DUMMY_WS if ws else None), L.rsuper_conv3_workspace_bytes() if ws else 0)
            for var in VARIANTS:
                L.rsuper_conv3_variant(var)
                for di, dt in enumerate(DTYPES):
                    for epi in (None, 0, 1):
                        for mixed in (False, True):
                            for vi, dims in enumerate(DIMS):
                                tiles = L.rsuper_conv3_tiles(*dims[1:]) * dims[0]
                                for nc in COLS:
                                    bn = ops.pick_bn(nc, dt, tiles, dims, epi=epi, mixed=mixed)
                                    r = [L.rsuper_conv3_part_rows(ops._DT[dt], e, *dims, nc, bn, int(mixed)) for e in (0, 1)]
                                    s1.append((ws, var, di, -1 if epi is None else epi, int(mixed), vi, nc, bn, r[0], r[1]))
        for var in VARIANTS:
            L.rsuper_conv3_variant(var)
            for di, dt in enumerate(DTYPES):
                for nc in COLS:
                    nodims.append((var, di, nc, ops.pick_bn(nc, dt)))
                    for epi in (0, 1):
                        for mixed in (False, True):
                            for vi, dims in enumerate(DIMS):
                                notiles.append((var, di, epi, int(mixed), vi, nc, ops.pick_bn(nc, dt, dims=dims, epi=epi, mixed=mixed)))
        for k in (1, 0):
            _setenv('RSUPER_S2K', None if k else '0')
            for d in (1, 0):
                _setenv('RSUPER_S2D', None if d else '0')
                for di, dt in enumerate(DTYPES):
                    for mode in (1, 2):
                        for Ca, Cb in S2_SRC:
                            for vi, dims in enumerate(S2_DIMS):
                                for nc in S2_COLS:
                                    s2.append((k, d, di, mode, Ca, Cb, vi, nc, L.rsuper_conv3_s2_part_rows(ops._DT[dt], mode, Ca, Cb, nc, *dims)))
    finally:
        L.rsuper_conv3_variant(var0)
        for k, v in env0.items():
            _setenv(k, v)
        if ops._WS is not None:
            L.rsuper_conv3_set_workspace(ops._WS.data_ptr(), ops._WS.numel())
        else:
            L.rsuper_conv3_set_workspace(None, 0)
    return {'s1': np.array(s1, dtype=np.int32), 'nodims': np.array(nodims, dtype=np.int32), 'notiles': np.array(notiles, dtype=np.int32),
            's2': np.array(s2, dtype=np.int32)}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    if len(sys.argv) > 1:
        commit, dirty = sys.argv[1], False
    else:
        commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], text=True).strip()
        dirty = bool(subprocess.check_output(['git', '-C', ROOT, 'status', '--porcelain', '--', 'r-super_amd', 'include'], text=True).strip())
    t = table()
    out = os.path.join(HERE, 'dispatch_table.npz')
    np.savez_compressed(out, commit=np.array(commit + ('+dirty' if dirty else '')), **t)
    print(out, {k: v.shape for k, v in t.items()}, commit, 'dirty' if dirty else 'clean')
