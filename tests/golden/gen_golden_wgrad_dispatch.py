"""The 3x3x3 weight-gradient dispatch table: split count and kernel of every launch shape the host answers for.

The counts go through functions that exist before and after the decision became one plan function (rsuper_conv3_wgrad_splits,
rsuper_conv3_wgrad_s2_splits, rsuper_conv3_wgrad2_min_tiles), so the committed wgrad_dispatch_table.npz -- generated at the commit it
records, the last one with the decision spread over api.hip and three launchers -- pins them for every later tree.  That commit cannot be
asked on a CPU which KERNEL it runs: `parent_kernel` restates its launch ladder (launch_wgrad_impl / rs_launch_wgrad2 / rs_wgrad_sv_splits of
that commit) in Python, and the table stores the restatement's answer next to each count.  The restatement also derives the count; `table()`
requires that it equals the library's, row for row, so a table is only ever written from a restatement the recorded commit agrees with.
tests/test_dispatch_cpu.py recomputes the table and compares the plan with it.

    python tests/golden/gen_golden_wgrad_dispatch.py [commit]   # rewrites tests/golden/wgrad_dispatch_table.npz from the current checkout
                                                                # (commit: the hash to record -- a tree without its .git, or a rerun on a later tree,
                                                                # which reproduces the file byte for byte)
"""
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

F32, BF16 = 0, 1
TILE, WGRAD2, SV = 0, 1, 2                        # plan[0] of rsuper_conv3_wgrad_plan (RS_WGRAD_TILE / _2 / _SV in csrc/kernels.hpp)
SWITCHES = ('RSUPER_WGRAD_SV', 'RSUPER_WGRAD_SV_MAX', 'RSUPER_WGRAD2', 'RSUPER_WGRAD2_MIN_TILES',
            'RSUPER_WG2_MT1', 'RSUPER_WG2_MT1_MAXM', 'RSUPER_WG2_MT1_MIN_TILES')
THRESHOLDS = (12, 0, 1 << 20)                     # rsuper_conv3_wgrad2_min_tiles: the default, "always", "never"
BATCHES = (1, 2, 4, 33)                           # 33: beyond the second-generation kernel's per-sample table
VOLUMES = [(96, 96, 96), (48, 48, 48), (24, 24, 24), (12, 12, 12), (6, 6, 6), (3, 3, 3), (1, 1, 1), (8, 8, 16), (5, 7, 9), (13, 11, 17)]
X_CH = [(8, 0), (32, 0), (64, 0), (320, 0), (16, 16), (32, 64), (256, 256)]
Y_ROWS = [(8, 0), (32, 0), (40, 0), (64, 0), (128, 0), (320, 0), (16, 16), (48, 16), (32, 32), (256, 256)]
MODES = ((0, 0), (0, 1), (1, 0), (1, 1))          # (use_tr, mixed sources): the kernel columns of a row, in this order
SV_LDS_MAX = 158 * 1024


def _tiles(N, D, H, W):
    return N * ((D + 3) // 4) * ((H + 3) // 4) * ((W + 15) // 16)


def _config(dt, Mtot, tiles):
    return 0 if Mtot <= 32 else 2 if dt == BF16 and tiles >= 128 else 1


def _mt1(dt, Mtot, tiles):
    return dt == BF16 and Mtot == 64 and 512 <= tiles < 2048


def _sv_parts(N, D, H, W, nch, Mtot):
    """sv_geometry of conv3d_wgrad_sv.hip: depth parts per sample (0: no slab fits LDS)."""
    parts, mg = 0, (Mtot + 31) // 32
    for P in range(1, D + 1):
        dr = (D + P - 1) // P
        if (P - 1) * dr >= D:
            continue
        rx, ry = (dr + 2) * (H + 2) * (W + 2), dr * H * W
        nks = (ry + 15) // 16
        if 64 * (rx + nks * 16) + 4 * nks * 16 + 1024 > SV_LDS_MAX:
            continue
        parts = P
        if nch * mg * N * P >= 192 or dr <= 2:
            break
    return parts


def _sv_splits(dt, thr, Mtot, Ya, nch, N, D, H, W):
    if dt != BF16 or thr == 0 or thr >= (1 << 20):
        return 0
    if _tiles(N, D, H, W) > 64 or (Ya < Mtot and Ya % 32):
        return 0
    if D * H * W > 216 and Mtot * nch > 4096:
        return 0
    return N * _sv_parts(N, D, H, W, nch, Mtot)


def parent_splits(dt, thr, Ca, Cb, Ya, Yb, N, D, H, W):
    """rsuper_conv3_wgrad_splits of the recorded commit, every switch at its default."""
    nch, Mtot, tiles = (Ca + 31) // 32 + (Cb + 31) // 32, Ya + Yb, _tiles(N, D, H, W)
    sv = _sv_splits(dt, thr, Mtot, Ya, nch, N, D, H, W)
    if sv:
        return sv
    cfg = _config(dt, Mtot, tiles)
    gy = 1 if cfg == 0 else (3 if cfg == 1 else 1) * ((Mtot + 63) // 64)
    if _mt1(dt, Mtot, tiles):
        gy = Mtot // 32
    return max(1, min((512 if cfg == 1 else 256) // (nch * gy), tiles))


def parent_kernel(dt, thr, use_tr, mixed, Ca, Cb, Ya, Yb, N, D, H, W, splits):
    """(kernel, configuration, 32-row groups per block) of launch_wgrad_impl at the recorded commit for a launch with `splits` slabs.
    mixed: one normalised and one raw x source (the last line of rs_wgrad2_supported)."""
    nch, Mtot, tiles = (Ca + 31) // 32 + (Cb + 31) // 32, Ya + Yb, _tiles(N, D, H, W)
    cfg = _config(dt, Mtot, tiles)
    tile = (TILE, cfg, 1 if cfg == 0 else 2)
    if dt == F32 or not use_tr:
        return tile
    sv = _sv_splits(dt, thr, Mtot, Ya, nch, N, D, H, W)
    if sv > 0 and sv == splits:
        return (SV, cfg, 1)
    if cfg != 1 and tiles >= thr * splits and N <= 32 and not (Yb > 0 and Ya % 32) and not mixed:
        return (WGRAD2, cfg, 1 if Mtot <= 32 or _mt1(dt, Mtot, tiles) else 2)
    return tile


def table():
    """{'s1': (dtype, threshold, N, volume index, Ca, Cb, Ya, Yb, splits, then (kernel, configuration, row groups) for each of MODES),
        's2': (dtype, N, volume index, Ca, Mtot, splits) of the stride-2 weight gradient} as int32 arrays.
    Leaves the threshold as it found it."""
    assert not [k for k in SWITCHES if k in os.environ], 'the table is defined with every weight-gradient switch unset'
    from rsuper_amd.hip import lib
    L = lib.lib()
    thr0 = L.rsuper_conv3_wgrad2_min_tiles(-1)
    assert thr0 == THRESHOLDS[0]
    s1, s2 = [], []
    try:
        for dt in (F32, BF16):
            for thr in THRESHOLDS:
                assert L.rsuper_conv3_wgrad2_min_tiles(thr) == thr
                for N in BATCHES:
                    for vi, (D, H, W) in enumerate(VOLUMES):
                        for Ca, Cb in X_CH:
                            for Ya, Yb in Y_ROWS:
                                s = L.rsuper_conv3_wgrad_splits(dt, Ca, Cb, Ya, Yb, N, D, H, W)
                                assert s == parent_splits(dt, thr, Ca, Cb, Ya, Yb, N, D, H, W), (dt, thr, N, D, H, W, Ca, Cb, Ya, Yb, s)
                                row = [dt, thr, N, vi, Ca, Cb, Ya, Yb, s]
                                for use_tr, mixed in MODES:
                                    row += parent_kernel(dt, thr, use_tr, mixed, Ca, Cb, Ya, Yb, N, D, H, W, s)
                                s1.append(row)
            for N in BATCHES:
                for vi, (D, H, W) in enumerate(VOLUMES):
                    for Ca in sorted({a + b for a, b in X_CH}):
                        for Mtot in sorted({a + b for a, b in Y_ROWS}):
                            s2.append((dt, N, vi, Ca, Mtot, L.rsuper_conv3_wgrad_s2_splits(dt, Ca, Mtot, N, D, H, W)))
    finally:
        L.rsuper_conv3_wgrad2_min_tiles(thr0)
    return {'s1': np.array(s1, dtype=np.int32), 's2': np.array(s2, dtype=np.int32)}


def save(path, arrays):
    """An .npz whose bytes depend on the arrays alone (np.savez stamps every member with the current time)."""
    with zipfile.ZipFile(path, 'w') as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    if len(sys.argv) > 1:
        commit, dirty = sys.argv[1], False
    else:
        commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], text=True).strip()
        dirty = bool(subprocess.check_output(['git', '-C', ROOT, 'status', '--porcelain', '--', 'r-super_amd', 'include'], text=True).strip())
    t = table()
    out = os.path.join(HERE, 'wgrad_dispatch_table.npz')
    save(out, dict(commit=np.array(commit + ('+dirty' if dirty else '')), **t))
    print(out, {k: v.shape for k, v in t.items()}, commit, 'dirty' if dirty else 'clean')
