#!/usr/bin/env python3
"""The distinct C-ABI calls one MedFormer training step (tools/medformer_step.py: shipped config, 96^3, B = 2) makes into the pointwise / depthwise /
channel-norm family, as rows for tests/golden/gen_golden_mf_launches.py (STEP).  Usage: python tools/mf_step_shapes.py OUT.json [dtype]"""
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rsuper_amd.hip import ops  # noqa: E402

# entry point -> (row name, indices of the shape arguments); flags say which optional operands were given
ENTRY = {
    'rsuper_pointwise': ('pw', (0, 1, 10, 11, 12), (4, 5, 6)),                   # dtype, mode, R, K, N; w, bias, res
    'rsuper_pointwise_wgrad': ('pw_wgrad', (0, 5, 6, 7), (11,)),                # dtype, R, N, K; db
    'rsuper_pointwise_pack_batch': ('pw_pack_batch', (0, 2, 3), ()),            # dtype, n, items
    'rsuper_cnorm_forward': ('cnorm_fwd', (4, 5, 6, 7), ()),                    # N, vox, C, relu
    'rsuper_cnorm_backward': ('cnorm_bwd', (6, 7, 8, 9), ()),
    'rsuper_cnorm_stats': ('cnorm_stats', (4, 5, 6, 7, 8), ()),                 # N, vox, C, relu, mode
    'rsuper_cnorm_apply': ('cnorm_apply', (5, 6, 7, 8, 9), ()),
    'rsuper_se_forward': ('se_fwd', (10, 11, 12, 13), ()),                      # N, vox, C, r
    'rsuper_se_backward': ('se_bwd', (17, 18, 19, 20), ()),
    'rsuper_cl_planar': ('cl_planar', (2, 3, 4, 5, 6), ()),                     # N, vox, C, K, dir
    'rsuper_depthwise3_fwd': ('dw', (3, 4, 5, 6, 7, 8), ()),                    # N, D, H, W, C, flip
    'rsuper_depthwise3_wgrad': ('dw_wgrad', (4, 5, 6, 7, 8), ()),
}
SMALL = {0: 'cnorm_fwd', 1: 'cnorm_bwd'}      # rsuper_cnorm_small by mode, where the module still calls it itself: N, vox, C, relu


class Tap:
    def __init__(self, L, seen):
        self.L, self.seen = L, seen

    def __getattr__(self, name):
        f = getattr(self.L, name)
        if name == 'rsuper_cnorm_small':
            def g(*a):
                self.seen[(SMALL[a[10]], a[5], a[6], a[7], a[8])] = self.seen.get((SMALL[a[10]], a[5], a[6], a[7], a[8]), 0) + 1
                return f(*a)
            return g
        if name not in ENTRY:
            return f
        row, idx, flags = ENTRY[name]

        def g(*a):
            k = (row,) + tuple(int(a[i]) for i in idx) + tuple(int(a[i] is not None) for i in flags)
            self.seen[k] = self.seen.get(k, 0) + 1
            return f(*a)
        return g


if __name__ == '__main__':
    out, dtype = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else 'bf16'
    seen, real = {}, ops._L
    ops._L = lambda: Tap(real(), seen)
    sys.argv = ['medformer_step.py', '1', dtype]
    runpy.run_path(os.path.join(ROOT, 'tools', 'medformer_step.py'), run_name='__main__')
    rows = sorted(seen)
    json.dump([list(r) + [seen[r]] for r in rows], open(out, 'w'))
    print(f'{len(rows)} distinct calls, {sum(seen.values())} calls in 5 steps -> {out}')
