#!/usr/bin/env python3
"""tests/golden/glue_launches.json: the launches of the bandwidth-bound glue kernels (csrc/unet_misc.hip: InstanceNorm backward tail, max pool,
stride-2 subsample, trilinear up-sampling) as a kernel trace recorded them, one row per C-ABI call.  The table was recorded on the commit BEFORE
csrc/glue_plan.hpp existed (its hash is in the file), where the decisions were visible as launches only; tests/test_glue_plan_cpu.py asserts that
rsuper_glue_plan reproduces kernel, template arguments, blocks and threads of every row without a GPU.

ROWS reaches every rung of the dispatch at the smallest shape that does (the rungs beyond 32-bit offsets need tensors of 4 GB and are pinned by
the CPU test from the limits themselves).  Every row runs under the default kernels and again under rsuper_glue_variant(0).

Three steps (an MI355X for the first):
    rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python tests/golden/gen_golden_glue_launches.py drive --root TREE --out rows.json
    python tests/golden/gen_golden_glue_launches.py table DIR rows.json COMMIT -o tests/golden/glue_launches.json
    python tests/golden/gen_golden_glue_launches.py compare A.json B.json        # two trees: same launches, row for row
`drive` issues exactly one C-ABI call per row on NaN-prefilled outputs (and fails if a NaN is left), `table` joins the trace's glue-kernel
launches, in order, with the rows that launched."""
import argparse
import csv
import glob
import json
import os
import re
import sys

# the __global__ functions of the family (the trace holds torch's own kernels and the zero fill of odd-sized pooling gradients too)
FAMILY = ('in_bwd_finalize_kernel', 'in_bwd_finalize2_kernel', 'maxpool_fwd_kernel', 'maxpool_fwd2_kernel', 'maxpool_bwd_kernel',
          'subsample_fwd_kernel', 'subsample_bwd_kernel', 'upsample_fwd_kernel', 'upsample_fwd2_kernel', 'upsample_fwd3_kernel',
          'upsample_bwd_kernel', 'upsample_bwd2_kernel', 'upsample_bwd4_kernel')

STEP_POOL = [(2, (96, 96, 96), 32), (2, (48, 48, 48), 64), (2, (24, 24, 24), 128), (2, (12, 12, 12), 256)]
STEP_UP = [(2, (48, 48, 48, 96, 96, 96), 64), (2, (24, 24, 24, 48, 48, 48), 128), (2, (12, 12, 12, 24, 24, 24), 256), (2, (6, 6, 6, 12, 12, 12), 320)]
SPLIT = [(2, (S, S, S), C) for S in (24, 12) for C in (128, 256, 320)]      # channel split of the statistics-row kernels
SMALL = [(1, (7, 9, 11), 8), (1, (6, 10, 14), 8), (3, (10, 6, 14), 320)]

ROWS = []      # (op, dtype, N, shape, C); shape: (vox,), the input's (D, H, W), or (ID, IH, IW, OD, OH, OW)
# InstanceNorm backward tail: the step's shapes of tests/test_gpu_glue_kernels.py ...
ROWS += [('in_bwd', 'bf16', 2, (v,), C) for v, C in ((96 ** 3, 32), (48 ** 3, 64), (48 ** 3, 128), (24 ** 3, 128), (24 ** 3, 256), (12 ** 3, 256),
                                                     (12 ** 3, 320), (6 ** 3, 320))]
ROWS += [('in_bwd', 'bf16', 1, (7 * 9 * 11,), 8), ('in_bwd', 'bf16', 3, (37 * 41 * 43,), 16),
         ('in_bwd', 'f32', 2, (48 ** 3,), 64), ('in_bwd', 'f32', 2, (24 ** 3,), 128), ('in_bwd', 'f32', 1, (7 * 9 * 11,), 8)]
# ... 255 | 256, 1023 | 1024, 8192 | 8193 blocks' worth of vectors, and vector counts per voxel that are no power of two
ROWS += [('in_bwd', 'bf16', 1, (v,), 8) for v in (65280, 65281, 261888, 261889, 2097152, 2097153)]
ROWS += [('in_bwd', 'bf16', 1, (48 ** 3,), 24), ('in_bwd', 'bf16', 1, (24 ** 3,), 320)]
# max pool: step, ragged and f32 shapes; 1008 | 1024 rows forward, 496 | 512 blocks backward; the channel split
POOL = [('bf16',) + r for r in STEP_POOL + SMALL] + [('f32', 2, (24, 24, 24), 128), ('f32', 2, (12, 12, 12), 256), ('f32', 1, (7, 9, 11), 8)]
POOL += [('bf16', 1, (126, 64, 64), 8), ('bf16', 1, (128, 64, 64), 8), ('bf16', 1, (128, 128, 62), 8), ('bf16', 1, (128, 128, 64), 8)]
POOL += [('bf16',) + r for r in SPLIT if r not in STEP_POOL]
ROWS += [(op, dt, N, s, C) for dt, N, s, C in POOL for op in ('pool_fwd', 'pool_bwd')]
# subsample: the same small and split cases
SUB = [('bf16',) + r for r in STEP_POOL[1:] + SMALL[:1]] + [('f32', 2, (12, 12, 12), 256), ('f32', 1, (7, 9, 11), 8)]
SUB += [('bf16',) + r for r in SPLIT if r not in STEP_POOL]
ROWS += [(op, dt, N, s, C) for dt, N, s, C in SUB for op in ('sub_fwd', 'sub_bwd')]
# trilinear forward: step, ragged, f32; the per-axis table stops fitting 64 KB next to the statistics scratch between 3070 and 3071 outputs
ROWS += [('up_fwd', 'bf16') + r for r in STEP_UP] + [('up_fwd', 'bf16', 1, (3, 5, 4, 7, 9, 11), 8), ('up_fwd', 'bf16', 1, (5, 1, 7, 5, 4, 7), 8)]
ROWS += [('up_fwd', 'f32') + r for r in STEP_UP[1:]] + [('up_fwd', 'f32', 1, (3, 5, 4, 7, 9, 11), 8)]
ROWS += [('up_fwd', 'bf16', 1, (1, 1, 1536, 1, 1, 3070), 8), ('up_fwd', 'bf16', 1, (1, 1, 1536, 1, 1, 3071), 8)]
# trilinear backward: step (NT = 4), a ragged scale (NT = 6), f32 (gather kernel), 4x (refused by the row-sharing kernel's tile tables),
# and a scale above 5 that no kernel takes
ROWS += [('up_bwd', 'bf16') + r for r in STEP_UP] + [('up_bwd', 'bf16', 1, (3, 5, 4, 7, 9, 11), 8), ('up_bwd', 'f32', 2, (12, 12, 12, 24, 24, 24), 256),
                                                     ('up_bwd', 'bf16', 2, (6, 6, 6, 24, 24, 24), 8), ('up_bwd', 'bf16', 1, (4, 4, 4, 24, 24, 24), 8)]
UNSUPPORTED = 3      # RSUPER_ERR_UNSUPPORTED


def drive(root, out):
    sys.path.insert(0, root)
    import torch
    from rsuper_amd.hip import lib, ops
    lib.require_device()
    L, dev = ops._L(), 'cuda'
    dts = {'f32': torch.float32, 'bf16': torch.bfloat16}

    def rnd(shape, dt, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.randn(shape, generator=g, device=dev, dtype=torch.float32).to(dt)

    def nan(shape, dt):
        return torch.full(shape, float('nan'), device=dev, dtype=dt)

    def one(op, mode, N, s, C):
        """exactly one C-ABI call; returns (return code, outputs)"""
        dt = dts[mode]
        d, st = ops._DT[dt], ops._stream()
        if op == 'in_bwd':
            g, x, o = rnd((N, s[0], C), dt, 1), rnd((N, s[0], C), dt, 2), nan((N, s[0], C), dt)
            mr, gm = torch.ones((N, C, 2), device=dev), torch.zeros((N, C, 2), device=dev)
            return L.rsuper_in_bwd_finalize(d, ops._ptr(g), C, ops._ptr(x), C, ops._ptr(mr), ops._ptr(gm), None, C, None, C, ops._ptr(o), C, N, s[0], C, st), [o]
        if op in ('pool_fwd', 'pool_bwd', 'sub_fwd', 'sub_bwd'):
            D, H, W = s
            O = tuple(v // 2 for v in s) if op.startswith('pool') else tuple((v + 1) // 2 for v in s)
            x = rnd((N, D, H, W, C), dt, 3)
            if op.endswith('fwd'):
                blocks = ops._stat_blocks(O[0] * O[1] * O[2])
                y, part = nan((N,) + O + (C,), dt), nan((N, blocks, C, 2), torch.float32)
                f = L.rsuper_maxpool2_fwd if op == 'pool_fwd' else L.rsuper_subsample2_fwd
                return f(d, ops._ptr(x), C, ops._ptr(y), C, ops._ptr(part), blocks, N, D, H, W, C, st), [y, part]
            dy, dx = rnd((N,) + O + (C,), dt, 4), nan((N, D, H, W, C), dt)
            if op == 'pool_bwd':
                return L.rsuper_maxpool2_bwd(d, ops._ptr(x), C, ops._ptr(dy), C, ops._ptr(dx), C, N, D, H, W, C, st), [dx]
            return L.rsuper_subsample2_bwd(d, ops._ptr(dy), C, ops._ptr(dx), C, N, D, H, W, C, st), [dx]
        I, O = tuple(s[:3]), tuple(s[3:])
        if op == 'up_fwd':
            blocks = ops._stat_blocks(O[0] * O[1] * O[2])
            x, y, part = rnd((N,) + I + (C,), dt, 5), nan((N,) + O + (C,), dt), nan((N, blocks, C, 2), torch.float32)
            return L.rsuper_upsample_fwd(d, ops._ptr(x), C, ops._ptr(y), C, ops._ptr(part), blocks, N, *I, *O, C, st), [y, part]
        dy, dx = rnd((N,) + O + (C,), dt, 6), nan((N,) + I + (C,), dt)
        return L.rsuper_upsample_bwd(d, ops._ptr(dy), C, ops._ptr(dx), C, N, *I, *O, C, st), [dx]

    done = []
    for variant in (1, 0):
        assert L.rsuper_glue_variant(variant) == variant
        for op, mode, N, s, C in ROWS:
            rc, outs = one(op, mode, N, s, C)
            torch.cuda.synchronize()
            assert rc in (0, UNSUPPORTED), (op, mode, N, s, C, variant, rc)
            if rc == 0:
                assert not any(bool(torch.isnan(o.float()).any()) for o in outs), ('NaN (unwritten output)', op, mode, N, s, C, variant)
            done.append({'op': op, 'dtype': mode, 'N': N, 'shape': list(s), 'C': C, 'variant': variant, 'rc': rc})
            del outs
    L.rsuper_glue_variant(1)
    json.dump(done, open(out, 'w'))
    print(f'{len(done)} calls, {sum(r["rc"] == 0 for r in done)} launched')


def launches(trace_dir):
    """the family's launches of a rocprofv3 kernel trace, in start order: (name with template arguments, blocks, workgroup, LDS bytes)"""
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    assert len(files) == 1, files
    got = []
    for r in csv.DictReader(open(files[0])):
        name = re.sub(r'^void ', '', r['Kernel_Name'].replace('(anonymous namespace)::', ''))
        name = name[:name.index('(')] if '(' in name else name
        if name.split('<')[0] not in FAMILY:
            continue
        wg = [int(r['Workgroup_Size_' + a]) for a in 'XYZ']
        grid = [int(r['Grid_Size_' + a]) // w for a, w in zip('XYZ', wg)]
        got.append((int(r['Start_Timestamp']), name, grid, wg[0], int(r['LDS_Block_Size'])))
        assert wg[1] == wg[2] == 1
    return [g[1:] for g in sorted(got)]


def table(trace_dir, rows_json, commit, out):
    rows, ls = json.load(open(rows_json)), launches(trace_dir)
    assert len(rows) == 2 * len(ROWS) and len(ls) == sum(r['rc'] == 0 for r in rows), (len(rows), len(ls))
    it = iter(ls)
    for r in rows:
        r['kernel'], r['blocks'], r['threads'], r['lds'] = next(it) if r['rc'] == 0 else (None, None, None, None)
    with open(out, 'w') as f:
        f.write('{"commit": "%s",\n "columns": ["op", "dtype", "N", "shape", "C", "variant", "rc", "kernel", "blocks", "threads", "lds"],\n "rows": [\n' % commit)
        f.write(',\n'.join('  ' + json.dumps([r[k] for k in ('op', 'dtype', 'N', 'shape', 'C', 'variant', 'rc', 'kernel', 'blocks', 'threads', 'lds')]) for r in rows))
        f.write('\n ]}\n')
    print(f'{out}: {len(rows)} rows, {len(ls)} launches, {len(set(l[0] for l in ls))} kernel instantiations')


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    diff = [(x, y) for x, y in zip(A['rows'], B['rows']) if x != y]
    for x, y in diff:
        print('differs:\n  ', x, '\n  ', y)
    print(f'{a} ({A["commit"]}) vs {b} ({B["commit"]}): {len(A["rows"])} / {len(B["rows"])} rows, {len(diff)} differ')
    return 1 if diff or len(A['rows']) != len(B['rows']) else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('drive'); p.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))); p.add_argument('--out', required=True)
    p = sub.add_parser('table'); p.add_argument('trace_dir'); p.add_argument('rows'); p.add_argument('commit'); p.add_argument('-o', required=True)
    p = sub.add_parser('compare'); p.add_argument('a'); p.add_argument('b')
    a = ap.parse_args()
    sys.exit(drive(a.root, a.out) if a.cmd == 'drive' else table(a.trace_dir, a.rows, a.commit, a.o) if a.cmd == 'table' else compare(a.a, a.b))
