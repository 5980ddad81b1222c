#!/usr/bin/env python3
"""tests/golden/mf_launches.json: the launches of the kernels MedFormer's attention stages run on (csrc/pointwise.hip, depthwise.hip, instnorm.hip) as a
kernel trace recorded them, one row per C-ABI call (a call is one to five launches).  The table was recorded on the commit BEFORE csrc/mf_plan.hpp
existed (its hash is in the file), where the decisions were visible as launches only -- and the one-launch channel norm was chosen in hip/ops.py;
tests/test_mf_plan_cpu.py asserts that rsuper_mf_plan reproduces kernel, template arguments, blocks and threads of every launch without a GPU.

ROWS reaches every rung of the dispatch at the smallest shape that does, and holds every distinct call of one MedFormer training step (shipped
config, 96^3, B = 2, bf16: STEP, from tools/mf_step_shapes.py).

Three steps (an MI355X for the first):
    rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python tests/golden/gen_golden_mf_launches.py drive --root TREE --out rows.json
    python tests/golden/gen_golden_mf_launches.py table DIR rows.json COMMIT -o tests/golden/mf_launches.json
    python tests/golden/gen_golden_mf_launches.py compare A.json B.json        # two trees: same launches, row for row
`drive` issues exactly one C-ABI call per row on NaN-prefilled outputs (and fails if a NaN is left) and a marker kernel after it; `table` cuts the
trace's family launches at the markers and joins them with the rows."""
import argparse
import csv
import glob
import json
import os
import re
import sys

# the __global__ functions of the family, in the order of lib.MF_KERNELS
FAMILY = ('pw_pack_kernel', 'pw_pack_batch_kernel', 'pw_gemm_kernel', 'pw_wgrad_kernel', 'pw_wgrad_reduce_kernel', 'depthwise_fwd_kernel',
          'depthwise_lds_kernel', 'depthwise_wgrad_kernel', 'depthwise_wgrad_reduce_kernel', 'cnorm_stats_kernel', 'cnorm_apply_kernel',
          'cnorm_small_kernel', 'se_hidden_fwd_kernel', 'se_gate_fwd_kernel', 'se_excite_bwd_hidden_kernel', 'se_excite_wgrad_kernel', 'se_dm_kernel',
          'cl_planar_kernel')
MARKER = 'bitwise_not'       # the ATen kernel `drive` launches after every row; nothing else in the run uses it

# One MedFormer step: (R, K, N) of the pointwise GEMMs per mode, (R, N, K) of their weight gradients, (spatial size, channels) per stage
STEP_PW0 = [(54, 128, 128), (54, 128, 256), (54, 128, 320), (54, 256, 256), (54, 256, 320), (54, 256, 512), (54, 320, 128), (54, 320, 256),
            (54, 320, 320), (54, 320, 640), (54, 384, 128), (54, 576, 256), (162, 320, 320), (162, 320, 960), (216, 320, 32), (432, 320, 320),
            (432, 320, 640), (432, 320, 1280), (432, 1280, 320), (432, 2048, 320), (1728, 256, 32), (3456, 256, 256), (3456, 256, 512),
            (3456, 256, 1024), (3456, 576, 256), (3456, 576, 512), (3456, 1024, 256), (13824, 128, 32), (27648, 128, 28), (27648, 128, 128),
            (27648, 128, 256), (27648, 128, 512), (27648, 384, 128), (27648, 384, 256), (27648, 512, 128), (221184, 256, 64)]
STEP_PW1 = [(54, 128, 128), (54, 128, 320), (54, 128, 384), (54, 256, 128), (54, 256, 256), (54, 256, 320), (54, 256, 576), (54, 320, 128),
            (54, 320, 256), (54, 320, 320), (54, 512, 256), (54, 640, 320), (162, 320, 320), (162, 960, 320), (216, 32, 320), (432, 320, 320),
            (432, 320, 1280), (432, 320, 2048), (432, 640, 320), (432, 1280, 320), (1728, 32, 256), (3456, 256, 256), (3456, 256, 576),
            (3456, 256, 1024), (3456, 512, 256), (3456, 512, 576), (3456, 1024, 256), (13824, 32, 128), (27648, 28, 128), (27648, 128, 128),
            (27648, 128, 384), (27648, 128, 512), (27648, 256, 128), (27648, 256, 384), (27648, 512, 128), (221184, 64, 256)]
STEP_WG = STEP_PW1                                            # (R, N, K) of dW: the data gradient of the same layer, x := dy
STEP_DW = [(6, 320), (6, 1280), (6, 2048), (12, 256), (12, 576), (12, 1024), (24, 128), (24, 384), (24, 512), (48, 256)]
STEP_NORM = [(27, 128, 0), (27, 256, 0), (27, 320, 0), (216, 320, 0), (216, 320, 1), (216, 1280, 0), (216, 1280, 1), (216, 2048, 0), (1728, 256, 0),
             (1728, 256, 1), (1728, 576, 0), (1728, 576, 1), (1728, 1024, 0), (1728, 1024, 1), (13824, 128, 0), (13824, 128, 1), (13824, 384, 0),
             (13824, 384, 1), (13824, 512, 0), (13824, 512, 1), (110592, 256, 0)]

ROWS = []      # (op, dtype, shape); dtype: the compute type of the pointwise kernels, 'f32' (storage) elsewhere
# pointwise GEMM (mode, R, K, N): the step; 1 / ragged 2 / 2 / 4 tiles of 32 output channels; the reduction split on at 8 k-steps (K = 113 bf16,
# 57 f32) and off at 128 whole-K row blocks (R = 16257 with one column block); both modes
ROWS += [('pw', 'bf16', (0,) + s) for s in STEP_PW0] + [('pw', 'bf16', (1,) + s) for s in STEP_PW1]
ROWS += [('pw', 'bf16', (0, 200, 32, N)) for N in (32, 36, 64, 128)] + [('pw', 'f32', (1, 200, 32, N)) for N in (32, 36, 64, 128)]
ROWS += [('pw', 'bf16', (0, 200, K, 64)) for K in (112, 113)] + [('pw', 'f32', (0, 200, K, 64)) for K in (56, 57)]
ROWS += [('pw', dt, (m, R, 128, 128)) for dt, m in (('bf16', 0), ('f32', 1)) for R in (16256, 16257)]
# its weight gradient (R, N, K): the step; WNW 1 / 4 / 2; one slab written directly vs two slabs + reduce; 256 / tiles caps the slabs (one tile: 256,
# four tiles: 64); rows no multiple of 16
ROWS += [('pw_wgrad', 'bf16', s) for s in STEP_WG]
ROWS += [('pw_wgrad', 'bf16', (4096, N, K)) for N in (64, 68) for K in (64, 68)] + [('pw_wgrad', 'f32', (4096, 68, 68))]
ROWS += [('pw_wgrad', dt, (R, 64, 64)) for dt in ('bf16', 'f32') for R in (64, 65)]
ROWS += [('pw_wgrad', 'bf16', (R, 64, 64)) for R in (16384, 16448)] + [('pw_wgrad', 'bf16', (R, 256, 256)) for R in (4096, 4160)]
ROWS += [('pw_wgrad', 'bf16', (1000, 64, 64)), ('pw_wgrad', 'f32', (1001, 132, 36))]
# batched fragment packing: (rows, cols, mode) per weight
ROWS += [('pw_pack_batch', 'bf16', ((36, 20, 0), (20, 36, 1))), ('pw_pack_batch', 'f32', ((36, 20, 0),)),
         ('pw_pack_batch', 'bf16', tuple((1280, 320, i & 1) for i in range(8)))]
# depthwise forward / data gradient (N, D, H, W, C, flip): the step; the LDS kernel from 6 x 32 x 32; two D segments from D = 12; partial channel
# groups of both kernels; the register kernel's grid: all passes (small), the 1024-block floor, 8 passes per block, the 2048 cap
ROWS += [('dw', 'f32', (2, S, S, S, C, f)) for S, C in STEP_DW for f in (0, 1)]
ROWS += [('dw', 'f32', (1,) + s + (32, 0)) for s in ((6, 32, 32), (5, 32, 32), (6, 31, 32), (6, 32, 31), (11, 32, 32), (12, 32, 32))]
ROWS += [('dw', 'f32', (1, 6, 32, 32, C, 1)) for C in (4, 36, 68)] + [('dw', 'f32', (1, 4, 6, 7, C, f)) for C, f in ((4, 0), (32, 1), (36, 0), (68, 1))]
ROWS += [('dw', 'f32', (1, 5, 256, 256, 4, 0)), ('dw', 'f32', (1, 5, 256, 256, 128, 1)), ('dw', 'f32', (1, 5, 512, 512, 4, 0))]
# depthwise weight gradient (N, D, H, W, C): the step; 1 | 2 rows at 128 | 129 voxels, 1024 rows reached at 131072 and kept at 131073
ROWS += [('dw_wgrad', 'f32', (2, S, S, S, C)) for S, C in STEP_DW]
ROWS += [('dw_wgrad', 'f32', (1,) + s + (C,)) for s, C in (((1, 8, 16), 4), ((1, 3, 43), 4), ((32, 64, 64), 4), ((1, 3, 43691), 4), ((2, 5, 7), 68))]
# channel norm (N, vox, C, relu), forward and backward: the step; one launch up to 512 voxels; 512 statistics rows from 65536 voxels; 2048 apply
# blocks from 32768 voxels; one and two channel groups
ROWS += [(op, 'f32', (2,) + s) for s in STEP_NORM for op in ('cnorm_fwd', 'cnorm_bwd')]
ROWS += [(op, 'f32', (1, v, 4, 0)) for v in (512, 513, 32768, 32769, 65536, 65537) for op in ('cnorm_fwd', 'cnorm_bwd')]
ROWS += [(op, 'f32', (2, v, 68, 1)) for v in (512, 513) for op in ('cnorm_fwd', 'cnorm_bwd')]
# the statistics and apply launches on their own (N, vox, C, relu, mode): the step's channel_stats calls; below 513 voxels; the affine map
ROWS += [('cnorm_stats', 'f32', (2, v, C, 0, 0)) for v, C in ((216, 320), (1728, 256), (13824, 128), (110592, 64))]
ROWS += [('cnorm_stats', 'f32', (1, 100, 68, 1, 1)), ('cnorm_apply', 'f32', (1, 100, 68, 1, 0)), ('cnorm_apply', 'f32', (2, 32769, 4, 0, 1)),
         ('cnorm_apply', 'f32', (2, 513, 68, 0, 2))]
# squeeze-excite (N, vox, C, r): the step; 16 hidden units per block forward (r = 16 | 17), 32 backward (r = 32 | 33)
ROWS += [(op, 'f32', (2,) + s) for s in ((216, 1280, 320), (1728, 1024, 256), (13824, 512, 128)) for op in ('se_fwd', 'se_bwd')]
ROWS += [(op, 'f32', (2, 100, 4 * r, r)) for r in (16, 17, 32, 33) for op in ('se_fwd', 'se_bwd')]
# channels-last <-> planar (N, vox, C, K, dir): the step; 64 channels taken, 68 refused; fewer planes than channels
ROWS += [('cl_planar', 'f32', (2, 884736, 32, 26, d)) for d in (0, 1)]
ROWS += [('cl_planar', 'f32', (2, 1000, 64, 64, 0)), ('cl_planar', 'f32', (2, 1000, 68, 4, 0)), ('cl_planar', 'f32', (1, 129, 8, 3, 1))]
UNSUPPORTED = 3      # RSUPER_ERR_UNSUPPORTED


def pack_table(entries, f32):
    """rows of rsuper_pointwise_pack_batch's table without the weight pointers: [0, byte offset, rows, cols, mode, ntiles, ksteps, first item]"""
    tab, first = [], 0
    for rows, cols, mode in entries:
        N, K = (rows, cols) if mode == 0 else (cols, rows)
        ntiles, ksteps = -(-N // 32), -(-K // (8 if f32 else 16))
        tab.append([0, first * 16, rows, cols, mode, ntiles, ksteps, first])
        first += ksteps * ntiles * 64
    return tab + [[0, 0, 0, 0, 0, 0, 0, first]], first


def drive(root, out):
    sys.path.insert(0, root)
    import torch
    from rsuper_amd.hip import lib, ops
    lib.require_device()
    L, dev = ops._L(), 'cuda'
    dts = {'f32': torch.float32, 'bf16': torch.bfloat16}
    marker = torch.zeros(64, device=dev, dtype=torch.int32)
    p = ops._ptr

    def rnd(shape, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)

    def nan(*shape):
        return torch.full(shape, float('nan'), device=dev, dtype=torch.float32)

    def norm(N, vox, C, relu, bwd):
        """the one C-ABI call of ChannelNormFn; where the module itself still chooses the one-launch kernel (the recorded commit), as it chooses"""
        x, dy, o = rnd((N, vox, C), 1), rnd((N, vox, C), 2), nan(N, vox, C)
        mr = torch.stack([rnd((N, C), 3), rnd((N, C), 4).abs() + 0.5], -1).contiguous() if bwd else nan(N, C, 2)
        st = ops._stream()
        if hasattr(ops, 'CNORM_SMALL_VOX'):
            if vox <= ops.CNORM_SMALL_VOX:
                return (L.rsuper_cnorm_small(p(x), p(dy), p(mr), p(o), None, N, vox, C, relu, 0.0, 1, st) if bwd else
                        L.rsuper_cnorm_small(p(x), None, None, p(o), p(mr), N, vox, C, relu, 1e-5, 0, st)), [o, mr]
            rows = L.rsuper_cnorm_rows(vox)
        else:
            rows = L.rsuper_cnorm_part_rows(vox)
        part, gm = nan(N, max(rows, 1), C, 2), nan(N, C, 2)
        if bwd:
            return L.rsuper_cnorm_backward(p(x), p(dy), p(mr), p(part) if rows else None, p(gm) if rows else None, p(o), N, vox, C, relu, st), [o, mr] + [part, gm] * bool(rows)
        return L.rsuper_cnorm_forward(p(x), p(part) if rows else None, p(mr), p(o), N, vox, C, relu, 1e-5, st), [o, mr] + [part] * bool(rows)

    def one(op, mode, s):
        """exactly one C-ABI call; returns (return code, outputs)"""
        d, st = ops._DT[dts[mode]], ops._stream()
        if op == 'pw':
            m, R, K, N = s
            ldx = (K + 3) // 4 * 4                                # row strides are whole float4s
            x, w, y = rnd((R, ldx), 1), rnd((N, K) if m == 0 else (K, N), 2), nan(R, N)
            ws = torch.empty((L.rsuper_pointwise_packed_bytes(d, K, N),), device=dev, dtype=torch.uint8)
            return L.rsuper_pointwise(d, m, p(x), ldx, p(w), None, None, N, p(y), N, R, K, N, p(ws), st), [y]
        if op == 'pw_wgrad':
            R, N, K = s
            dy, x, dw, db = rnd((R, N), 1), rnd((R, K), 2), nan(N, K), nan(N)
            S = L.rsuper_pointwise_wgrad_splits(R, N, K)
            ws = nan(S * (N * K + N))
            return L.rsuper_pointwise_wgrad(d, p(dy), N, p(x), K, R, N, K, p(ws), S, p(dw), p(db), st), [dw, db] + [ws] * (S > 1)
        if op == 'pw_pack_batch':
            tab, total = pack_table(s, mode == 'f32')
            ws = [rnd((r, c), 3 + i) for i, (r, c, _) in enumerate(s)]
            for row, w in zip(tab, ws):
                row[0] = w.data_ptr()
            t = torch.tensor(tab, dtype=torch.int64).to(dev)
            arena = torch.full((total * 16,), 255, device=dev, dtype=torch.uint8)      # all ones: NaN in either compute type
            return L.rsuper_pointwise_pack_batch(d, p(t), len(s), total, p(arena), st), [arena.view(dts[mode])]
        if op == 'dw':
            N, D, H, W, C, flip = s
            x, w, y = rnd((N, D, H, W, C), 1), rnd((C, 1, 3, 3, 3), 2), nan(N, D, H, W, C)
            return L.rsuper_depthwise3_fwd(p(x), p(w), p(y), N, D, H, W, C, flip, st), [y]
        if op == 'dw_wgrad':
            N, D, H, W, C = s
            x, dy, dw = rnd((N, D, H, W, C), 1), rnd((N, D, H, W, C), 2), nan(C, 1, 3, 3, 3)
            part = nan(L.rsuper_depthwise3_rows(N * D * H * W), 27, C)
            return L.rsuper_depthwise3_wgrad(p(x), p(dy), p(part), p(dw), N, D, H, W, C, st), [dw, part]
        if op in ('cnorm_fwd', 'cnorm_bwd'):
            return norm(*s, op == 'cnorm_bwd')
        if op in ('cnorm_stats', 'cnorm_apply'):
            N, vox, C, relu, m = s
            x, dy, mr, gm = rnd((N, vox, C), 1), rnd((N, vox, C), 2), rnd((N, C, 2), 3).abs() + 0.5, rnd((N, C, 2), 4) * 0.1
            if op == 'cnorm_stats':
                part = nan(N, L.rsuper_cnorm_rows(vox), C, 2)
                return L.rsuper_cnorm_stats(p(x), p(dy), p(mr), p(part), N, vox, C, relu, m, st), [part]
            o = nan(N, vox, C)
            return L.rsuper_cnorm_apply(p(x), p(dy), p(mr), p(gm), p(o), N, vox, C, relu, m, st), [o]
        if op in ('se_fwd', 'se_bwd'):
            N, vox, C, r = s
            x, w1, b1, w2, b2 = rnd((N, vox, C), 1), rnd((r, C), 2) * 0.1, rnd((r,), 3), rnd((C, r), 4) * 0.1, rnd((C,), 5)
            part = nan(N, L.rsuper_cnorm_rows(vox), C, 2)
            if op == 'se_fwd':
                ms, tab, hbuf, y = nan(N, C, 2), nan(N, C, 2), nan(N, r), nan(N, vox, C)
                return L.rsuper_se_forward(p(x), p(w1), p(b1), p(w2), p(b2), p(part), p(ms), p(tab), p(hbuf), p(y), N, vox, C, r, st), [part, ms, tab, hbuf, y]
            dy, ms, tab, hbuf = rnd((N, vox, C), 6), rnd((N, C, 2), 7), torch.rand((N, C, 2), device=dev), rnd((N, r), 8).abs()
            gm, dz1, tab2, dx = nan(N, C, 2), nan(N, r), nan(N, C, 2), nan(N, vox, C)
            dw1, db1, dw2, db2 = nan(r, C), nan(r), nan(C, r), nan(C)
            return L.rsuper_se_backward(p(x), p(dy), p(ops._se_identity(N, C, dev)), p(w1), p(w2), p(ms), p(tab), p(hbuf), p(part), p(gm), p(dz1), p(tab2),
                                        p(dx), p(dw1), p(db1), p(dw2), p(db2), N, vox, C, r, st), [part, gm, dz1, tab2, dx, dw1, db1, dw2, db2]
        N, vox, C, K, to_cl = s
        src, dst = (rnd((N, K, vox), 1), nan(N, vox, C)) if to_cl else (rnd((N, vox, C), 1), nan(N, K, vox))
        return L.rsuper_cl_planar(p(src), p(dst), N, vox, C, K, to_cl, st), [dst]

    done = []
    for op, mode, s in ROWS:
        rc, outs = one(op, mode, s)
        marker.bitwise_not_()
        torch.cuda.synchronize()
        assert rc in (0, UNSUPPORTED), (op, mode, s, rc)
        if rc == 0:
            assert not any(bool(torch.isnan(o.float()).any()) for o in outs), ('NaN (unwritten output)', op, mode, s)
        done.append({'op': op, 'dtype': mode, 'shape': json.loads(json.dumps(s)), 'rc': rc})
        del outs
    json.dump(done, open(out, 'w'))
    print(f'{len(done)} calls, {sum(r["rc"] == 0 for r in done)} launched')


def launches(trace_dir):
    """the family's launches of a rocprofv3 kernel trace in start order, cut at the markers: per row a list of
    [name with template arguments, blocks, workgroup, LDS bytes]"""
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    assert len(files) == 1, files
    got = []
    for r in csv.DictReader(open(files[0])):
        name = re.sub(r'^void ', '', r['Kernel_Name'].replace('(anonymous namespace)::', ''))
        if MARKER in name:
            got.append((int(r['Start_Timestamp']), None))
            continue
        name = name[:name.index('(')] if '(' in name else name
        if name.split('<')[0] not in FAMILY:
            continue
        wg = [int(r['Workgroup_Size_' + a]) for a in 'XYZ']
        assert wg[1] == wg[2] == 1
        got.append((int(r['Start_Timestamp']), [name, [int(r['Grid_Size_' + a]) // w for a, w in zip('XYZ', wg)], wg[0], int(r['LDS_Block_Size'])]))
    rows, cur = [], []
    for _, l in sorted(got, key=lambda g: g[0]):
        if l is None:
            rows.append(cur)
            cur = []
        else:
            cur.append(l)
    assert not cur, cur
    return rows


def table(trace_dir, rows_json, commit, out):
    rows, ls = json.load(open(rows_json)), launches(trace_dir)
    assert len(rows) == len(ROWS) == len(ls), (len(rows), len(ROWS), len(ls))
    for r, l in zip(rows, ls):
        assert bool(l) == (r['rc'] == 0), (r, l)
        r['launches'] = l
    with open(out, 'w') as f:
        f.write('{"commit": "%s",\n "columns": ["op", "dtype", "shape", "rc", "launches"],\n "launch": ["kernel", "blocks", "threads", "lds"],\n "rows": [\n' % commit)
        f.write(',\n'.join('  ' + json.dumps([r[k] for k in ('op', 'dtype', 'shape', 'rc', 'launches')]) for r in rows))
        f.write('\n ]}\n')
    n = [l[0] for r in ls for l in r]
    print(f'{out}: {len(rows)} rows, {len(n)} launches, {len(set(n))} kernel instantiations of {len(set(k.split("<")[0] for k in n))} __global__s')


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
    q = sub.add_parser('drive'); q.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))); q.add_argument('--out', required=True)
    q = sub.add_parser('table'); q.add_argument('trace_dir'); q.add_argument('rows'); q.add_argument('commit'); q.add_argument('-o', required=True)
    q = sub.add_parser('compare'); q.add_argument('a'); q.add_argument('b')
    a = ap.parse_args()
    sys.exit(drive(a.root, a.out) if a.cmd == 'drive' else table(a.trace_dir, a.rows, a.commit, a.o) if a.cmd == 'table' else compare(a.a, a.b))
