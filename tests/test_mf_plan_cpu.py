"""Which kernel, template arguments, grid, workgroup, rows of `part` and workspace a launch of the kernels of MedFormer's attention stages gets
(csrc/pointwise.hip, depthwise.hip, instnorm.hip) is ONE decision, csrc/mf_plan.hpp, that the launches read and rsuper_mf_plan answers from the shape
alone.  tests/golden/mf_launches.json holds the launches a kernel trace recorded on the commit before that header existed
(tests/golden/gen_golden_mf_launches.py: one C-ABI call per row, every rung of the dispatch at the smallest shape that reaches it and every distinct
call of a MedFormer step); the plan must reproduce every one of them.  Pure host code: no GPU."""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
import gen_golden_mf_launches as gen  # noqa: E402

TABLE = json.load(open(os.path.join(GOLDEN, 'mf_launches.json')))
RECORDED = [dict(zip(TABLE['columns'], r)) for r in TABLE['rows']]
CTYPE = {'f32': 'float', 'bf16': 'unsigned short'}
UNSUPPORTED, ERR_ARG = 3, 1


@pytest.fixture
def L():
    from rsuper_amd.hip import lib
    return lib.lib()


def plan(L, op, dtype, *shape):
    """(return code, dict of the ten plan fields)"""
    from rsuper_amd.hip import lib
    out = (ctypes.c_int * 10)(*([-7] * 10))
    rc = L.rsuper_mf_plan(op, {'f32': lib.F32, 'bf16': lib.BF16}[dtype], (ctypes.c_int * 8)(*shape), out)
    return rc, dict(zip(lib.MF_PLAN_FIELDS, out))


def call_plans(L, op, dt, s):
    """the launches of one C-ABI call of gen.ROWS as the plan names them: (return code, [plan, ...]); a refused launch refuses the call"""
    from rsuper_amd.hip import lib as l
    if op == 'pw':
        ask = [(l.MF_PW_PACK, s[2], s[3]), (l.MF_PW, s[1], s[2], s[3])]
    elif op == 'pw_wgrad':
        ask = [(l.MF_PW_WGRAD, *s), (l.MF_PW_WGRAD_REDUCE, *s)]
    elif op == 'pw_pack_batch':
        ask = [(l.MF_PW_PACK_BATCH, gen.pack_table(s, dt == 'f32')[1])]
    elif op == 'dw':
        ask = [(l.MF_DW, *s[:5])]
    elif op == 'dw_wgrad':
        ask = [(l.MF_DW_WGRAD, *s), (l.MF_DW_WGRAD_REDUCE, *s)]
    elif op in ('cnorm_fwd', 'cnorm_bwd'):
        N, vox, C, _ = s
        mode = int(op == 'cnorm_bwd')
        rc, first = plan(L, l.MF_CNORM, dt, N, vox, C, mode)
        assert rc == 0
        ask = [(l.MF_CNORM, N, vox, C, mode)] + ([(l.MF_CNORM_APPLY, N, vox, C, mode)] if l.MF_KERNELS[first['kernel']] == 'cnorm_stats_kernel' else [])
    elif op in ('cnorm_stats', 'cnorm_apply'):
        ask = [(l.MF_CNORM_STATS if op == 'cnorm_stats' else l.MF_CNORM_APPLY, s[0], s[1], s[2], s[4])]
    elif op in ('se_fwd', 'se_bwd'):
        N, vox, C, r = s
        mid = (l.MF_SE_HIDDEN, l.MF_SE_GATE) if op == 'se_fwd' else (l.MF_SE_BWD_HIDDEN, l.MF_SE_WGRAD, l.MF_SE_DM)
        ask = [(l.MF_CNORM_STATS, N, vox, C, int(op == 'se_bwd'))] + [(o, N, C, r) for o in mid] + [(l.MF_CNORM_APPLY, N, vox, C, 2)]
    else:
        ask = [(l.MF_CL_PLANAR, *s[:4])]
    got = [plan(L, a[0], dt, *a[1:]) for a in ask]
    bad = [rc for rc, _ in got if rc]
    return (bad[0], []) if bad else (0, [p for _, p in got if p['kernel'] >= 0])


def instantiation(p, dtype):
    """the plan's kernel as the trace names it"""
    from rsuper_amd.hip import lib
    base, T = lib.MF_KERNELS[p['kernel']], CTYPE[dtype]
    args = {'pw_pack_kernel': T, 'pw_pack_batch_kernel': T, 'pw_gemm_kernel': f'{T}, {p["sel"]}, {"true" if p["arg"] else "false"}',
            'pw_wgrad_kernel': f'{T}, {p["sel"]}', 'cnorm_stats_kernel': str(p['sel']), 'cnorm_apply_kernel': str(p['sel']),
            'cnorm_small_kernel': str(p['sel'])}.get(base)
    return f'{base}<{args}>' if args else base


def test_table_holds_every_row_and_every_kernel():
    assert len(TABLE['commit']) == 12 and int(TABLE['commit'], 16) >= 0
    assert [(r['op'], r['dtype'], r['shape']) for r in RECORDED] == [(op, dt, json.loads(json.dumps(s))) for op, dt, s in gen.ROWS]
    assert [r['shape'] for r in RECORDED if r['rc']] == [[2, 1000, 68, 4, 0]] and all(r['rc'] in (0, UNSUPPORTED) for r in RECORDED)
    from rsuper_amd.hip import lib
    seen = {l[0].split('<')[0] for r in RECORDED for l in r['launches']}
    assert seen == set(lib.MF_KERNELS) == set(gen.FAMILY) and lib.MF_KERNELS == gen.FAMILY
    # ... which are the __global__s of the three files
    src = ''.join(open(os.path.join(ROOT, 'r-super_amd', 'csrc', f + '.hip')).read() for f in ('pointwise', 'depthwise', 'instnorm'))
    assert set(re.findall(r'__global__ .*?void (\w+)\(', src)) == seen


def test_plan_reproduces_the_recorded_launches(L):
    for r in RECORDED:
        rc, plans = call_plans(L, r['op'], r['dtype'], r['shape'])
        assert rc == r['rc'], (r, rc)
        got = [[instantiation(p, r['dtype']), [p['bx'], p['by'], p['bz']], p['threads']] for p in plans]
        assert got == [l[:3] for l in r['launches']], (r, plans)


def test_thin_queries_agree_with_the_plan(L):
    from rsuper_amd.hip import lib
    small = 0
    for r in RECORDED:
        op, dt, s = r['op'], r['dtype'], r['shape']
        if op == 'pw':                                           # ops.pointwise_gemm allocates rsuper_pointwise_packed_bytes
            rc, p = plan(L, lib.MF_PW_PACK, dt, s[2], s[3])
            assert rc == 0 and p['ws'] == L.rsuper_pointwise_packed_bytes({'f32': lib.F32, 'bf16': lib.BF16}[dt], s[2], s[3]) and p['bx'] == -(-p['ws'] // (256 * 16))
        elif op == 'pw_wgrad':                                   # ops.pointwise_wgrad allocates plan['ws'] floats and passes plan['rows'] slabs
            R, N, K = s
            (rc, p), (rc2, red) = plan(L, lib.MF_PW_WGRAD, dt, R, N, K), plan(L, lib.MF_PW_WGRAD_REDUCE, dt, R, N, K)
            S = L.rsuper_pointwise_wgrad_splits(R, N, K)
            assert rc == rc2 == 0 and p['rows'] == p['bz'] == S >= 1 and p['ws'] == S * (N * K + N), (r, p)
            assert p['arg'] % 16 == 0 and (S - 1) * p['arg'] < R <= S * p['arg'], (r, p)        # whole MFMA steps per slab, no slab without rows
            assert (red['kernel'] == -1) == (S == 1), (r, red)
        elif op == 'dw_wgrad':                                   # DepthwiseConvFn allocates rsuper_depthwise3_rows x 27 x C
            rc, p = plan(L, lib.MF_DW_WGRAD, dt, *s)
            assert rc == 0 and p['rows'] == p['bx'] == L.rsuper_depthwise3_rows(s[0] * s[1] * s[2] * s[3]), (r, p)
        elif op in ('cnorm_fwd', 'cnorm_bwd'):                   # ChannelNormFn allocates rsuper_cnorm_part_rows, none for the one launch
            N, vox, C, _ = s
            rc, p = plan(L, lib.MF_CNORM, dt, N, vox, C, int(op == 'cnorm_bwd'))
            one = lib.MF_KERNELS[p['kernel']] == 'cnorm_small_kernel'
            assert rc == 0 and p['rows'] == L.rsuper_cnorm_part_rows(vox) == (0 if one else L.rsuper_cnorm_rows(vox)) and one == (vox <= 512), (r, p)
            small += one
        elif op in ('cnorm_stats', 'se_fwd', 'se_bwd'):          # channel_stats and SqueezeExciteFn allocate rsuper_cnorm_rows at every size
            rc, p = plan(L, lib.MF_CNORM_STATS, dt, s[0], s[1], s[2], 0)
            assert rc == 0 and p['rows'] == p['bx'] == L.rsuper_cnorm_rows(s[1]) >= 1, (r, p)
    assert small
    for vox in (1, 127, 128, 129, 512, 513, 65535, 65536, 65537, 96 ** 3, 2 ** 31 + 5):
        assert L.rsuper_cnorm_rows(vox) == max(1, min(512, -(-vox // 128))) and L.rsuper_depthwise3_rows(vox) == max(1, min(1024, -(-vox // 128))), vox
        assert L.rsuper_cnorm_part_rows(vox) == (0 if vox <= 512 else L.rsuper_cnorm_rows(vox)), vox
    assert L.rsuper_cnorm_part_rows(0) == 0 and L.rsuper_pointwise_wgrad_splits(0, 64, 64) == 0 and L.rsuper_pointwise_packed_bytes(lib.BF16, 0, 64) == 0


def test_ops_allocates_what_the_plan_names():
    """hip/ops.py holds no threshold, row formula or environment switch of the family: it asks."""
    src = open(os.path.join(ROOT, 'r-super_amd', 'hip', 'ops.py')).read()
    assert 'CNORM_SMALL_VOX' not in src and 'rsuper_cnorm_small' not in src
    fn = src[src.index('def pointwise_wgrad('):src.index('def pointwise_supported(')]
    assert 'rsuper_mf_plan' in fn and 'N * K' not in fn and fn.count('_L().') == 2          # one query, one launch call
    norm = src[src.index('class ChannelNormFn'):src.index('class DepthwiseConvFn')]
    assert norm.count('rsuper_cnorm_part_rows') == 1 and norm.count('_L().') == 3 and 'if vox' not in norm
    # the switches are read in one place
    csrc = os.path.join(ROOT, 'r-super_amd', 'csrc')
    for f in ('pointwise.hip', 'depthwise.hip', 'instnorm.hip'):
        assert 'getenv' not in open(os.path.join(csrc, f)).read(), f
    assert open(os.path.join(csrc, 'mf_plan.hpp')).read().count('getenv(') == 1


def test_limits(L):
    """The rungs only a multi-GB tensor reaches, and the refusals, from the limits themselves."""
    from rsuper_amd.hip import lib
    K = lib.MF_KERNELS
    # depthwise: 32-bit byte offsets of the buffer loads
    for op in (lib.MF_DW, lib.MF_DW_WGRAD, lib.MF_DW_WGRAD_REDUCE):
        assert plan(L, op, 'f32', 1, 64, 64, 64, 4096)[0] == UNSUPPORTED               # 2^30 elements
        assert plan(L, op, 'f32', 1, 64, 64, 64, 4092)[0] == 0
    rc, p = plan(L, lib.MF_DW, 'f32', 1, 6, 4096, 4096, 4)                              # (the plane limit of the LDS kernel lies beyond this one)
    assert rc == 0 and K[p['kernel']] == 'depthwise_lds_kernel' and (p['bx'], p['by'], p['bz'], p['threads'], p['arg']) == (512 * 512, 1, 1, 128, 1)
    # squeeze-excite: channel and hidden counts up to 8192
    for op in (lib.MF_SE_HIDDEN, lib.MF_SE_GATE, lib.MF_SE_BWD_HIDDEN, lib.MF_SE_WGRAD, lib.MF_SE_DM):
        assert plan(L, op, 'f32', 2, 8192, 8192)[0] == 0
        assert plan(L, op, 'f32', 2, 8196, 64)[0] == UNSUPPORTED and plan(L, op, 'f32', 2, 64, 8193)[0] == UNSUPPORTED
    rc, p = plan(L, lib.MF_SE_BWD_HIDDEN, 'f32', 2, 8192, 8192)
    assert (p['bx'], p['by'], p['threads'], p['lds']) == (2, 256, 1024, (8192 + 32 * 33) * 4)
    # cl_planar: one 64-channel tile, whole float4s, no more planes than channels
    assert plan(L, lib.MF_CL_PLANAR, 'f32', 2, 1000, 64, 64)[0] == 0
    for C, Kp in ((68, 4), (6, 2), (8, 9)):
        assert plan(L, lib.MF_CL_PLANAR, 'f32', 2, 1000, C, Kp)[0] == UNSUPPORTED
    # the grids that follow the voxel count keep following it
    rc, p = plan(L, lib.MF_CL_PLANAR, 'f32', 1, 2 ** 31 - 1, 4, 1)
    assert rc == 0 and p['bx'] == 2 ** 24
    rc, p = plan(L, lib.MF_PW, 'bf16', 2 ** 31 - 1, 16, 32)
    assert rc == 0 and (p['sel'], p['arg'], p['bx']) == (1, 0, 2 ** 24)


def test_bad_arguments_answer_an_error_not_a_plan(L):
    from rsuper_amd.hip import lib
    good = {'op': lib.MF_DW, 'dtype': lib.F32, 'shape': [2, 6, 32, 32, 64]}

    def ask(**kw):
        a = dict(good, **kw)
        out = (ctypes.c_int * 10)(*([-7] * 10))
        rc = L.rsuper_mf_plan(a['op'], a['dtype'], (ctypes.c_int * 8)(*a['shape']) if a['shape'] else None, out)
        assert rc == 0 or list(out) == [-7] * 10                 # an error leaves no plan behind
        return rc
    assert ask() == 0
    for bad in ({'op': -1}, {'op': 17}, {'dtype': 5}, {'shape': None}, {'shape': [0, 6, 32, 32, 64]}, {'shape': [2, 6, 32, -1, 64]},
                {'shape': [2, 6, 32, 32, 66]}, {'shape': [2, 6, 32, 32, 0]}):
        assert ask(**bad) == ERR_ARG, bad
    assert ask(op=lib.MF_PW, dtype=lib.BF16, shape=[100, 64, 30]) == ERR_ARG            # N % 4
    assert ask(op=lib.MF_PW_WGRAD, dtype=lib.BF16, shape=[100, 64, 30]) == ERR_ARG and ask(op=lib.MF_PW_WGRAD, dtype=lib.BF16, shape=[100, 30, 64]) == ERR_ARG
    assert ask(op=lib.MF_CNORM, shape=[2, 100, 64, 2]) == ERR_ARG and ask(op=lib.MF_CNORM_APPLY, shape=[2, 100, 64, 2]) == 0
    assert ask(op=lib.MF_CNORM_APPLY, shape=[2, 100, 64, 3]) == ERR_ARG and ask(op=lib.MF_CNORM_STATS, shape=[2, 100, 66, 0]) == ERR_ARG
    assert ask(op=lib.MF_SE_GATE, shape=[2, 66, 16]) == ERR_ARG and ask(op=lib.MF_SE_GATE, shape=[2, 64, 0]) == ERR_ARG
    assert ask(op=lib.MF_CL_PLANAR, shape=[2, 0, 32, 26]) == ERR_ARG
    assert ask(shape=[1, 64, 64, 64, 4096]) == UNSUPPORTED
    assert L.rsuper_mf_plan(lib.MF_DW, lib.F32, (ctypes.c_int * 8)(*good['shape']), None) == ERR_ARG
