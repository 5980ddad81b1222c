"""Which kernel, template arguments, grid, workgroup and statistics rows a launch of the bandwidth-bound glue kernels gets (InstanceNorm backward tail,
max pool, stride-2 subsample, trilinear up-sampling: csrc/unet_misc.hip) is ONE decision, csrc/glue_plan.hpp, that the launches read and
rsuper_glue_plan / rsuper_stat_rows answer from the shape alone.  tests/golden/glue_launches.json holds the launches a kernel trace recorded on the
commit before that header existed (tests/golden/gen_golden_glue_launches.py: one C-ABI call per row, every rung of the dispatch at the smallest shape
that reaches it, each under both values of rsuper_glue_variant); the plan must reproduce every one of them.  Pure host code: no GPU."""
import ctypes
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import gen_golden_glue_launches as gen  # noqa: E402

TABLE = json.load(open(os.path.join(GOLDEN, 'glue_launches.json')))
RECORDED = [dict(zip(TABLE['columns'], r)) for r in TABLE['rows']]
OPS = ('in_bwd', 'pool_fwd', 'pool_bwd', 'sub_fwd', 'sub_bwd', 'up_fwd', 'up_bwd')      # rsuper_glue_plan's op, in the order of the header's enum
CTYPE = {'f32': 'float', 'bf16': 'unsigned short'}
UNSUPPORTED, ERR_ARG = 3, 1


@pytest.fixture
def L():
    from rsuper_amd.hip import lib
    L = lib.lib()
    assert L.rsuper_glue_variant(-1) == 1 and L.rsuper_lazy_tails(-1) == 1
    yield L
    assert L.rsuper_glue_variant(1) == 1 and L.rsuper_lazy_tails(1) == 1


def plan(L, op, dtype, N, shape, C, ld=None):
    """(return code, dict of the eight plan fields)"""
    from rsuper_amd.hip import lib
    s = (ctypes.c_int * 7)(N, *shape)
    out = (ctypes.c_int * 8)(*([-7] * 8))
    rc = L.rsuper_glue_plan(OPS.index(op), {'f32': lib.F32, 'bf16': lib.BF16}[dtype], s, C, C if ld is None else ld, out)
    return rc, dict(zip(('kernel', 'sel', 'bx', 'by', 'bz', 'threads', 'lds', 'rows'), out))


def instantiation(p, dtype):
    """the plan's kernel as the trace names it"""
    from rsuper_amd.hip import lib
    base, T = lib.GLUE_KERNELS[p['kernel']], CTYPE[dtype]
    args = {'in_bwd_finalize2_kernel': f'{T}, {p["sel"]}', 'maxpool_fwd2_kernel': f'{T}, 4', 'maxpool_bwd_kernel': f'{T}, 0',      # no lazy gradient in the table
            'upsample_bwd4_kernel': f'{p["sel"]}, false'}.get(base, T)
    return f'{base}<{args}>'


def out_vox(op, shape):
    if op == 'pool_fwd':
        return (shape[0] // 2) * (shape[1] // 2) * (shape[2] // 2)
    if op == 'sub_fwd':
        return ((shape[0] + 1) // 2) * ((shape[1] + 1) // 2) * ((shape[2] + 1) // 2)
    return shape[3] * shape[4] * shape[5]


def test_table_holds_every_row_under_both_variants():
    assert len(TABLE['commit']) == 12 and int(TABLE['commit'], 16) >= 0
    want = [(op, dt, N, list(s), C, v) for v in (1, 0) for op, dt, N, s, C in gen.ROWS]
    assert [(r['op'], r['dtype'], r['N'], r['shape'], r['C'], r['variant']) for r in RECORDED] == want
    assert sum(r['rc'] == UNSUPPORTED for r in RECORDED) == 2 and all(r['rc'] in (0, UNSUPPORTED) for r in RECORDED)
    from rsuper_amd.hip import lib
    seen = {r['kernel'].split('<')[0] for r in RECORDED if r['rc'] == 0}
    # the first-generation trilinear kernels run only beyond 32-bit offsets (4 GB tensors): test_limits_of_32_bit_offsets pins those rungs
    assert seen == set(lib.GLUE_KERNELS) - {'upsample_fwd_kernel', 'upsample_bwd_kernel'}


def test_plan_reproduces_the_recorded_launches(L):
    for r in RECORDED:
        assert L.rsuper_glue_variant(r['variant']) == r['variant']
        rc, p = plan(L, r['op'], r['dtype'], r['N'], r['shape'], r['C'])
        assert rc == r['rc'], (r, rc)
        if rc:
            continue
        got = (instantiation(p, r['dtype']), [p['bx'], p['by'], p['bz']], p['threads'])
        assert got == (r['kernel'], r['blocks'], r['threads']), (r, p)


def test_grid_fields_and_statistics_rows(L):
    from rsuper_amd.hip import lib
    split = False
    for r in RECORDED:
        L.rsuper_glue_variant(r['variant'])
        rc, p = plan(L, r['op'], r['dtype'], r['N'], r['shape'], r['C'])
        if rc:
            continue
        assert p['bx'] >= 1 and p['bz'] >= 1 and p['by'] == r['N'] <= 65535 and 64 <= p['threads'] <= 1024 and p['lds'] >= 0, (r, p)
        if r['op'] in ('pool_fwd', 'sub_fwd', 'up_fwd'):      # the kernels that write rows of `part`: one row per block in x, as many as the caller allocates
            assert p['rows'] == p['bx'] == L.rsuper_stat_rows(OPS.index(r['op']), out_vox(r['op'], r['shape'])), (r, p)
        else:
            assert p['rows'] == 0 and p['bz'] == 1 and L.rsuper_stat_rows(OPS.index(r['op']), 4096) == 0, (r, p)
        if r['variant'] == 0:
            assert lib.GLUE_KERNELS[p['kernel']] not in ('in_bwd_finalize2_kernel', 'maxpool_fwd2_kernel', 'upsample_fwd3_kernel') and p['bz'] == 1, (r, p)
        split |= p['bz'] > 1
    assert split                                                 # the default variant's channel-split grids are in the table


def test_stat_rows(L):
    from rsuper_amd.hip import lib
    for vox in (0, 1, 63, 64, 127, 128, 216, 1728, 64 * 2048 - 1, 64 * 2048, 64 * 2048 + 64, 96 ** 3, 2 ** 31 + 5):
        for op in (lib.GLUE_POOL_FWD, lib.GLUE_SUB_FWD, lib.GLUE_UP_FWD):
            assert L.rsuper_stat_rows(op, vox) == max(1, min(2048, vox // 64)), (op, vox)
    for vox in (1, 255, 256, 257, 32 ** 3, 96 ** 3, 96 ** 3 + 1):
        assert L.rsuper_stat_rows(lib.GLUE_STEM_FWD, vox) == -(-vox // 256), vox
    assert L.rsuper_stat_rows(lib.GLUE_POOL_FWD, -1) == 0 and L.rsuper_stat_rows(8, 64) == 0 and L.rsuper_stat_rows(-1, 64) == 0
    from rsuper_amd.hip import ops
    assert [ops._stat_blocks(v) for v in (6 ** 3, 12 ** 3, 48 ** 3, 96 ** 3)] == [3, 27, 1728, 2048]


def test_lazy_trilinear_backward_only_where_the_plan_names_the_row_sharing_kernel(L):
    from rsuper_amd.hip import lib
    shapes = [(r['N'], r['shape'], r['C']) for r in RECORDED if r['op'] == 'up_bwd' and r['dtype'] == 'bf16' and r['variant'] == 1]
    shapes += [(2, [6, 6, 6, 18, 18, 18], 16), (1, [4, 4, 4, 10, 10, 10], 8), (2, [8, 8, 8, 16, 16, 16], 8 * 257)]
    assert L.rsuper_lazy_tails(2) == 2
    answers = []
    for N, s, C in shapes:
        lazy = L.rsuper_upsample_bwd_lazy_plan(lib.BF16, N, *s, C)
        rc, p = plan(L, 'up_bwd', 'bf16', N, s, C)
        named = rc == 0 and lib.GLUE_KERNELS[p['kernel']] == 'upsample_bwd4_kernel'
        assert lazy in (0, 1) and (lazy != 1 or named), (N, s, C, lazy, rc, p)
        assert lazy == int(named), (N, s, C)                     # and under the measuring switch every launch the kernel takes is admitted
        answers.append(lazy)
    assert 0 in answers and 1 in answers


def test_limits_of_32_bit_offsets(L):
    """The rungs no 34 MB tensor reaches, from the limits themselves: the kernels after the first generation address their operands with 32-bit
    offsets (vectors of the tail; elements and bytes of the trilinear input; bytes of the trilinear output gradient)."""
    from rsuper_amd.hip import lib
    K = lib.GLUE_KERNELS
    # tail: the vector index of a sample is 32 bits
    rc, p = plan(L, 'in_bwd', 'bf16', 1, [2 ** 31 - 1], 16)      # 2^32 - 2 vectors
    assert rc == 0 and K[p['kernel']] == 'in_bwd_finalize_kernel' and p['bx'] == 4096
    assert plan(L, 'in_bwd', 'bf16', 1, [2 ** 31 - 1], 24)[0] == UNSUPPORTED
    # trilinear forward: N x input elements below 2^31 - 1, input bytes of a sample below 2^32 - 1
    big_in, out = [1024, 1024, 128], [1024, 1024, 256]           # 2^27 voxels; tables of 2304 outputs fit
    rc, p = plan(L, 'up_fwd', 'bf16', 1, big_in + out, 8)        # 2^30 elements, 2^31 bytes
    assert rc == 0 and K[p['kernel']] == 'upsample_fwd3_kernel'
    rc, p = plan(L, 'up_fwd', 'f32', 1, big_in + out, 8)         # 2^32 bytes: no table kernel
    assert rc == 0 and K[p['kernel']] == 'upsample_fwd2_kernel'
    rc, p = plan(L, 'up_fwd', 'bf16', 2, big_in + out, 8)        # 2^31 elements: the first generation
    assert rc == 0 and K[p['kernel']] == 'upsample_fwd_kernel' and (p['bx'], p['by'], p['bz'], p['threads'], p['rows']) == (2048, 2, 1, 256, 2048)
    rc, p = plan(L, 'up_fwd', 'bf16', 1, big_in + out, 8, ld=16)      # the row stride counts, not the channels
    assert rc == 0 and K[p['kernel']] == 'upsample_fwd_kernel'
    # trilinear backward: output-gradient bytes of a sample below 2^32 - 1 for the row-sharing and the table kernel
    I, O = [256, 512, 512], [512, 1024, 1024]
    rc, p = plan(L, 'up_bwd', 'bf16', 1, I + O, 8)               # 2^29 voxels x 16 bytes
    assert rc == 0 and K[p['kernel']] == 'upsample_bwd_kernel' and (p['bx'], p['threads'], p['lds']) == (4096, 256, 0)
    rc, p = plan(L, 'up_bwd', 'bf16', 1, [128, 512, 512, 256, 1024, 1024], 8)      # 2^28 voxels x 16 bytes = 2^32: still one too many
    assert rc == 0 and K[p['kernel']] == 'upsample_bwd_kernel'
    rc, p = plan(L, 'up_bwd', 'bf16', 1, [128, 512, 256, 256, 1024, 512], 8)
    assert rc == 0 and K[p['kernel']] == 'upsample_bwd4_kernel' and p['sel'] == 4
    # more than 256 vectors per voxel: no kernel of the pooling / trilinear family
    for op, s in (('pool_fwd', [4, 4, 6]), ('pool_bwd', [4, 4, 6]), ('sub_fwd', [4, 4, 6]), ('sub_bwd', [4, 4, 6]), ('up_fwd', [3, 3, 4, 6, 6, 8]),
                  ('up_bwd', [3, 3, 4, 6, 6, 8])):
        assert plan(L, op, 'bf16', 1, s, 8 * 257)[0] == UNSUPPORTED and plan(L, op, 'f32', 1, s, 4 * 258)[0] == UNSUPPORTED, op
        assert plan(L, op, 'bf16', 1, s, 8 * 256)[0] == 0, op


def test_bad_arguments_answer_an_error_not_a_plan(L):
    from rsuper_amd.hip import lib
    good = {'op': 5, 'dtype': lib.BF16, 'shape': [2, 3, 5, 4, 7, 9, 11], 'C': 8, 'ld': 8}

    def ask(**kw):
        a = dict(good, **kw)
        out = (ctypes.c_int * 8)(*([-7] * 8))
        rc = L.rsuper_glue_plan(a['op'], a['dtype'], (ctypes.c_int * 7)(*a['shape']) if a['shape'] else None, a['C'], a['ld'], out)
        assert rc == 0 or list(out) == [-7] * 8                  # an error leaves no plan behind
        return rc
    assert ask() == 0
    for bad in ({'op': -1}, {'op': 7}, {'op': 8}, {'dtype': 5}, {'C': 0}, {'C': 12}, {'C': -8}, {'ld': 4}, {'ld': 12}, {'shape': None},
                {'shape': [0, 3, 5, 4, 7, 9, 11]}, {'shape': [2, 3, 0, 4, 7, 9, 11]}, {'shape': [2, 3, 5, 4, 7, 9, -1]}):
        assert ask(**bad) == ERR_ARG, bad
    assert ask(op=1, shape=[2, 1, 4, 4, 0, 0, 0]) == ERR_ARG      # nothing to pool
    assert ask(op=0, shape=[2, 0, 0, 0, 0, 0, 0]) == ERR_ARG
    assert ask(shape=[65536, 3, 5, 4, 7, 9, 11]) == UNSUPPORTED   # N is gridDim.y
    assert L.rsuper_glue_plan(5, lib.BF16, (ctypes.c_int * 7)(*good['shape']), 8, 8, None) == ERR_ARG
