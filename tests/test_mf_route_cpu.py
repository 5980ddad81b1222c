"""Which implementation a 1x1x1 convolution / linear layer of MedFormer's attention stages takes is ONE decision,
model/dim3/medformer_utils.py linear_route, answered from the sizes alone.  Pinned here: every call of `linear` in a step of the shipped
configuration (config/abdomenatlas_ufo/medformer_3d.yaml as bench.py builds it: 2 x 96^3, 26 classes, deep supervision) runs on
csrc/pointwise.hip, and the edges between the four arms.  Pure host code: no GPU."""
import math

import pytest
import torch
import torch.nn as nn

SHIPPED = dict(base_chan=32, map_size=[3, 3, 3], conv_num=[2, 0, 0, 0, 0, 0, 2, 2], trans_num=[0, 2, 4, 6, 4, 2, 0, 0],
               num_heads=[1, 4, 8, 10, 8, 4, 1, 1], fusion_depth=2, fusion_dim=320, fusion_heads=10, expansion=4, aux_loss=True)
B, S, CLASSES = 2, 96, 26

# (rows, cin, cout, bias, res) -> (route, calls per forward) of that network
PINNED = {
    (221184, 256, 64, False, False): ('hip', 1),          # patch merging 96^3 -> 48^3
    (27648, 512, 128, False, False): ('hip', 1),          # ... -> 24^3, then down2's two attention blocks and up2's
    (27648, 128, 256, False, False): ('hip', 3),
    (27648, 128, 128, False, True): ('hip', 4),
    (27648, 128, 512, False, False): ('hip', 4),
    (27648, 512, 128, False, True): ('hip', 4),
    (27648, 384, 256, False, False): ('hip', 1),
    (27648, 384, 128, False, False): ('hip', 1),
    (27648, 128, 26, True, False): ('hip_padded', 1),     # the deep-supervision head: 26 -> 28 output rows
    (3456, 1024, 256, False, False): ('hip', 1),          # 12^3: down3, up1
    (3456, 256, 512, False, False): ('hip', 7),
    (3456, 256, 256, False, True): ('hip', 8),
    (3456, 256, 1024, False, False): ('hip', 8),
    (3456, 1024, 256, False, True): ('hip', 8),
    (3456, 576, 512, False, False): ('hip', 1),
    (3456, 576, 256, False, False): ('hip', 1),
    (432, 2048, 320, False, False): ('hip', 1),           # 6^3: down4
    (432, 320, 640, False, False): ('hip', 6),
    (432, 320, 320, False, True): ('hip', 6),
    (432, 320, 1280, False, False): ('hip', 6),
    (432, 1280, 320, False, True): ('hip', 6),
    (54, 128, 256, False, False): ('hip', 4),             # the 27-token semantic maps of two samples
    (54, 128, 128, False, True): ('hip', 3),
    (54, 256, 512, False, False): ('hip', 8),
    (54, 256, 256, False, True): ('hip', 8),
    (54, 320, 640, False, False): ('hip', 6),
    (54, 320, 320, False, True): ('hip', 6),
    (54, 128, 320, False, False): ('hip', 1),             # map fusion: in / out projections
    (54, 256, 320, False, False): ('hip', 1),
    (54, 320, 320, False, False): ('hip', 2),
    (54, 320, 256, False, False): ('hip', 1),
    (54, 320, 128, False, False): ('hip', 1),
    (54, 576, 256, False, False): ('hip', 1),             # map shortcuts of up1 / up2
    (54, 384, 128, False, False): ('hip', 1),
    (162, 320, 960, False, False): ('hip', 2),            # fusion transformer over the 81 tokens
    (162, 320, 320, True, True): ('hip', 4),
    (162, 320, 320, True, False): ('hip', 2),
}


def linear_calls(net, batch, size):
    """Every call of medformer_utils.linear in one forward of `net` on batch x size^3 as (rows, cin, cout, bias, res), from the modules
    the constructor built and the walk of their forward()s (BidirectionAttentionBlock, MBConv, PatchMerging, SemanticMapFusion, up_block,
    the aux head); squeeze-excite, the 3x3x3 convolutions and the output head are other kernels."""
    from rsuper_amd.model.dim3 import medformer_utils as mu
    pw = lambda rows, conv, res=False: (rows, conv.in_channels, conv.out_channels, conv.bias is not None, res)
    lin = lambda rows, l, res=False: (rows, l.in_features, l.out_features, l.bias is not None, res)
    tokens = batch * math.prod(net.down2.map_gen.map_size)
    vox = lambda halvings: batch * (size >> halvings) ** 3
    out = []

    def blocks(layer, V):
        for blk in layer.blocks:
            a, ff = blk.attn, blk.feedforward
            out.extend([pw(V, a.feat_qv.pointwise), pw(tokens, a.map_qv), pw(V, a.feat_out.pointwise, True)])
            if not isinstance(a.map_out, nn.Identity):
                out.append(pw(tokens, a.map_out, True))
            if isinstance(blk.shortcut, mu.GlueConvNormAct):
                out.append(pw(V, blk.shortcut.conv))
            if not isinstance(ff.expand_proj, nn.Identity):
                out.append(pw(V, ff.expand_proj.conv))
            out.append(pw(V, ff.pointwise.conv, True))

    for i, down in enumerate((net.down1, net.down2, net.down3, net.down4), 1):
        out.append(pw(vox(i), down.patch_merging.reduction.pointwise))
        blocks(down.trans_blocks, vox(i))
    out.extend(pw(tokens, p) for p in list(net.map_fusion.in_proj) + list(net.map_fusion.out_proj))
    for attn, ffn in net.map_fusion.fusion.layers:
        T = len(net.map_fusion.in_proj) * tokens
        out.extend([lin(T, attn.fn.to_qkv), lin(T, attn.fn.to_out, True), lin(T, ffn.fn.fc1), lin(T, ffn.fn.fc2, True)])
    for i, up in ((3, net.up1), (2, net.up2), (1, net.up3), (0, net.up4)):
        if not isinstance(up.map_reduction, nn.Identity):
            out.append(pw(tokens, up.map_reduction))
        blocks(up.trans_blocks, vox(i))
    if net.aux_loss:
        out.append(pw(vox(2), net.aux_out))
    return out


def test_every_linear_of_the_shipped_network_runs_on_the_hip_gemm():
    from collections import Counter
    from rsuper_amd.model.dim3 import medformer_utils as mu
    from rsuper_amd.model.dim3.medformer import MedFormer
    with torch.device('meta'):
        net = MedFormer(1, CLASSES, compute_dtype='bf16', **SHIPPED)
    calls = linear_calls(net, B, S)
    got = {k: (mu.linear_route(True, torch.float32, k[0], k[1], k[2], k[4]), n) for k, n in Counter(calls).items()}
    assert got == PINNED, sorted(set(got.items()) ^ set(PINNED.items()))
    assert {r for r, _ in got.values()} == {'hip', 'hip_padded'} and len(calls) == sum(n for _, n in PINNED.values()) == 130
    # the walk saw every 1x1x1 convolution and linear layer the constructor built, bar the output head and squeeze-excite's two
    layers = [m for n, m in net.named_modules() if (isinstance(m, nn.Linear) or (isinstance(m, nn.Conv3d) and m.kernel_size == (1, 1, 1)))
              and n != 'outc' and '.se.' not in n]
    assert len(layers) == len(calls)


F32, BF16 = torch.float32, torch.bfloat16
GIB4_ROWS = (1 << 32) // (4 * 64) - 1           # (rows + 1) * max(cin, cout) * 4 == 4 GiB at 64 channels

EDGES = [
    # is_cuda, dtype, rows, cin, cout, has_res -> route
    ((True, F32, 32, 8, 8, True), 'hip'),
    ((True, F32, 31, 8, 8, True), 'aten'),                        # below POINTWISE_MIN_ROWS
    ((True, F32, 32, 8, 6, False), 'hip_padded'),
    ((True, F32, 31, 8, 6, False), 'aten'),
    ((True, F32, 27648, 128, 26, False), 'hip_padded'),           # the aux head
    ((True, F32, 27648, 128, 26, True), 'library'),               # the padded GEMM takes no shortcut
    ((True, F32, 8191, 128, 26, True), 'aten'),
    ((True, F32, 8191, 30, 128, False), 'aten'),                  # input channels no multiple of 4: never HIP
    ((True, F32, 8192, 30, 128, False), 'library'),
    ((True, F32, 8192, 30, 26, False), 'library'),                # ... padded outputs do not help
    ((True, F32, 8192, 6, 6, False), 'library'),
    ((True, F32, 8192, 8, 6, True), 'library'),
    ((True, BF16, 27648, 128, 128, False), 'aten'),               # bf16 rows: ATen at every size
    ((True, BF16, 27648, 128, 26, False), 'aten'),
    ((True, torch.float16, 32, 8, 8, False), 'aten'),
    ((False, F32, 8191, 128, 128, False), 'aten'),                # host tensors: never HIP
    ((False, F32, 8192, 128, 128, False), 'library'),
    ((False, F32, 8192, 128, 26, False), 'library'),
    ((False, BF16, 8192, 128, 128, False), 'aten'),
    ((True, F32, GIB4_ROWS - 1, 64, 64, False), 'hip'),           # the 4 GiB bound of the kernel's 32-bit byte offsets
    ((True, F32, GIB4_ROWS, 64, 64, False), 'library'),
    ((True, F32, GIB4_ROWS - 1, 64, 62, False), 'hip_padded'),
    ((True, F32, GIB4_ROWS - 1, 64, 66, False), 'library'),       # padded to 68: over the bound
    ((True, F32, 2 * GIB4_ROWS, 32, 32, False), 'hip'),
    ((True, F32, 2 * GIB4_ROWS, 32, 64, False), 'library'),       # the wider side counts
]


@pytest.mark.parametrize('args,route', EDGES)
def test_route_edges(args, route):
    from rsuper_amd.model.dim3 import medformer_utils as mu
    assert mu.linear_route(*args) == route
    assert (mu.POINTWISE_MIN_ROWS, mu.SPLITK_MIN_ROWS) == (32, 8192)


def test_pointwise_supported_is_the_shape_helper():
    """ops.pointwise_supported(x, w) = device and dtype of the tensors + ops.pointwise_shape_supported of their sizes: one copy of the arithmetic."""
    from rsuper_amd.hip import ops
    for rows, cin, cout, ok in ((32, 8, 8, True), (1, 4, 4, True), (32, 8, 6, False), (32, 6, 8, False), (GIB4_ROWS - 1, 64, 64, True),
                                (GIB4_ROWS, 64, 64, False), (GIB4_ROWS, 32, 64, False), (GIB4_ROWS, 32, 32, True)):
        assert ops.pointwise_shape_supported(rows, cin, cout) is ok, (rows, cin, cout)
        for dt in (F32, BF16):
            x, w = torch.empty((rows, cin), dtype=dt, device='meta'), torch.empty((cout, cin), dtype=F32, device='meta')
            assert not ops.pointwise_supported(x, w)                                   # not on the GPU
    import inspect
    assert 'pointwise_shape_supported(' in inspect.getsource(ops.pointwise_supported) and '<<' not in inspect.getsource(ops.pointwise_supported)
