"""MedFormer with the constructor and state_dict of rsuper_train/model/dim3/medformer.py:81-175 -- the network R-Super actually
trains.  forward returns {'segmentation': logits} or {'segmentation': [logits, aux_logits]} with aux_loss
(prepare_return, medformer.py:205-222), which is what calculate_loss consumes.

Execution: conv stem, BasicBlock stages, the trilinear up-sampling in front of them and the 1x1x1 output head on the gfx950 kernels
(bf16 or f32 `compute_dtype`); patch merging, semantic maps and the bidirectional-attention stages as fp32 PyTorch-ROCm ops for
now (medformer_utils.py explains the split).  The classification / CLIP branches of the multi-task and CLIP baselines (medformer.py:12-78, :148-158)
read the bottleneck: `ClassificationBranch` below, its tail on csrc/cls_branch.hip.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import medformer_utils as _mu
from .medformer_utils import Feat, inconv, down_block, up_block, SemanticMapFusion, TransformerBlock, pointwise, linear, upsample_trilinear
from ...hip import ops, lib as _lib

_DEFAULTS = dict(conv_num=[2, 1, 0, 0, 0, 1, 2, 2], trans_num=[0, 1, 2, 2, 2, 1, 0, 0], chan_num=[64, 128, 256, 320, 256, 128, 64, 32],
                 num_heads=[1, 4, 8, 16, 8, 4, 1, 1])


# RSUPER_MF_CLS_FUSED=0: the tail of ClassificationBranch through pointwise / TransformerBlock / linear instead of csrc/cls_branch.hip (A/B switch)
CLS_FUSED = os.environ.get('RSUPER_MF_CLS_FUSED', '1') == '1'


class ClassificationBranch(nn.Module):
    """Classification / CLIP head on the bottleneck (medformer.py:12-78), constructor defaults and state_dict of the reference: `extra_layer` (a
    down_block with one attention stage and map generation) halves the grid, then reducer Conv3d(in_dim, reduced_dim, 1) -> TransformerBlock(depth 1)
    -> mean over the tokens -> Linear(reduced_dim, num_classes).  With the default sizes and at most 64 tokens everything after `extra_layer` is
    ONE launch per direction (torch.ops.rsuper.cls_tail, csrc/cls_branch.hip); other sizes, more tokens or RSUPER_MF_CLS_FUSED=0 take the same
    chain through pointwise / TransformerBlock / linear.  `x + 0 * tmp_map.sum()` (medformer.py:77) is kept: the parameters that feed only the
    branch's semantic map end a backward with a zero-filled gradient instead of none (clip_grad_norm_, the fused optimiser and the bucketed
    reducer see every parameter).  The reference's `segmentation_out` / `voxel_choice` inputs are never passed by MedFormer and are not taken."""

    def __init__(self, in_dim=160, reduced_dim=64, heads=4, dim_head=16, mlp_dim=320, num_classes=3, extra_layer=None, reducer=True):
        super().__init__()
        self.reducer = nn.Conv3d(in_dim, reduced_dim, kernel_size=1) if reducer else nn.Identity()
        self.extra_layer = extra_layer
        self.transformer = TransformerBlock(dim=reduced_dim, depth=1, heads=heads, dim_head=dim_head, mlp_dim=mlp_dim)
        self.head = nn.Linear(reduced_dim, num_classes)
        self._default_sizes = bool(reducer) and (in_dim, reduced_dim, heads, dim_head, mlp_dim) == (160, 64, 4, 16, 320)

    def tail_parameters(self):
        """The 15 parameters of the tail in the order torch.ops.rsuper.cls_tail takes them."""
        attn, ffn = self.transformer.layers[0]
        return (self.reducer.weight.reshape(self.reducer.weight.shape[0], -1), self.reducer.bias, attn.norm.weight, attn.norm.bias, attn.fn.to_qkv.weight,
                attn.fn.to_out.weight, attn.fn.to_out.bias, ffn.norm.weight, ffn.norm.bias, ffn.fn.fc1.weight, ffn.fn.fc1.bias, ffn.fn.fc2.weight,
                ffn.fn.fc2.bias, self.head.weight, self.head.bias)

    def fused(self, tokens):
        """Whether a (B, L, C) token tensor takes the one-launch tail."""
        return (CLS_FUSED and self._default_sizes and tokens.is_cuda and tokens.dtype == torch.float32
                and ops.cls_tail_supported(tokens.shape[1], self.head.out_features))

    def tail(self, g):
        """g: (B, d, h, w, in_dim) f32 channels-last -> (B, num_classes)."""
        tokens = g.flatten(1, 3)
        if self.fused(tokens):
            return ops.ClsTailFn.apply(tokens.contiguous(), *self.tail_parameters())
        f32 = torch.float32                                            # f32 operands in both compute modes, like the fused kernel
        x = g if isinstance(self.reducer, nn.Identity) else pointwise(g, self.reducer, compute=f32)
        x = self.transformer(x.flatten(1, 3), compute=f32)
        return linear(x.mean(dim=1), self.head.weight, self.head.bias, compute=f32)

    def forward(self, x, dtype=torch.float32):
        """x: the bottleneck as a `Feat`."""
        if self.extra_layer is not None:
            x, tmp_map = self.extra_layer(x, dtype)
        else:
            tmp_map = torch.zeros(1, device=x.g().device)
        y = self.tail(x.g())
        return y + 0 * tmp_map.sum()


class MedFormer(nn.Module):
    def __init__(self, in_chan, num_classes, base_chan=32, map_size=[4, 8, 8], conv_block='BasicBlock', conv_num=None, trans_num=None,
                 chan_num=None, num_heads=None, fusion_depth=2, fusion_dim=320, fusion_heads=4, expansion=4, attn_drop=0., proj_drop=0.,
                 proj_type='depthwise', norm='in', act='relu', kernel_size=[3, 3, 3, 3], scale=[2, 2, 2, 2], aux_loss=False,
                 classification_branch=False, class_list_seg=None, class_list_cls=None, clip_branch=False, clip_feats=768,
                 compute_dtype=None):
        super().__init__()
        conv_num, trans_num = conv_num or _DEFAULTS['conv_num'], trans_num or _DEFAULTS['trans_num']
        chan_num, num_heads = chan_num or _DEFAULTS['chan_num'], num_heads or _DEFAULTS['num_heads']
        act_name = act if isinstance(act, str) else getattr(act, '__name__', str(act)).lower()
        if conv_block != 'BasicBlock' or norm != 'in' or act_name != 'relu' or proj_type != 'depthwise':
            raise NotImplementedError("MedFormer on gfx950: conv_block='BasicBlock', norm='in', act='relu', proj_type='depthwise' "
                                      '(config/abdomenatlas_ufo/medformer_3d.yaml)')
        if (classification_branch or clip_branch) and chan_num[3] != 320:
            # the branch's reducer is Conv3d(160, 64, 1) whatever chan_num says (medformer.py:13, :149): the reference fails at the first forward
            raise ValueError('classification / CLIP branches need chan_num[3] == 320 (their reducer reads 160 channels), got %d' % chan_num[3])
        if classification_branch and class_list_cls is None:
            raise NotImplementedError('classification_branch needs the class list (class_list_cls): it sizes the head')
        if attn_drop or proj_drop:
            raise NotImplementedError('dropout is 0 in every shipped MedFormer configuration')
        flat = lambda v: [tuple(t) if isinstance(t, (list, tuple)) else (t,) * 3 for t in v]
        if any(k != (3, 3, 3) for k in flat(kernel_size)) or any(s != (2, 2, 2) for s in flat(scale)):
            raise NotImplementedError('kernel size 3 and scale 2 at every stage (shipped configuration)')
        if in_chan != 1 or base_chan % 8 or base_chan > 32 or num_classes > 64:
            raise NotImplementedError('in_chan 1, base_chan a multiple of 8 and <= 32, <= 64 classes (stem / head kernels)')
        c, h = chan_num, num_heads
        dh = [c[i] // h[i] for i in range(8)]
        self.inc = inconv(in_chan, base_chan)
        self.down1 = down_block(base_chan, c[0], conv_num[0], trans_num[0], map_generate=False)
        self.down2 = down_block(c[0], c[1], conv_num[1], trans_num[1], h[1], dh[1], expansion, map_size, True)
        self.down3 = down_block(c[1], c[2], conv_num[2], trans_num[2], h[2], dh[2], expansion, map_size, True)
        self.down4 = down_block(c[2], c[3], conv_num[3], trans_num[3], h[3], dh[3], expansion, map_size, True)
        self.map_fusion = SemanticMapFusion(c[1:4], fusion_dim, fusion_heads, depth=fusion_depth)
        self.up1 = up_block(c[3], c[4], conv_num[4], trans_num[4], h[4], dh[4], expansion, map_shortcut=True)
        self.up2 = up_block(c[4], c[5], conv_num[5], trans_num[5], h[5], dh[5], expansion, map_shortcut=True, no_map_out=True)
        self.up3 = up_block(c[5], c[6], conv_num[6], trans_num[6])
        self.up4 = up_block(c[6], c[7], conv_num[7], trans_num[7])
        self.aux_loss = bool(aux_loss)
        if aux_loss:
            self.aux_out = nn.Conv3d(c[5], num_classes, kernel_size=1)
        self.outc = nn.Conv3d(c[7], num_classes, kernel_size=1)
        branch = lambda n: ClassificationBranch(num_classes=n, extra_layer=down_block(c[3], c[3] // 2, 0, 1, 4, dh[3], expansion, map_size, True))
        self.classification_branch = branch(len(class_list_cls)) if classification_branch else None      # medformer.py:148-158, in this order
        self.clip_branch = branch(clip_feats) if clip_branch else None
        self.compute_dtype = compute_dtype or os.environ.get('RSUPER_DTYPE', 'bf16')

    def _dtype(self):
        return {'bf16': torch.bfloat16, 'f32': torch.float32}[self.compute_dtype]

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.RSuperHipError('rsuper_amd MedFormer runs on MI355X only (no CPU fallback); move the input to cuda')
        _lib.require_device()
        dt = self._dtype()
        # the 1x1x1 GEMMs of the attention stages keep fp32 storage (bf16 storage was measured, then removed: 47-53 vs 44 ms/step, the casts
        # around every GEMM cost more than the faster MFMA rate saves at these sizes)
        _mu.GEMM_COMPUTE = dt                      # HIP pointwise GEMMs: bf16 MFMA operands in the bf16 mode, exact-f32 MFMA in the parity mode
        ops.pointwise_prepack(dt)                  # MFMA fragments of every 1x1x1 / linear weight of the attention stages: one launch per step
        x0 = self.inc(x, dt)
        x1, _ = self.down1(x0, dt)
        x2, m2 = self.down2(x1, dt)
        x3, m3 = self.down3(x2, dt)
        x4, m4 = self.down4(x3, dt)
        extra = {}
        if self.classification_branch is not None:             # multi-task baseline (medformer.py:174-182, :217-220)
            extra['classification'] = self.classification_branch(x4, dt)
        if self.clip_branch is not None:                       # CLIP baseline
            extra['clip'] = self.clip_branch(x4, dt)
        maps = self.map_fusion([m2, m3, m4])
        out, smap = self.up1(x4, x3, maps[2], maps[1], dt)
        out, smap = self.up2(out, x2, smap, maps[0], dt)
        aux = None
        if self.aux_loss:                                      # deep supervision head at 1/4 resolution, up-sampled (medformer.py:190-194)
            aux = upsample_trilinear(pointwise(out.g(), self.aux_out), x.shape[-3:], planar=True)
        out, smap = self.up3(out, x1, smap, None, dt)
        out, smap = self.up4(out, x0, smap, None, dt)
        feat, _ = out.cl(dt)
        logits = ops.HeadFn.apply(feat, self.outc.weight, self.outc.bias)
        return {'segmentation': [logits, aux] if self.aux_loss else logits, **extra}


def update_output_layer_onk(model, original_classes, new_classes, copy_pancreas=False):
    """Output-layer surgery for the public checkpoints (medformer.py:224-319, call site train_ddp.py:574-580 `--update_output_layer`): the 1x1x1
    heads `model.outc` and -- with deep supervision -- `model.aux_out` are rebuilt for `new_classes`; the row of every class that also exists in
    `original_classes` is copied from the old head, with `copy_pancreas` (the `--no_mask` runs) the remaining rows take the 'pancreatic_lesion' row,
    otherwise they keep the fresh nn.Conv3d initialisation.  A head that already has len(new_classes) outputs is left untouched, as in the reference.
    The new layers are created in the reference's order (outc, then aux_out) so a seeded run draws the same initial rows; they live on the device and
    in the dtype of the layers they replace.  Then, as in the reference (:293-315), the head of the classification branch is rebuilt for the
    classification classes of `new_classes` (names with background / lesion / pdac / pnet / cyst): rows of classes that are also `lesion` entries of
    `original_classes` are copied -- the old head's rows are indexed by that lesion list -- and `copy_pancreas` gives the classes new to
    `original_classes` the 'pancreatic_lesion' row.  Returns the model."""
    def update_conv(old_conv, full_class_list):
        new_conv = nn.Conv3d(old_conv.in_channels, len(full_class_list), kernel_size=old_conv.kernel_size, stride=old_conv.stride, padding=old_conv.padding,
                             dilation=old_conv.dilation, groups=old_conv.groups, bias=old_conv.bias is not None)
        new_conv = new_conv.to(device=old_conv.weight.device, dtype=old_conv.weight.dtype)
        with torch.no_grad():
            for new_idx, new_cls in enumerate(full_class_list):
                src = None
                if new_cls in original_classes:
                    src = original_classes.index(new_cls)
                elif copy_pancreas:
                    src = original_classes.index('pancreatic_lesion')          # ValueError when the old list has no such class, as in the reference
                if src is not None:
                    new_conv.weight[new_idx] = old_conv.weight[src]
                    if old_conv.bias is not None:
                        new_conv.bias[new_idx] = old_conv.bias[src]
        return new_conv

    original_classes, new_classes = list(original_classes), list(new_classes)
    if model.outc.out_channels != len(new_classes):
        model.outc = update_conv(model.outc, new_classes)
    if hasattr(model, 'aux_out') and model.aux_loss and model.aux_out.out_channels != len(new_classes):
        model.aux_out = update_conv(model.aux_out, new_classes)
    if getattr(model, 'classification_branch', None) is not None:
        new_cls = [c for c in new_classes if any(p in c for p in ('background', 'lesion', 'pdac', 'pnet', 'cyst'))]
        old_cls = [c for c in original_classes if 'lesion' in c]
        old_head = model.classification_branch.head
        if old_head.out_features != len(new_cls):
            new_head = nn.Linear(old_head.in_features, len(new_cls)).to(device=old_head.weight.device, dtype=old_head.weight.dtype)
            with torch.no_grad():
                for new_idx, c in enumerate(new_cls):
                    src = None
                    if c not in original_classes and copy_pancreas:
                        src = old_cls.index('pancreatic_lesion')              # ValueError when the old list has no such class, as in the reference
                    if c in old_cls:
                        src = old_cls.index(c)
                    if src is not None:
                        new_head.weight[new_idx] = old_head.weight[src]
                        if old_head.bias is not None:
                            new_head.bias[new_idx] = old_head.bias[src]
            model.classification_branch.head = new_head
    return model
