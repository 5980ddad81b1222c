"""Torch restatements, on the CPU and in any float dtype, of what the multi-task / CLIP baselines compute after the branch's extra layer: the tail of
ClassificationBranch (rsuper_train/model/dim3/medformer.py:65-75 with trans_layers.py:79-118), classification_loss (training/losses_foundation.py
:614-664, the live branches) and info_nce with implicit negatives (training/info_nce.py:63-126).  tests/test_mtl_cpu.py checks them in float32 against
the fixture of the unmodified reference (tests/golden/mtl.npz); the GPU tests evaluate them in float64 on the operands they give the device."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import synth  # noqa: E402

L0 = 'transformer.layers.0.'
TAIL_KEYS = ['reducer.weight', 'reducer.bias', L0 + '0.norm.weight', L0 + '0.norm.bias', L0 + '0.fn.to_qkv.weight', L0 + '0.fn.to_out.weight',
             L0 + '0.fn.to_out.bias', L0 + '1.norm.weight', L0 + '1.norm.bias', L0 + '1.fn.fc1.weight', L0 + '1.fn.fc1.bias', L0 + '1.fn.fc2.weight',
             L0 + '1.fn.fc2.bias', 'head.weight', 'head.bias']

# x4 of the branch-alone cases: (B, 320, s, s, s) -> L = (s / 2)^3 tokens
BRANCH_SHAPES = {'L8': (2, 4), 'L27': (2, 6), 'L64': (1, 8), 'L1': (1, 2)}
BRANCH_NC = (3, 768)
BRANCH_SEED = 21
# whole model: small everywhere but the bottleneck the branches read
MODEL_CFG = dict(base_chan=8, map_size=[2, 2, 2], conv_num=[2, 0, 0, 0, 0, 0, 2, 2], trans_num=[0, 1, 1, 1, 1, 1, 0, 0],
                 chan_num=[16, 32, 64, 320, 64, 32, 16, 8], num_heads=[1, 2, 4, 16, 4, 2, 1, 1], fusion_depth=1, fusion_dim=64, fusion_heads=4,
                 aux_loss=True)
MODEL_SIZE, MODEL_SEED, MODEL_CLS, MODEL_CLIP = 64, 9, ['background', 'kidney_lesion', 'pancreatic_lesion'], 32
LOSS_CLASSES = ['kidney_left', 'kidney_lesion', 'kidney_right', 'pancreas', 'pancreatic_lesion']
NCE_SHAPES = [(1, 768), (2, 768), (5, 7), (8, 768)]
ONK_OLD = sorted(['background', 'aorta', 'kidney_left', 'kidney_right', 'liver', 'pancreas', 'pancreatic_lesion', 'kidney_lesion', 'spleen'])
ONK_NEW = sorted(['background', 'liver', 'pancreas', 'pancreatic_lesion', 'pancreatic_pdac', 'pancreatic_pnet', 'pancreatic_cyst', 'spleen', 'colon_lesion',
                  'adrenal_gland_left'])
ONK_SEED = 1234


def fill(shapes, seed):
    """synth.fill_state_dict with the LayerNorm weights moved to 1 + noise (a LayerNorm weight around 0 would mute the block)."""
    sd = synth.fill_state_dict(shapes, seed)
    return {k: (v + np.float32(1.0) if k.endswith('norm.weight') else v) for k, v in sd.items()}


def x4(tag):
    B, s = BRANCH_SHAPES[tag]
    return synth.rng(300 + s).standard_normal((B, 320, s, s, s)).astype(np.float32)


def out_grad(tag, nc):
    B, _ = BRANCH_SHAPES[tag]
    return synth.rng(400 + nc).standard_normal((B, nc)).astype(np.float32)


def tail(x, p):
    """x (B, L, 160), p: the TAIL_KEYS tensors (reducer.weight as (64, 160, 1, 1, 1) or (64, 160)) -> (B, Nc)."""
    B, L, _ = x.shape
    x0 = F.linear(x, p['reducer.weight'].reshape(64, 160), p['reducer.bias'])
    n1 = F.layer_norm(x0, (64,), p[L0 + '0.norm.weight'], p[L0 + '0.norm.bias'], 1e-5)
    q, k, v = (t.reshape(B, L, 4, 16).transpose(1, 2) for t in F.linear(n1, p[L0 + '0.fn.to_qkv.weight']).chunk(3, -1))
    att = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * 16 ** -0.5, -1)
    o = torch.matmul(att, v).transpose(1, 2).reshape(B, L, 64)
    x1 = x0 + F.linear(o, p[L0 + '0.fn.to_out.weight'], p[L0 + '0.fn.to_out.bias'])
    n2 = F.layer_norm(x1, (64,), p[L0 + '1.norm.weight'], p[L0 + '1.norm.bias'], 1e-5)
    x2 = x1 + F.linear(F.gelu(F.linear(n2, p[L0 + '1.fn.fc1.weight'], p[L0 + '1.fn.fc1.bias'])), p[L0 + '1.fn.fc2.weight'], p[L0 + '1.fn.fc2.bias'])
    return F.linear(x2.mean(1), p['head.weight'], p['head.bias'])


def tail_with_grads(x, params, go, dtype):
    """(out, dx, {key: grad}) of sum(tail(x) * go) evaluated in `dtype`; x, params values, go: numpy / tensors."""
    x = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    p = {k: torch.as_tensor(params[k]).to(dtype).clone().requires_grad_(True) for k in TAIL_KEYS}
    out = tail(x, p)
    (out * torch.as_tensor(go).to(dtype)).sum().backward()
    return out.detach(), x.grad, {k: p[k].grad for k in TAIL_KEYS}


def classification_loss(cls_out, label, unk_voxels, chosen_segment_mask, classes, class_weights=None):
    idx = [i for i, c in enumerate(classes) if 'lesion' in c]
    t = label[:, idx].to(cls_out.dtype)
    if chosen_segment_mask is not None:
        t = t + chosen_segment_mask[:, idx].to(cls_out.dtype)
    t = (t.sum(dim=(-1, -2, -3)) > 0).to(cls_out.dtype)
    loss = F.binary_cross_entropy_with_logits(cls_out, t, reduction='none', weight=class_weights)
    if unk_voxels is not None:
        u = (unk_voxels[:, idx].sum(dim=(-1, -2, -3)) > 0).to(cls_out.dtype)
        loss = loss * (((1 - u) + t) > 0).to(cls_out.dtype)
    return loss.mean()


def info_nce(q, k, temperature=0.1):
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    return F.cross_entropy(q @ k.t() / temperature, torch.arange(len(q)))


def loss_cases():
    """name -> (label, unk or None, mask, class_weights or None) on (2, 5, 16, 16, 16) uint8 volumes, lesion channels 1 and 4."""
    z = lambda: np.zeros((2, 5, 16, 16, 16), np.uint8)
    cases = {}
    lab = z(); lab[0, 1, 3:6, 3:6, 3:6] = 1; lab[1, 0, 2:9, 2:9, 2:9] = 1
    cases['label'] = (lab, z(), z(), None)
    msk = z(); msk[1, 4, 8:12, 8:12, 8:12] = 1
    cases['mask_only'] = (z(), z(), msk, None)
    unk = z(); unk[0, 4, 1:3, 1:3, 1:3] = 1; unk[1, 1, 0, 0, 0] = 1
    cases['unk_zero_target'] = (lab, unk, z(), None)
    unk2 = z(); unk2[0, 1, 4, 4, 4] = 1; unk2[1, 4, 9, 9, 9] = 1
    cases['unk_nonzero_target'] = (lab, unk2, msk, None)
    cases['unk_none'] = (lab, None, msk, None)
    cases['weights'] = (lab, unk, msk, np.array([[0.5, 2.0], [1.5, 0.25]], np.float32))
    cases['all_zero'] = (z(), z(), z(), None)
    return cases


def loss_logits():
    return (synth.rng(501).standard_normal((2, 2)) * 2).astype(np.float32)


def nce_inputs(n, d):
    g = synth.rng(600 + n * 1000 + d)
    return g.standard_normal((n, d)).astype(np.float32), g.standard_normal((n, d)).astype(np.float32)
