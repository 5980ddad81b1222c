"""Multi-task and CLIP baselines, host side: the branch modules and their wiring, the restatements of tests/mtl_ref.py against the fixture of the
unmodified reference (tests/golden/gen_golden_mtl.py -> mtl.npz), and the C ABI of csrc/cls_branch.hip."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import mtl_ref as mr
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def _shapes(g, key):
    return {str(n): tuple(int(d) for d in str(s).split(',')) if str(s) else () for n, s in zip(g[key + '_names'], g[key + '_shapes'])}


def _model(**kw):
    from rsuper_amd.model.dim3.medformer import MedFormer
    return MedFormer(1, len(synth.TINY_CLASSES), **mr.MODEL_CFG, **kw)


def test_branches_construct_with_the_reference_state_dict(golden):
    g = golden['mtl']
    net = _model(classification_branch=True, class_list_cls=mr.MODEL_CLS, clip_branch=True, clip_feats=mr.MODEL_CLIP)
    mine = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert mine == _shapes(g, 'model')
    assert any(k.startswith('classification_branch.extra_layer.') for k in mine) and mine['clip_branch.head.weight'] == (mr.MODEL_CLIP, 64)
    assert mine['classification_branch.reducer.weight'] == (64, 160, 1, 1, 1) and mine['classification_branch.head.bias'] == (3,)
    plain = {k: tuple(v.shape) for k, v in _model().state_dict().items()}
    assert plain == {k: v for k, v in mine.items() if not k.startswith(('classification_branch.', 'clip_branch.'))}      # nothing else changed
    bare = _model()
    assert bare.classification_branch is None and bare.clip_branch is None
    from rsuper_amd.model.dim3.medformer import ClassificationBranch
    br = ClassificationBranch()                                       # the reference's constructor defaults
    assert br.head.weight.shape == (3, 64) and br.reducer.weight.shape == (64, 160, 1, 1, 1) and br.extra_layer is None
    assert {k: tuple(v.shape) for k, v in br.state_dict().items()} == _shapes(g, 'branch_L1_3')
    with pytest.raises(ValueError):                                  # the reducer reads 160 channels: chan_num[3] must be 320
        from rsuper_amd.model.dim3.medformer import MedFormer
        MedFormer(1, 5, **{**mr.MODEL_CFG, 'chan_num': [16, 32, 64, 80, 64, 32, 16, 8], 'num_heads': [1, 2, 4, 5, 4, 2, 1, 1]}, clip_branch=True)


def test_get_model_builds_the_branches():
    import yaml
    from rsuper_amd.model.utils import get_model
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'r-super_amd', 'config', 'abdomenatlas_ufo', 'medformer_3d.yaml')))
    classes = ['background', 'kidney_left', 'kidney_lesion', 'pancreas', 'pancreatic_cyst', 'pancreatic_pdac', 'pancreatic_pnet', 'spleen']
    args = argparse.Namespace(model='medformer', dimension='3d', **{**cfg, 'classification_branch': True})
    net = get_model(args, classes=classes)
    assert net.classification_branch.head.out_features == 5 and net.clip_branch is None          # background, lesion, cyst, pdac, pnet
    assert net.outc.out_channels == len(classes)
    net = get_model(args, classes=classes, classes_cls=['a', 'b'])
    assert net.classification_branch.head.out_features == 2
    net = get_model(argparse.Namespace(**{**vars(args), 'classification_branch': False, 'clip_loss': True}), classes=classes)
    assert net.classification_branch is None and net.clip_branch.head.out_features == 768
    with pytest.raises(NotImplementedError, match='class list'):
        get_model(args)


@pytest.mark.parametrize('tag,copy_pancreas', [('plain', False), ('copy_pancreas', True)])
def test_update_output_layer_rewires_the_classification_head(golden, tag, copy_pancreas):
    import torch.nn as nn
    from rsuper_amd.model.dim3.medformer import update_output_layer_onk
    g = golden['mtl']

    class Carrier(nn.Module):
        def __init__(self, n, n_cls):
            super().__init__()
            self.aux_loss = True
            self.outc = nn.Conv3d(8, n, kernel_size=1)
            self.aux_out = nn.Conv3d(32, n, kernel_size=1)
            self.classification_branch = nn.Module()
            self.classification_branch.head = nn.Linear(64, n_cls)
    car = Carrier(len(mr.ONK_OLD), len([c for c in mr.ONK_OLD if 'lesion' in c]))
    shapes = {k: tuple(v.shape) for k, v in car.state_dict().items()}
    car.load_state_dict({k: T(v) for k, v in mr.fill(shapes, 11).items()})
    torch.manual_seed(mr.ONK_SEED)
    update_output_layer_onk(car, original_classes=mr.ONK_OLD, new_classes=mr.ONK_NEW, copy_pancreas=copy_pancreas)
    sd = car.state_dict()
    assert sd['classification_branch.head.weight'].shape == (6, 64)
    for k, v in sd.items():                                        # copied rows and, through the creation order, the fresh rows too
        assert np.array_equal(v.numpy(), g[f'onk_{tag}.{k}']), k


def test_update_output_layer_on_a_branched_medformer(golden):
    """The same surgery on a MedFormer built with the branch (on the host): head rebuilt for the derived class list in the dtype of the old one,
    rows of the old lesion classes copied, the rest of the branch untouched, and the tail's parameter list follows the new head."""
    from rsuper_amd.model.dim3.medformer import MedFormer, update_output_layer_onk
    old_cls = [c for c in mr.ONK_OLD if 'lesion' in c]
    net = MedFormer(1, len(mr.ONK_OLD), classification_branch=True, class_list_cls=old_cls, **mr.MODEL_CFG)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    ret = update_output_layer_onk(net, original_classes=mr.ONK_OLD, new_classes=mr.ONK_NEW, copy_pancreas=True)
    assert ret is net
    new_cls = [c for c in mr.ONK_NEW if any(p in c for p in ('background', 'lesion', 'pdac', 'pnet', 'cyst'))]
    head = net.classification_branch.head
    assert head.weight.shape == (len(new_cls), 64) and head.weight.dtype == before['classification_branch.head.weight'].dtype
    pan = before['classification_branch.head.weight'][old_cls.index('pancreatic_lesion')]
    for i, c in enumerate(new_cls):
        if c in old_cls:
            assert torch.equal(head.weight[i], before['classification_branch.head.weight'][old_cls.index(c)]), c
        elif c not in mr.ONK_OLD:                                   # copy_pancreas: classes new to the old list take the pancreatic_lesion row
            assert torch.equal(head.weight[i], pan), c
    assert net.classification_branch.tail_parameters()[13] is head.weight and net.outc.out_channels == len(mr.ONK_NEW)
    after = net.state_dict()
    untouched = [k for k in before if not k.startswith(('outc.', 'aux_out.', 'classification_branch.head.'))]
    assert all(torch.equal(before[k], after[k]) for k in untouched)


def _close(a, b, rel=2e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-30), (np.abs(a - b).max(), np.abs(b).max())


@pytest.mark.parametrize('tag', list(mr.BRANCH_SHAPES))
@pytest.mark.parametrize('nc', mr.BRANCH_NC)
def test_tail_restatement_matches_the_reference_in_float32(golden, tag, nc):
    g = golden['mtl']
    key = f'branch_{tag}_{nc}'
    params = mr.fill(_shapes(g, f'branch_{"L1" if tag == "L1" else "L8"}_{nc}'), mr.BRANCH_SEED)
    out, dx, grads = mr.tail_with_grads(g[f'branch_{tag}_xtail'], params, mr.out_grad(tag, nc), torch.float32)
    _close(out, g[key + '_out'])
    _close(synth.subsample(dx.numpy(), len(g[key + '_dxtail_sub']))[0], g[key + '_dxtail_sub'], 1e-4)
    for k in mr.TAIL_KEYS:
        ref = g[f'{key}_g_{k}_sub']
        _close(synth.subsample(grads[k].numpy(), 1024 if grads[k].numel() > 4096 else grads[k].numel())[0], ref, 1e-4)


def test_loss_restatements_match_the_reference_in_float32(golden):
    g = golden['mtl']
    for name, (lab, unk, msk, cw) in mr.loss_cases().items():
        x = T(mr.loss_logits()).requires_grad_(True)
        l = mr.classification_loss(x, T(lab), None if unk is None else T(unk), T(msk), mr.LOSS_CLASSES, None if cw is None else T(cw))
        l.backward()
        _close(l.detach(), g[f'cls_{name}_value'], 1e-6)
        _close(x.grad, g[f'cls_{name}_grad'], 1e-6)
    assert float(g['cls_unk_zero_target_grad'][1, 0]) == 0.0 and float(g['cls_unk_nonzero_target_grad'][0, 0]) != 0.0      # masked / kept entries
    for n, d in mr.NCE_SHAPES:
        q, k = (T(a).requires_grad_(True) for a in mr.nce_inputs(n, d))
        l = mr.info_nce(q, k)
        l.backward()
        _close(l.detach(), g[f'nce_{n}_{d}_value'], 1e-6)
        _close(q.grad, g[f'nce_{n}_{d}_dq'], 1e-5)
        _close(k.grad, g[f'nce_{n}_{d}_dk'], 1e-5)
    q, k = (T(a) for a in mr.nce_inputs(2, 768))
    sym = 0.5 * (mr.info_nce(q, k) + mr.info_nce(k, q)) * 2
    _close(sym, g['clip_only_value'], 1e-6)


NEW_SYMBOLS = {'rsuper_cls_tail_supported': 2, 'rsuper_cls_tail_save_floats': 1, 'rsuper_cls_tail_param_floats': 1, 'rsuper_cls_tail_partial_floats': 2,
               'rsuper_cls_tail_fwd': 8, 'rsuper_cls_tail_bwd': 11, 'rsuper_cls_loss': 12, 'rsuper_info_nce_supported': 2, 'rsuper_info_nce': 9}


def test_new_symbols_are_declared_bound_and_exported():
    from rsuper_amd.hip import lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read(), flags=re.S)
    for name, arity in NEW_SYMBOLS.items():
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/rsuper_hip.h'
        assert len([p for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']) == arity == len(lib._SIGS[name][1]), name
        assert name in lib.exported_symbols() and hasattr(lib.lib(), name)
    L = lib.lib()
    assert [L.rsuper_cls_tail_supported(*a) for a in [(1, 1), (27, 3), (64, 768), (65, 3), (0, 3)]] == [1, 1, 1, 0, 0]      # answered on the host
    assert L.rsuper_cls_tail_supported(8, 769) == 0 and L.rsuper_cls_tail_supported(8, 0) == 0
    assert L.rsuper_cls_tail_param_floats(3) == 64 * 160 + 64 + 128 + 192 * 64 + 64 * 64 + 64 + 128 + 320 * 64 + 320 + 64 * 320 + 64 + 3 * 64 + 3
    assert L.rsuper_cls_tail_save_floats(64) > 0 and L.rsuper_cls_tail_save_floats(65) == 0
    assert L.rsuper_info_nce_supported(8, 768) == 1 and L.rsuper_info_nce_supported(65, 8) == 0
    # refused before anything is launched
    assert L.rsuper_cls_tail_fwd(None, None, None, None, 1, 8, 3, None) == 1
    assert L.rsuper_info_nce(None, None, 2, 4, 0.1, None, None, None, None) == 1


def test_operators_have_no_cpu_kernel():
    from rsuper_amd.hip import ops, library   # noqa: F401
    from rsuper_amd.training import losses_foundation as lf
    from rsuper_amd.training.info_nce import info_nce
    for n in ('cls_tail', 'info_nce', 'classification_loss'):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'rsuper::{n}', 'CUDA')
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'rsuper::{n}', 'AutogradCUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'rsuper::{n}', 'CPU')
    shapes = [(64, 160), (64,), (64,), (64,), (192, 64), (64, 64), (64,), (64,), (64,), (320, 64), (320,), (64, 320), (64,), (3, 64), (3,)]
    with pytest.raises(NotImplementedError):
        torch.ops.rsuper.cls_tail(torch.zeros(1, 8, 160), *[torch.zeros(s) for s in shapes])
    with pytest.raises(NotImplementedError):
        torch.ops.rsuper.info_nce(torch.zeros(2, 8), torch.zeros(2, 8), 0.1)
    with pytest.raises((NotImplementedError, RuntimeError)):
        info_nce(torch.zeros(2, 8), torch.zeros(2, 8))
    with pytest.raises(NotImplementedError):                        # explicit negatives are not part of the training path
        info_nce(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(3, 8))
    with pytest.raises(RuntimeError):                               # no CPU fallback of the loss either
        lf.classification_loss(torch.zeros(2, 2), torch.zeros(2, 5, 4, 4, 4), None, None, None, mr.LOSS_CLASSES)
    with pytest.raises(ValueError):                                 # wrong class count, as torch's BCE
        lf.classification_loss(torch.zeros(2, 3), torch.zeros(2, 5, 4, 4, 4), None, None, None, mr.LOSS_CLASSES)
