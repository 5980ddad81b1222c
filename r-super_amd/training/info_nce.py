"""InfoNCE with the signature of rsuper_train/training/info_nce.py:63 (itself RElbers/info-nce-pytorch) for the CLIP-like pre-training baseline.

The case the training path uses -- `negative_keys=None`, reduction 'mean': the negatives of a sample are the positive keys of the other samples of
the batch -- is ONE launch that produces the value and the gradients of both inputs (torch.ops.rsuper.info_nce, csrc/cls_branch.hip): rows
L2-normalised as F.normalize does (eps 1e-12), logits = q k^T / temperature, cross-entropy against the diagonal; f64 sums in a fixed order, rounded
once.  Explicit negative keys are not implemented (nothing in the training path passes them).  No CPU fallback."""
from ..hip import ops

__all__ = ['InfoNCE', 'info_nce']


def info_nce(query, positive_key, negative_keys=None, temperature=0.1, reduction='mean', negative_mode='unpaired'):
    if query.dim() != 2:
        raise ValueError('<query> must have 2 dimensions.')
    if positive_key.dim() != 2:
        raise ValueError('<positive_key> must have 2 dimensions.')
    if len(query) != len(positive_key):
        raise ValueError('<query> and <positive_key> must must have the same number of samples.')
    if query.shape[-1] != positive_key.shape[-1]:
        raise ValueError('Vectors of <query> and <positive_key> should have the same number of components.')
    if negative_keys is not None:
        raise NotImplementedError('info_nce on gfx950: explicit negative keys are not implemented (the training path passes none)')
    if reduction != 'mean':
        raise NotImplementedError("info_nce on gfx950: reduction 'mean' only (the training path's)")
    return ops.InfoNceFn.apply(query, positive_key, float(temperature))


class InfoNCE:
    """Callable with the constructor of the reference's nn.Module (it has no parameters)."""

    def __init__(self, temperature=0.1, reduction='mean', negative_mode='unpaired'):
        self.temperature, self.reduction, self.negative_mode = temperature, reduction, negative_mode

    def __call__(self, query, positive_key, negative_keys=None):
        return info_nce(query, positive_key, negative_keys, temperature=self.temperature, reduction=self.reduction, negative_mode=self.negative_mode)
