"""rsuper_train/metric/utils.py: calculate_distance (:8-26), calculate_dice_split (:30-49), calculate_dice (:59-79) on device tensors.

Reference quirks fixed here on purpose (in the style of SURVEY Appendix A):
  * calculate_distance :19 slices `label_true[:, i+1]`, which on the (C, D, H, W) stacks validation() passes is a depth slice of every channel, not
    channel i+1.  Here the channel axis is axis 0 and `channels` names the planes that are measured.
  * calculate_dice_split :43 reads the loop variable `i` after a loop that may not have run (N < block_size): a NameError.  Here the tail block
    starts at split_num * block_size.
"""
import numpy as np
import torch

from ..hip.lib import RSuperHipError
from . import metrics


def calculate_distance(label_pred, label_true, spacing, C, percentage=95, channels=None, area_table=None):
    """label_pred, label_true: (C, D, H, W) bool / uint8 stacks on the device; spacing: 3 values (tensor, array or list).  All requested channels
    run in batched launches.  Returns (ASD, HD) float64 numpy arrays, one entry per channel: ASD = mean of the two average surface distances, HD
    = robust Hausdorff at `percentage`.  channels=None means range(1, C): the reference's count, background excluded."""
    if label_pred.dim() != 4 or label_pred.shape != label_true.shape or label_pred.shape[0] != C:
        raise RSuperHipError(f'calculate_distance: two (C={C}, D, H, W) stacks, got {tuple(label_pred.shape)} and {tuple(label_true.shape)}')
    channels = list(range(1, C)) if channels is None else [int(c) for c in channels]
    if hasattr(spacing, 'detach'):
        spacing = spacing.detach().cpu().numpy()
    spacing = [float(s) for s in np.asarray(spacing).reshape(-1)]
    ASD, HD = np.zeros(len(channels)), np.zeros(len(channels))
    if not channels:
        return ASD, HD
    whole = channels == list(range(C))
    gt = label_true if whole else label_true[channels]
    pred = label_pred if whole else label_pred[channels]
    results, _ = metrics.surface_distances_stack(gt, pred, spacing, area_table)
    for i, sd in enumerate(results):
        a, b = metrics.compute_average_surface_distance(sd)
        ASD[i] = (a + b) / 2
        HD[i] = metrics.compute_robust_hausdorff(sd, percentage)
    return ASD, HD


def calculate_dice(pred, target, C):
    """pred, target: (N, 1) integer label vectors.  Returns (dice, intersection, summ) float32 (C,) tensors: intersection[c] = #(pred == c and
    target == c), summ[c] = #(pred == c) + #(target == c) + 1e-5, dice = 2 * intersection / summ -- the reference's one-hot scatter as counts."""
    p, t = pred.reshape(-1).long(), target.reshape(-1).long()
    assert p.shape == t.shape
    inter = torch.bincount(t[p == t], minlength=C)[:C].to(torch.float32)
    summ = (torch.bincount(p, minlength=C)[:C] + torch.bincount(t, minlength=C)[:C]).to(torch.float32)
    summ += 1e-5
    return 2 * inter / summ, inter, summ


def calculate_dice_split(pred, target, C, block_size=64 * 64 * 64):
    """calculate_dice block by block with float32 totals, dice = 2 * total_intersection / (total_sum + 1e-5) (every block's summ already carries
    its own + 1e-5, as in the reference)."""
    assert pred.shape[0] == target.shape[0]
    N = pred.shape[0]
    total_sum = torch.zeros(C, device=pred.device)
    total_intersection = torch.zeros(C, device=pred.device)
    for s in range(0, N, block_size):
        _, inter, summ = calculate_dice(pred[s:s + block_size], target[s:s + block_size], C)
        total_intersection += inter
        total_sum += summ
    return 2 * total_intersection / (total_sum + 1e-5), total_intersection, total_sum
