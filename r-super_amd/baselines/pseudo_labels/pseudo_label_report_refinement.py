"""Report-guided refinement of pseudo-labels (rsuper_train/baselines/pseudo_labels/pseudo_label_report_refinement.py) on the MI355X path:
extract_lesion_candidates (:48-70), the per-case decision of process_bdmap (:89-155) as `refine_case`, and the helpers slice_indices, load_yaml and
dump_yaml under the reference's names.

The reference runs the candidate loop in host scipy: per iteration a global max / argmax, a threshold at peak_cut * peak, a 26-connected
ndimage.label of the whole volume, a component pick and a zero-out.  Here the probabilities `predict_case` returns stay on the device and the loop
runs there (csrc/pseudo_label.hip, `torch.ops.rsuper.lesion_candidates`): all lesion planes of a case advance in the same launches, each with its own
counters, and loop control is predicated on the device -- the host enqueues `batch` iterations back to back, reads the 32-byte state of each plane
once, and repeats while a plane is unfinished.  Iterations enqueued past a plane's end change nothing.  The results are the reference's, bit for bit.
"""
import ctypes

import numpy as np
import torch

from ...hip import lib as _l
from ...hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ...hip import library as _library

MAX_PLANES = 64            # RSUPER_LESION_MAX_PLANES of the header: planes per launch group (more planes run as several groups)
STATE_WORDS = 8            # RSUPER_LESION_STATE_WORDS: kept, iterations, done, n_lesions, peak key (2 words), seed root, seed component size
DEFAULT_BATCH = 4          # iterations enqueued per read of the state block, see extract_lesion_candidates

# what the last extract_lesion_candidates / lesion_candidates call did, per plane: 'kept', 'iterations' (labelling passes, the reference's loop count),
# 'reads' (device-to-host reads of the state block until the plane was finished; 0 for a plane with n_lesions <= 0), and the 'batch' used
last_state = {'kept': [], 'iterations': [], 'reads': [], 'batch': DEFAULT_BATCH}


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _check_params(peak_cut, min_voxels, min_peak, batch):
    """The bounds of the C ABI, in the float32 the kernels compare in.  The reference has no such check: with peak_cut <= 0 or min_peak <= 0 its loop
    does not end on an all-zero volume, with peak_cut > 1 the peak voxel is outside its own mask and another component is picked."""
    pc, mp = np.float32(peak_cut), np.float32(min_peak)
    if not (pc > 0 and pc <= 1):
        raise ValueError(f'extract_lesion_candidates: peak_cut must satisfy 0 < peak_cut <= 1 in float32, got {peak_cut!r}')
    if not mp > 0:
        raise ValueError(f'extract_lesion_candidates: min_peak must be > 0 in float32, got {min_peak!r}')
    if int(min_voxels) != min_voxels or min_voxels < 1:
        raise ValueError(f'extract_lesion_candidates: min_voxels must be an integer >= 1, got {min_voxels!r}')
    if int(batch) != batch or batch < 1:
        raise ValueError(f'extract_lesion_candidates: batch must be an integer >= 1, got {batch!r}')


def _lesion_candidates_impl(prob, n_lesions, peak_cut, min_voxels, min_peak, batch):
    """The C ABI calls.  prob (P, D, H, W) float32 on the device -> (mask (P, D, H, W) uint8, state (P, STATE_WORDS) int32 on the device)."""
    if prob.dim() != 4 or prob.dtype != torch.float32:
        raise ValueError(f'lesion_candidates: a float32 (P, D, H, W) stack, got {prob.dtype} {tuple(prob.shape)}')
    P, D, H, W = prob.shape
    if len(n_lesions) != P:
        raise ValueError(f'lesion_candidates: {len(n_lesions)} lesion counts for {P} planes')
    if min(D, H, W) < 1 or D * H * W > 2 ** 31:
        raise ValueError(f'lesion_candidates: planes of 1 .. 2^31 voxels, got {(D, H, W)}')
    _check_params(peak_cut, min_voxels, min_peak, batch)
    counts = [max(int(n), 0) for n in n_lesions]
    L = _l.lib()
    work = prob.contiguous().clone()                      # consumed in place; the caller's tensor stays as it is
    out = torch.empty((P, D, H, W), device=prob.device, dtype=torch.uint8)
    state = torch.empty((P, STATE_WORDS), device=prob.device, dtype=torch.int32)
    reads = [0] * P
    with torch.cuda.device(prob.device):
        st = _stream(prob)
        for p0 in range(0, P, MAX_PLANES):
            n = min(MAX_PLANES, P - p0)
            ws = torch.empty((L.rsuper_lesion_candidates_workspace_bytes(n, D, H, W),), device=prob.device, dtype=torch.uint8)
            w, o, s = work[p0:p0 + n], out[p0:p0 + n], state[p0:p0 + n]
            _l.check(L.rsuper_lesion_candidates_begin(o.data_ptr(), n, D, H, W, (ctypes.c_int * n)(*counts[p0:p0 + n]), s.data_ptr(), st),
                     'lesion_candidates_begin')
            open_planes = [p for p in range(n) if counts[p0 + p] > 0]
            k = 0
            while open_planes:
                if k * int(batch) > D * H * W:            # every iteration of an open plane zeroes a voxel or ends the plane: cannot happen
                    raise _l.RSuperHipError('lesion_candidates: a plane is still open after D*H*W iterations')
                _l.check(L.rsuper_lesion_candidates_run(w.data_ptr(), o.data_ptr(), n, D, H, W, float(peak_cut), int(min_voxels), float(min_peak),
                                                        s.data_ptr(), ws.data_ptr(), int(batch), st), 'lesion_candidates_run')
                host = s.cpu()                            # the one synchronising read per batch
                k += 1
                still = []
                for p in open_planes:
                    if host[p, 2] != 0 or host[p, 0] >= counts[p0 + p]:
                        reads[p0 + p] = k
                    else:
                        still.append(p)
                open_planes = still
    final = state.cpu()
    last_state.update(kept=[int(v) for v in final[:, 0]], iterations=[int(v) for v in final[:, 1]], reads=reads, batch=int(batch))
    return out, state


def extract_lesion_candidates(prob, n_lesions, peak_cut=0.40, min_voxels=11, min_peak=0.01, batch=None):
    """extract_lesion_candidates (:48-70) on the device.  prob: float32 device tensor (D, H, W) with an integer n_lesions -> (mask uint8 (D, H, W), kept);
    or (P, D, H, W) with a list of P counts -> (mask (P, D, H, W), [kept per plane]): the planes advance in the same launches.

    Until `kept == n_lesions`: peak = max of the remaining probabilities (ties: the first voxel in C order, np.argmax); stop unless peak >= float32(min_peak);
    the 26-connected component of `work >= float32(peak_cut) * peak` (a float32 product, NumPy 2 scalar rules) that holds the peak voxel is zeroed and,
    if it has at least min_voxels voxels, added to the mask and counted.  Masks, kept and the iteration count equal the reference's exactly.

    prob is not modified (the kernels consume a copy).  A CPU tensor raises RSuperHipError: there is no host fallback.  Non-finite values in prob are
    the caller's error and the result is then unspecified, but the call returns: a plane whose peak is NaN is ended at once (`done`, with the
    iterations it had made until then; the reference would mark the whole volume instead), and +inf is a peak like any other.
    n_lesions <= 0 returns zeros and 0 without a launch.

    Deviation from the reference: parameters outside `0 < peak_cut <= 1`, `min_peak > 0` (both as float32), `min_voxels >= 1` raise ValueError; the
    reference loops forever or labels a component that does not hold the peak there.

    batch: iterations enqueued between two reads of the per-plane state (each iteration is five launches; the ones past a plane's end return at
    once).  Default DEFAULT_BATCH = 4: radiology reports mostly count one to three lesions, so the common case needs a single read, and an unused
    iteration costs a few empty launches, less than the synchronising read it saves.  The result does not depend on it.  `last_state` holds, per plane,
    kept, iterations and the number of reads."""
    if not isinstance(prob, torch.Tensor) or not prob.is_cuda:
        raise _l.RSuperHipError('extract_lesion_candidates: the probabilities must be on the MI355X device (no CPU fallback)')
    batch = DEFAULT_BATCH if batch is None else batch
    single = prob.dim() == 3
    if single:
        if isinstance(n_lesions, (list, tuple)):
            raise ValueError('extract_lesion_candidates: one (D, H, W) volume takes one lesion count')
        counts, stack = [int(n_lesions)], prob.unsqueeze(0)
    else:
        if prob.dim() != 4 or not isinstance(n_lesions, (list, tuple)) or len(n_lesions) != prob.shape[0]:
            raise ValueError('extract_lesion_candidates: (D, H, W) with a count, or (P, D, H, W) with a list of P counts')
        counts, stack = [int(n) for n in n_lesions], prob
    if stack.dtype != torch.float32:
        raise ValueError(f'extract_lesion_candidates: float32 probabilities, got {stack.dtype}')
    _check_params(peak_cut, min_voxels, min_peak, batch)
    if all(n <= 0 for n in counts):
        mask = torch.zeros(stack.shape, device=stack.device, dtype=torch.uint8)
        kept = [0] * len(counts)
        last_state.update(kept=list(kept), iterations=[0] * len(counts), reads=[0] * len(counts), batch=int(batch))
    else:
        mask, state = torch.ops.rsuper.lesion_candidates(stack, counts, float(peak_cut), int(min_voxels), float(min_peak), int(batch))
        kept = [int(v) for v in state[:, 0].cpu()]        # from the call's own result; last_state is a report only
    return (mask[0], kept[0]) if single else (mask, kept)


def lesion_column(class_name):
    """The metadata column that counts the lesions of a class (:111-112): the first '_' field of the name, lower case."""
    return f"number of {class_name.split('_')[0].lower()} lesion instances"


def refine_case(raw, classes, meta_row, extractor=None):
    """process_bdmap's decision (:107-155) on the raw probabilities of one case, e.g. `predict_case(...)['raw']`: raw (C, D, H, W) float32 on the
    device ((C, D, H, W, T) takes [..., 0], :126-127), classes its C names, meta_row the case's metadata row (a mapping column -> value) or None when
    the metadata has no such case.  Returns (included, {class: uint8 (D, H, W) mask}).

    For every class with 'lesion' in its name the report's count is `int(meta_row[lesion_column(class)])`.  A missing row or column, or a count int()
    refuses (NaN, None, text), excludes the case.  A count <= 0 asks for no mask.  Every other class needs as many candidates as the report counts:
    `found < n` for any of them excludes the case.  Masks are returned only for an included case.  All classes with a positive count go through one
    multi-plane extract_lesion_candidates call (the reference stops at the first class that falls short; the decision is the same)."""
    extractor = extract_lesion_candidates if extractor is None else extractor
    lesion = [(i, c) for i, c in enumerate(classes) if 'lesion' in c]
    todo = []
    for i, c in lesion:
        col = lesion_column(c)
        if meta_row is None or col not in meta_row:
            return False, {}
        try:
            n = int(meta_row[col])
        except (TypeError, ValueError):
            return False, {}
        if n > 0:
            todo.append((i, c, n))
    if not todo:
        return True, {}
    if raw.dim() == 5:
        raw = raw[..., 0]
    if raw.dim() != 4 or raw.shape[0] != len(classes):
        raise ValueError(f'refine_case: {tuple(raw.shape)} for {len(classes)} classes')
    stack = raw[[i for i, _, _ in todo]] if len(todo) != len(classes) else raw
    masks, found = extractor(stack.contiguous(), [n for _, _, n in todo])
    if any(f < n for f, (_, _, n) in zip(found, todo)):
        return False, {}
    return True, {c: masks[k] for k, (_, c, _) in enumerate(todo)}


def slice_indices(n, parts, part):
    """The part-th of `parts` contiguous chunks of range(n), the first n % parts chunks one longer (:161-166)."""
    base, rem = divmod(n, parts)
    start = part * base + min(part, rem)
    return slice(start, start + base + (1 if part < rem else 0))


def dump_yaml(path, data):
    """A list of names as a YAML sequence (:22-31); written by hand where PyYAML is missing."""
    from pathlib import Path
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    items = list(data)
    try:
        import yaml
    except ModuleNotFoundError:
        yaml = None
    with path.open('w') as f:
        if yaml is not None:
            yaml.safe_dump(items, f, default_flow_style=False, sort_keys=False)
        else:
            f.writelines(f'- {x}\n' for x in items)


def load_yaml(path):
    """The set of names of such a file, empty when it does not exist (:34-42)."""
    from pathlib import Path
    path = Path(path)
    if not path.exists():
        return set()
    text = path.read_text()
    try:
        import yaml
    except ModuleNotFoundError:
        names = set()
        for line in text.splitlines():                    # the hand-written form of dump_yaml: one "- name" per line
            if line.startswith('-'):
                names.add(line[1:].strip())
        return names
    return set(yaml.safe_load(text) or [])


_library.install_pseudo_label_ops(_lesion_candidates_impl)
