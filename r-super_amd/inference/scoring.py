"""One predicted case measured while it is still on the device: the CSV row of test_with_reports._process_single_file (rsuper_train/
test_with_reports.py:117-181) from the binary lesion planes and the nine rows of eval_AUC._process_single_file (eval_AUC.py:135-206) from the
lesion probability planes.  All lesion planes of a case go through one launch per flow and one device-to-host read per flow."""
import torch

from .detection import THRESHOLDS, _binary_counts, detection

# file-name suffix of a lesion class -> the word of its column ("<organ> <word> volume predicted"), in the reference's order of checks
LESION_SUFFIXES = (('_lesion', 'tumor'), ('_pdac', 'pdac'), ('_pnet', 'pnet'), ('_cyst', 'cyst'))


def normalize_id(name):
    """_normalize_id (:110-115): the BDMAP_ID of a case folder or file name."""
    return name.replace('_0000.', '.').replace('.nii.gz', '')


def column_name(class_name):
    """The volume column of a lesion class, or None for a class the reference does not measure: 'liver_lesion' -> 'liver tumor volume predicted',
    'pancreas_pdac' -> 'pancreas pdac volume predicted'."""
    for suffix, word in LESION_SUFFIXES:
        if class_name.endswith(suffix):
            return f'{class_name[:-len(suffix)]} {word} volume predicted'
    return None


def lesion_classes(classes):
    return [c for c in classes if column_name(c) is not None]


def _stack(planes, names):
    ps = [planes[n] if torch.is_tensor(planes[n]) else torch.as_tensor(planes[n]) for n in names]
    ps = [p.view(torch.uint8) if p.dtype == torch.bool else p for p in ps]
    return torch.stack(ps) if len(ps) > 1 else ps[0].unsqueeze(0)


def score_case(pred_dict, raw_dict, classes, spacing, th=0.5, thresholds=THRESHOLDS, erode=True, case_id=None):
    """pred_dict {class: (D, H, W) uint8 / bool / float32 mask}, raw_dict {class: (D, H, W) float32 probabilities} or None; `classes` the names to
    measure (those without a lesion suffix are skipped); spacing per array axis.  Returns (row, rows_by_threshold): row = {'BDMAP_ID'?, column:
    int volume} from detection_binary at `th`; rows_by_threshold = {t: {column: int volume, '... maximum probability': float}} from `detection`,
    or None without probabilities.  BDMAP_ID (normalised) is set when case_id is given."""
    base = {} if case_id is None else {'BDMAP_ID': normalize_id(case_id)}
    row = dict(base)
    names = [c for c in lesion_classes(classes) if c in pred_dict]
    if names:
        counts, _ = _binary_counts(_stack(pred_dict, names), spacing, th, erode)
        for n, v in zip(names, counts.cpu().tolist()):
            row[column_name(n)] = int(v)
    if raw_dict is None:
        return row, None
    rows = {t: dict(base) for t in thresholds}
    names = [c for c in lesion_classes(classes) if c in raw_dict]
    if names:
        res = detection(_stack(raw_dict, names).to(torch.float32), spacing, thresholds, erode)
        for n, (vols, mx) in zip(names, res):
            col = column_name(n)
            for t in thresholds:
                rows[t][col] = vols[t]
                rows[t][col.replace('volume predicted', 'maximum probability')] = mx
    return row, rows
