"""The host decisions of the report-annotated branch of `AbdomenAtlasDataset` (rsuper_train/training/dataset/dim3/dataset_abdomenatlas_UFO.py):
which organ or sub-segment a report lets a crop be taken on (`get_tumor_segment_labels` :647-754), which label classes that segment is
(`get_random_tumor_seg_mask` :756-791), the draws and retries of `crop()` (:855-934), and `assign_labels` (:1154-1298) and
`get_chosen_segment_mask` (:808-833) as bit tables: every output plane of the three volumes they build is an OR of input planes, all ones, or
zero, so a table of 64-bit class sets per output class says everything, and one rsuper_label_remap launch applies it to the packed crop.

Needs no device.  Report rows come as `augmented.estimate_tumor_volume` takes them: a DataFrame, or a list of mappings, with 'Standardized Organ',
'Standardized Location' and 'Tumor Size (mm)'; None = the case has no tumour rows.  The reference's outcomes are reproduced as they are, including
its quirks (a test of `'segment' in item` where item is a list, kidney sides that never match 'kidney_lesion', an organ name iterated by character).
`no_pancreas_subseg` is not covered.
"""
import random

import numpy as np

LIVER_SEGMENTS = ['segment %d' % i for i in range(1, 9)]
PANCREAS_SEGMENTS = ['head', 'body', 'tail']
RANDOM = 'random'


def _isna(v):
    """pd.isna for a scalar cell: None, a float NaN, or pandas' NA / NaT."""
    if v is None:
        return True
    if isinstance(v, float):
        return v != v
    if isinstance(v, (str, list, tuple, dict)):
        return False
    try:
        return bool(v != v)
    except (TypeError, ValueError):
        return type(v).__name__ in ('NAType', 'NaTType')


def _columns(rows):
    """-> (locations, sizes, organs) as lists, or None when there are no rows."""
    if rows is None:
        return None
    if hasattr(rows, 'iterrows'):
        return rows['Standardized Location'].tolist(), rows['Tumor Size (mm)'].tolist(), rows['Standardized Organ'].tolist()
    rows = list(rows)
    return ([r['Standardized Location'] for r in rows], [r['Tumor Size (mm)'] for r in rows], [r['Standardized Organ'] for r in rows])


def clean_subseg_list(tumor_segments):
    """clean_subseg_list (:633-645): drop NaN and 'u', split ' / ' pairs, unique sub-lists in order; and the flat list (a set in the reference)."""
    tmp = []
    for segment in tumor_segments:
        if _isna(segment) or segment == 'u':
            continue
        sublist = segment.split(' / ')
        if sublist not in tmp:
            tmp.append(sublist)
    return tmp, sorted(set(item for sublist in tmp for item in sublist))


def get_tumor_segment_labels(rows, no_pancreas_subseg=False):
    """get_tumor_segment_labels (:647-754) -> the reference's dict.  The lists the reference builds through list(set(...)) come in the hash order of
    its process, which differs from run to run; they are sorted here, so that random.choice over them is a function of the seed alone."""
    if no_pancreas_subseg:
        raise NotImplementedError('no_pancreas_subseg is not covered')
    cols = _columns(rows)
    keys = ('tumor_segments', 'tumor_segments_flat', 'tumor_organs', 'organs_with_unk_tumor_segment', 'organs_with_unk_tumor_size',
            'organs_with_only_known_sizes_n_segments', 'subseg_with_only_known_sizes', 'subseg_with_unk_tumor_size', 'subsegs_in_organs_with_unk')
    if cols is None:
        return {k: [] for k in keys}
    tumor_segments, tumor_sizes, tumor_organs = cols
    organs_with_unk_tumor_segment, organs_with_unk_tumor_size, subseg_with_unk_tumor_size = [], [], []
    for i in range(len(tumor_organs)):
        if _isna(tumor_sizes[i]) or tumor_sizes[i] == 'u' or tumor_sizes[i] == 'multiple':
            organs_with_unk_tumor_size.append(tumor_organs[i])
            subseg_with_unk_tumor_size.append(tumor_segments[i])
        if _isna(tumor_segments[i]) or tumor_segments[i] == 'u':
            organs_with_unk_tumor_segment.append(tumor_organs[i])
    subsegs_in_organs_with_unk = []
    for i in range(len(tumor_organs)):
        if tumor_organs[i] in organs_with_unk_tumor_segment or tumor_organs[i] in organs_with_unk_tumor_size:
            subsegs_in_organs_with_unk.append(tumor_segments[i])

    tumor_segments, tumor_segments_flat = clean_subseg_list(tumor_segments)
    subseg_with_unk_tumor_size, subseg_with_unk_tumor_size_flat = clean_subseg_list(subseg_with_unk_tumor_size)
    subsegs_in_organs_with_unk, subsegs_in_organs_with_unk_flat = clean_subseg_list(subsegs_in_organs_with_unk)

    def known(organs):
        return sorted(set(organ for organ in organs if not _isna(organ) and organ != 'u'))

    tumor_organs = known(tumor_organs)
    organs_with_unk_tumor_segment = known(organs_with_unk_tumor_segment)
    organs_with_unk_tumor_size = known(organs_with_unk_tumor_size)
    subseg_with_only_known_sizes = sorted(set(tumor_segments_flat) - set(subseg_with_unk_tumor_size_flat) - set(subsegs_in_organs_with_unk_flat))
    organs_with_only_known_sizes_n_segments = sorted(set(tumor_organs) - set(organs_with_unk_tumor_segment) - set(organs_with_unk_tumor_size))

    tmp = []
    for segment in subseg_with_only_known_sizes:                 # sub-segments that share a tumour (' / ' pairs) go together
        items = [item for item in tumor_segments if segment in item]
        items = sorted(set(item for sublist in items for item in sublist))
        if any(item in subseg_with_unk_tumor_size_flat for item in items) or any(item in subsegs_in_organs_with_unk_flat for item in items):
            continue
        tmp.append(items)
    return dict(zip(keys, (tumor_segments, tumor_segments_flat, tumor_organs, organs_with_unk_tumor_segment, organs_with_unk_tumor_size,
                           organs_with_only_known_sizes_n_segments, tmp, subseg_with_unk_tumor_size, subsegs_in_organs_with_unk)))


def _label_name(seg):
    return (seg.replace('segment ', 'liver_segment_').replace('head', 'pancreas_head').replace('body', 'pancreas_body')
            .replace('tail', 'pancreas_tail').replace('left', 'kidney_left').replace('right', 'kidney_right'))


def segment_class_names(tumor_segment):
    """The label names of a segment, an organ or a list of them (:760-773): 'pancreas' and 'liver' alone expand to their sub-segments."""
    if not isinstance(tumor_segment, list):
        tumor_segment = [tumor_segment]
    if len(tumor_segment) == 1 and tumor_segment[0] == 'pancreas':
        tumor_segment = PANCREAS_SEGMENTS
    if len(tumor_segment) == 1 and tumor_segment[0] == 'liver':
        tumor_segment = LIVER_SEGMENTS
    return [_label_name(seg) for seg in tumor_segment]


def segment_class_set(tumor_segment, classes, classes_ufo=None):
    """get_random_tumor_seg_mask (:756-806) as a 64-bit set over `classes`: the union of these planes is its mask.  A name that is not in
    classes_ufo (default: classes) raises ValueError as the reference does; no plane at all is torch.stack's RuntimeError."""
    names = segment_class_names(tumor_segment)
    known = list(classes if classes_ufo is None else classes_ufo)
    for name in names:
        if name not in known:
            raise ValueError('Label %s not in classes_UFO' % name)
    cset = 0
    for i, clss in enumerate(classes):
        if clss in names:
            cset |= 1 << i
    if cset == 0:
        raise RuntimeError('stack expects a non-empty TensorList')
    return cset


def segment_options(segments):
    """The list crop() draws from (:857-866), or None: no tumour the report sizes -> random_crop_on_tumor."""
    if len(segments['subseg_with_only_known_sizes']) > 0:
        return segments['subseg_with_only_known_sizes']
    if len(segments['organs_with_only_known_sizes_n_segments']) > 0:
        return segments['organs_with_only_known_sizes_n_segments']
    return None


def _report_crop_steps(options):
    """crop()'s report branch (:857-934) as a coroutine: it yields ('mask', segment) and expects the segment mask's voxel count, yields
    ('crop', segment) and expects crop_foreground_3d's outcome (True for a crop, else its string), and returns (how it ends, chosen segment)."""
    if options is None:
        return 'random_crop_on_tumor', RANDOM
    if np.random.random() < 0.1:
        return 'random_crop', RANDOM
    tumor_segment = random.choice(options)
    count = yield 'mask', tumor_segment
    if count == 0:
        options = [seg for seg in options if seg not in [tumor_segment]]
        if len(options) == 0:
            return 'random_crop_on_tumor', RANDOM
        tumor_segment = random.choice(options)
        count = yield 'mask', tumor_segment
        if count == 0:
            return 'random_crop_on_tumor', RANDOM
    out = yield 'crop', tumor_segment
    if out is True:
        return 'done', tumor_segment
    if len(options) == 1:
        return 'random_crop_on_tumor', RANDOM
    options = [seg for seg in options if seg not in [tumor_segment]]
    if len(options) == 0:
        return 'random_crop_on_tumor', RANDOM
    tumor_segment = random.choice(options)
    out = yield 'crop', tumor_segment                           # an empty mask is crop_foreground_3d's 'zero mask' here
    if out is True:
        return 'done', tumor_segment
    return 'random_crop_on_tumor', RANDOM


class ReportCropPlan:
    """The state machine of one report crop.  `action` is 'mask' (feed(count of the union of `tumor_segment`'s classes)), 'crop'
    (feed(True) when crop_foreground_3d cut a crop, feed(its string) otherwise), or final: 'done' (the crop of the last 'crop' stands),
    'random_crop' (the 0.1 gate) or 'random_crop_on_tumor' (tumor_case=False, ufo=True).  `tumor_segment` is then what crop() returns as the
    selected tumour.  np.random.random and random.choice are consumed in the reference's order; crop_foreground_3d's random.randint draws fall
    between them at the caller's 'crop' steps."""

    FINAL = ('done', 'random_crop', 'random_crop_on_tumor')

    def __init__(self, segments):
        self.asked = []
        self._steps = _report_crop_steps(segment_options(segments))
        self._take(lambda: next(self._steps))

    def _take(self, step):
        try:
            self.action, self.tumor_segment = step()
        except StopIteration as end:
            self.action, self.tumor_segment = end.value
        self.asked.append(self.action)

    def feed(self, answer):
        if self.action in self.FINAL:
            raise RuntimeError('the plan has ended with %r' % self.action)
        self._take(lambda: self._steps.send(answer))
        return self


def plan_report_crop(segments):
    """-> ReportCropPlan for the dict of get_tumor_segment_labels."""
    return ReportCropPlan(segments)


def _bits(cset):
    return [c for c in range(64) if cset >> c & 1]


def assign_labels_tables(classes, classes_ufo, rows, present):
    """assign_labels (:1154-1298) as tables over the classes_ufo planes of the crop.  present: the per-class voxel totals of the crop (they replace
    tensor_lab[seg_idx].max() > 0).  -> (masks_label [C], ones_label, masks_unk [C], ones_unk, unk_channels): label class j = OR of the input
    classes of masks_label[j]; unknown-map class j = OR of masks_unk[j], or all ones where bit j of ones_unk is set.  KeyError for a segment or
    an organ part that classes_ufo lacks and AssertionError when tumour segments are in the crop but the unknown map is empty, as there."""
    classes, classes_ufo = list(classes), list(classes_ufo)
    ufo_idx = {clss: i for i, clss in enumerate(classes_ufo)}
    all_data = get_tumor_segment_labels(rows)
    tumor_segments = all_data['tumor_segments']
    for tumor_organ in all_data['tumor_organs']:
        if isinstance(tumor_organ, str) and tumor_organ == 'liver':
            if not any('segment' in item for item in tumor_segments):
                if 'liver' not in tumor_segments:
                    tumor_segments.append('liver')
        elif isinstance(tumor_organ, str) and tumor_organ == 'pancreas':
            if not any('head' in item for item in tumor_segments) and not any('body' in item for item in tumor_segments) \
                    and not any('tail' in item for item in tumor_segments):
                if 'pancreas' not in tumor_segments:
                    tumor_segments.append('pancreas')
        elif isinstance(tumor_organ, str) and tumor_organ == 'kidney':
            if not any('left' in item for item in tumor_segments) and not any('right' in item for item in tumor_segments):
                if 'kidney' not in tumor_segments:
                    tumor_segments.append('kidney')
    tmp = []
    for item in tumor_segments:
        if isinstance(item, list):
            tmp.extend(item)
        elif item == 'pancreas':
            tmp.extend(PANCREAS_SEGMENTS)
        elif item == 'liver':
            tmp.extend(LIVER_SEGMENTS)
        elif item == 'kidney':
            tmp.extend(['left', 'right'])
        else:
            tmp.append(item)
    tumor_segments = sorted(set(_label_name(seg) for seg in set(tmp)))

    unk_segments = {'liver': 0, 'pancreas': 0, 'kidney': 0}      # per organ: the input classes whose union is the "tumour somewhere in here" mask
    unk_lesions = set()
    for seg in tumor_segments:
        seg_idx = ufo_idx[seg]
        if present[seg_idx] > 0:
            if 'liver' in seg:
                unk_segments['liver'] |= 1 << seg_idx
            elif 'pancreas' in seg:
                unk_segments['pancreas'] |= 1 << seg_idx
            elif 'kidney' in seg:
                unk_segments['kidney'] |= 1 << seg_idx
            else:
                raise ValueError('Unrecognized segment:', seg)
            organ = seg[:seg.rfind('_segment')] if '_segment' in seg else seg
            unk_lesions.add(organ.replace('_head', '').replace('_body', '').replace('_tail', '').replace('pancreas', 'pancreatic'))
    unk_lesions = sorted(unk_lesions)

    masks_label, masks_unk, ones_unk, unk_channels = [0] * len(classes), [0] * len(classes), 0, {}
    for j, clss in enumerate(classes):
        if clss in ufo_idx:
            masks_label[j] = 1 << ufo_idx[clss]
        elif 'lesion' not in clss.lower():
            if clss == 'liver':
                for i in range(1, 9):
                    masks_label[j] |= 1 << ufo_idx['liver_segment_%i' % i]
            elif clss == 'pancreas':
                for i in PANCREAS_SEGMENTS:
                    masks_label[j] |= 1 << ufo_idx['pancreas_%s' % i]
            else:
                unk_channels[clss] = j
                ones_unk |= 1 << j
        else:
            for organ in unk_lesions:
                if organ in clss:
                    unk_channels[clss] = j
                    if 'liver' in clss:
                        masks_unk[j] = unk_segments['liver']
                    elif 'pancreatic' in clss:
                        masks_unk[j] = unk_segments['pancreas']
                    elif 'kidney' in clss:
                        masks_unk[j] = unk_segments['kidney']
                    else:
                        raise ValueError('Organ not recognized:', clss)
                    break
    if len(unk_lesions) > 0:
        assert ones_unk or any(present[c] > 0 for m in masks_unk for c in _bits(m)), \
            'unk_channels_list should have some non-zero voxels if there are tumors in the crop, we have tumors in %s' % (unk_lesions,)
    return masks_label, 0, masks_unk, ones_unk, unk_channels


def chosen_segment_table(classes, tumor_segment, classes_ufo=None):
    """get_chosen_segment_mask (:808-833) over the planes of the assigned label (`classes`): -> (segment set, masks [C]) with masks[j] = the segment
    set for the lesion channels the segment belongs to and 0 elsewhere; 'random' -> (0, all zero).  A segment given as a plain string is iterated
    by character there, selects no channel and trips the assertion at :832: AssertionError here as well."""
    classes = list(classes)
    if tumor_segment == RANDOM:
        return 0, [0] * len(classes)
    cset = segment_class_set(tumor_segment, classes, classes_ufo)
    masks = []
    for c in classes:
        if (any('segment' in item for item in tumor_segment) or any('liver' in item for item in tumor_segment)) and 'liver_lesion' in c:
            masks.append(cset)
        elif (any('head' in item for item in tumor_segment) or any('body' in item for item in tumor_segment)
              or any('tail' in item for item in tumor_segment) or any('pancreas' in item for item in tumor_segment)) and 'pancreatic_lesion' in c:
            masks.append(cset)
        elif (any('left' in item for item in tumor_segment) or any('right' in item for item in tumor_segment)
              or any('kidney' in item for item in tumor_segment)) and 'kidney_lesion' in c:
            masks.append(cset)
        else:
            masks.append(0)
    assert any(masks), 'chosen segment mask is empty, crop is in %s' % (tumor_segment,)
    return cset, masks
