"""python -m rsuper_amd.predict_abdomenatlas: the npz path of rsuper_train/predict_abdomenatlas.py (:962-1226) on the device -- load the checkpoint(s),
then per case predict_case -> postprocess_npz -> write, with the reference's flag names.  The next case is read by one background thread while the
device works on the current one.

Inputs are `<id>.npz` (arr_0) or the `<id>.npy` files tools/pack_dataset.py writes.  A NIfTI input is refused unless --nifti is given; with it
`<id>.nii.gz` and `<id>/ct.nii.gz` are read by inference/nifti.py in the reader thread (no SimpleITK, no nibabel), reoriented and resampled to 1 mm
on the device (inference.predict_nifti_case), predicted, and saved as predictions/<class>.nii.gz on the scan's own grid, in
its own voxel order, with its affine (inference.save_nifti_masks); --score takes the spacing from the header unless --spacing_csv names the case;
the probabilities keep going out as .npz; --packed and --device_compress do not apply to such a case.
Outputs under `<save_path>/<dataset>/<folder of the first checkpoint>/<case>/`:

    predictions/<class>.npz          uint8 masks (default)
    predictions/<class>.nii.gz       uint8 masks of a NIfTI case (--nifti), compressed on the device
    predictions.npz                  --packed: arr_0 = np.packbits(masks, axis=0) of the saved classes (packed on the device; the training-label
                                     layout) and `classes`, their names
    predictions_raw/<class>.npz      float32 probabilities (--save_probabilities: all classes, --save_probabilities_lesions: lesion classes)
    *.nii.gz copies                  only when nibabel imports

--device_compress deflates the uint8 masks (per class or --packed) on the device and reads back the compressed bytes only (inference/npz_writer.py):
the same files, keys and arrays under np.load, other compressed bytes.  Without it every byte written is np.savez_compressed's.  The float32
probabilities stay on the host path.

--lesion_table measures the lesions of every saved lesion class while the masks are still on the device (inference.lesion_table: count, voxels, extent,
diameters; --lesion_min_voxels drops smaller components) and appends one row per lesion to <save_path>/lesions.csv, with the organ sub-segment it
sits in when planes named '<organ>_...' are among the classes.  Without the flag not one byte of output changes.

--score measures every case while it is still on the device (inference.score_case) and appends the rows to tumor_detection_results.csv and, with
probabilities, tumor_detection_results_th0.1.csv ... in the save path; with --not_save_binary nothing has to be written and read back.

Differences from the reference, on purpose: the ids are sorted, split into parts first (split_into_parts, every case in exactly one part -- the
reference's `len // parts` window drops the tail) and filtered second, and not shuffled."""
import argparse
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .test_with_reports import append_rows, csv_paths, read_ids, read_spacing_csv, split_into_parts

LESION_WORDS = ('lesion', 'pdac', 'pnet', 'cyst')


def get_parser(argv=None, config_root=None):
    """The reference's flag names (those the npz path reads) plus --config, --packed, --score, --spacing_csv and --th; the YAML is found the way
    train_ddp.get_parser finds it (<package>/config/<dataset>/<model>_<dimension>.yaml) and fills what the command line does not define."""
    import yaml
    from .train_ddp import merge_config
    p = argparse.ArgumentParser(prog='rsuper_amd.predict_abdomenatlas', description='Predict a list of cases on the MI355X and save / score them')
    p.add_argument('--dataset', type=str, default='abdomenatlas')
    p.add_argument('--model', type=str, default='unet')
    p.add_argument('--dimension', type=str, default='3d')
    p.add_argument('--config', type=str, default=None, help='YAML file to use instead of config/<dataset>/<model>_<dimension>.yaml')
    p.add_argument('--load', type=lambda s: [v for v in s.split(',') if v], required=True, help='checkpoint, or A,B,... for an ensemble (summed)')
    p.add_argument('--EMA', action='store_true', help='load ema_model_state_dict')
    p.add_argument('--img_path', type=str, required=True)
    p.add_argument('--save_path', type=str, default='./result/')
    p.add_argument('--ids', type=str, default=None, help='CSV with a BDMAP_ID (or "BDMAP ID") column; default: every case of --img_path')
    p.add_argument('--class_list', type=str, required=True, help='YAML list of class names (sorted on load)')
    p.add_argument('--old_classes', type=str, default=None)
    p.add_argument('--update_output_layer', action='store_true')
    p.add_argument('--organ_mask_on_lesion', action='store_true')
    p.add_argument('--connected_components', action='store_true')
    p.add_argument('--predict_pancreas_only', action='store_true', help='infer only windows that touch the pancreas of <id>_gt (packed or unpacked)')
    p.add_argument('--save_probabilities', action='store_true')
    p.add_argument('--save_probabilities_lesions', action='store_true')
    p.add_argument('--not_save_binary', action='store_true')
    p.add_argument('--save_pancreas_lesion_only', action='store_true')
    p.add_argument('--overwrite', action='store_true')
    p.add_argument('--parts', type=int, default=1)
    p.add_argument('--current_part', type=int, default=0)
    p.add_argument('--gpu', type=str, default='0')
    p.add_argument('--packed', action='store_true', help='one bit-packed predictions.npz per case instead of one file per class')
    p.add_argument('--device_compress', action='store_true', help='deflate the saved masks on the device; the files load to the same arrays')
    p.add_argument('--score', action='store_true', help='measure each case on the device and append the detection CSV rows')
    p.add_argument('--spacing_csv', type=str, default=None, help='CSV with BDMAP_ID and one spacing column per array axis (default: 1 mm)')
    p.add_argument('--nifti', action='store_true', help='accept <id>.nii.gz and <id>/ct.nii.gz cases: read, reorient and resample them on the device and '
                   'save the masks as .nii.gz on the scan\'s own grid (ignored for .npz / .npy cases)')
    p.add_argument('--th', type=float, default=0.5, help='threshold that binarises a mask for --score')
    p.add_argument('--lesion_table', action='store_true', help='measure the predicted lesions of every saved lesion class on the device and append '
                   'them to <save_path>/lesions.csv (inference/lesions.py)')
    p.add_argument('--lesion_min_voxels', type=int, default=1, help='components below this many voxels are no lesions for --lesion_table')
    args = p.parse_args(argv)
    path = args.config
    if path is None:
        root = config_root or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'config')
        path = os.path.join(root, args.dataset, f'{args.model}_{args.dimension}.yaml')
    if not os.path.exists(path):
        raise ValueError("The specified configuration doesn't exist: %s" % path)
    with open(path, 'r') as f:
        merge_config(args, yaml.load(f, Loader=yaml.SafeLoader))
    args.save_path = os.path.join(args.save_path, args.dataset, os.path.basename(os.path.dirname(args.load[0])))
    args.sliding_window = True
    args.window_size = args.training_size
    return args


def case_id_of(img_name):
    for ext in ('/ct.nii.gz', '.nii.gz', '.npz', '.npy'):
        img_name = img_name.replace(ext, '')
    return img_name


def refuse_nifti(name):
    if 'nii.gz' in name:
        raise ValueError(f'{name}: NIfTI input is not read here (no SimpleITK / nibabel dependency); convert the case with the dataset tools or wire the '
                         'device functions into the reference script as INTEGRATION section 3b describes')


def list_ids(args):
    """The case files of --img_path, sorted: every non-label file, or the ids of the --ids CSV with the extension its first id is found under."""
    if args.ids is None:
        ids = [i for i in os.listdir(args.img_path) if 'gt.' not in i]
    else:
        import csv
        with open(args.ids, newline='') as f:
            rd = csv.DictReader(f)
            col = 'BDMAP_ID' if 'BDMAP_ID' in rd.fieldnames else 'BDMAP ID'
            names = [r[col] for r in rd]
        for ext in ('.npz', '.npy', '/ct.nii.gz', '.nii.gz'):
            if names and os.path.exists(os.path.join(args.img_path, names[0] + ext)):
                ids = [n + ext for n in names]
                break
        else:
            raise ValueError('Path not found')
    nifti = getattr(args, 'nifti', False)
    if nifti:           # a case folder that holds ct.nii.gz is the case <folder>/ct.nii.gz
        ids = [i + '/ct.nii.gz' if os.path.isfile(os.path.join(args.img_path, i, 'ct.nii.gz')) else i for i in ids]
    else:
        for i in ids:
            refuse_nifti(i)
    kept = sorted(i for i in ids if os.path.exists(os.path.join(args.img_path, i)) and i.endswith(('.npz', '.npy') + (('.nii.gz',) if nifti else ())))
    print(f'After removing missing cases, {len(kept)} ids remain. Number of removed files: {len(ids) - len(kept)}')
    return kept


def saved_classes(class_list, args):
    return [c for c in class_list if 'pancrea' in c] if args.save_pancreas_lesion_only else list(class_list)


def already_predicted(case_dir, class_list, ext='.npz'):
    """Every class of class_list is saved: predictions/<class>.npz (.nii.gz for a NIfTI case) for all of them, or a packed predictions.npz that names
    them all."""
    pred_dir = os.path.join(case_dir, 'predictions')
    if os.path.isdir(pred_dir):
        stems = {f[:-len(ext)] for f in os.listdir(pred_dir) if f.endswith(ext)}
        if set(class_list).issubset(stems):
            return True
    packed = os.path.join(case_dir, 'predictions.npz')
    if os.path.isfile(packed):
        with np.load(packed) as z:
            return set(class_list).issubset(str(c) for c in z['classes'])
    return False


def filter_already_predicted(ids, save_path, class_list, overwrite, scored_ids=()):
    """filter_already_predicted (:928-960) for the .npz file names: drop the cases whose classes are all saved (or, for a run that saves no masks,
    whose row is already in the CSV)."""
    if overwrite:
        return ids
    kept = [i for i in ids if not (already_predicted(os.path.join(save_path, case_id_of(i)), class_list, '.nii.gz' if i.endswith('.nii.gz') else '.npz')
                                   or case_id_of(i) in scored_ids)]
    print(f'Ids after filtering: {len(kept)} / {len(ids)}')
    return kept


def init_model(args, classes, old_classes=None):
    """init_model (:744-783): one network per checkpoint of --load, its (EMA) state dict loaded non-strictly, on the device in eval mode; with
    --update_output_layer built for the old classes and its heads then rebuilt for `classes`."""
    from .model.utils import get_model
    if args.update_output_layer and old_classes is None:
        raise ValueError('--update_output_layer needs --old_classes')
    c = old_classes if args.update_output_layer else classes
    models = []
    for path in args.load:
        args.classes = len(c)
        model = get_model(args, classes=c)
        sd = torch.load(path, map_location='cpu', weights_only=False)['ema_model_state_dict' if args.EMA else 'model_state_dict']
        if isinstance(sd, torch.nn.Module):
            sd = sd.state_dict()
        model.load_state_dict(sd, strict=False)
        if args.update_output_layer:
            if not hasattr(model, 'aux_loss'):
                raise NotImplementedError('--update_output_layer rewires MedFormer heads (model/dim3/medformer.py)')
            from .model.dim3.medformer import update_output_layer_onk
            model = update_output_layer_onk(model, original_classes=old_classes, new_classes=classes)
        models.append(model.to('cuda').eval())
        print(f'Model loaded from {path}')
    args.classes = len(classes)
    return models


def _load_array(path):
    if path.endswith('.npy'):
        return np.load(path)
    with np.load(path) as z:
        return z['arr_0']


def load_case(args, img_name, class_list):
    """(HU array, pancreas mask or None) of a case; the label of --predict_pancreas_only is <id>_gt.npz / .npy, bit-packed or one byte per class.
    With --nifti a NIfTI case comes back as the inference.nifti.NiftiVolume of the file (read and inflated here, in the reader thread)."""
    if getattr(args, 'nifti', False) and 'nii.gz' in img_name:
        if args.predict_pancreas_only:
            raise ValueError('You cannot predict only pancreas with nii.gz files, please use npz files.')
        from .inference.nifti import read_nifti
        return read_nifti(os.path.join(args.img_path, img_name)), None
    refuse_nifti(img_name)
    path = os.path.join(args.img_path, img_name)
    hu = _load_array(path)
    pancreas = None
    if args.predict_pancreas_only:
        ext = path[-4:]
        labels = _load_array(path[:-4] + '_gt' + ext)
        n = len(class_list)
        if labels.shape[0] != n:
            labels = np.unpackbits(labels, axis=0)
            assert n <= labels.shape[0] < n + 10, f'{img_name}: label planes {labels.shape[0]} do not fit {n} classes'
        pancreas = np.ascontiguousarray(labels[class_list.index('pancreas')]).astype(np.float32)
    return hu, pancreas


def predict_one(models, hu, pancreas, args, class_list):
    """({class: (D, H, W) uint8 device tensor}, raw (C, D, H, W) float32) of one case."""
    from .inference import postprocess_npz, predict_case, prediction, preprocess_array
    if pancreas is None:
        return predict_case(models, hu, args, class_list)
    img, _ = preprocess_array(hu, args)
    if tuple(img.shape) != tuple(pancreas.shape):
        raise NotImplementedError(f'--predict_pancreas_only: the case {tuple(pancreas.shape)} is smaller than the training size and would be padded '
                                  f'to {tuple(img.shape)}; pad the case and its label first')
    label, raw = prediction(models, img, args, tgt_organ=torch.from_numpy(pancreas).to(img.device), to_cpu=False)
    return postprocess_npz(label, class_list, args), raw


def _save_nifti_copy(arr, path):
    try:
        import nibabel as nib
    except ImportError:
        return
    nib.save(nib.Nifti1Image(arr, np.eye(4)), path)


def write_binary(case_dir, pred_dict, names, packed, device_compress=False):
    """One device-to-host read of the saved planes; --packed packs them on the device first (8x fewer bytes over the bus and on disk);
    --device_compress deflates them on the device too, and the read is of the compressed bytes."""
    stack = torch.stack([pred_dict[n].to(torch.uint8) for n in names])
    if packed:
        from .training.dataset.packed import pack_bits_device
        bits = pack_bits_device(stack).packed[0]
        if device_compress:
            from .inference.npz_writer import savez_compressed_device
            savez_compressed_device(os.path.join(case_dir, 'predictions.npz'), table='mask', arr_0=bits, classes=np.array(names))
            return
        np.savez_compressed(os.path.join(case_dir, 'predictions.npz'), arr_0=bits.cpu().numpy(), classes=np.array(names))
        return
    if device_compress:
        from .inference.npz_writer import save_planes_npz
        os.makedirs(os.path.join(case_dir, 'predictions'), exist_ok=True)
        save_planes_npz([os.path.join(case_dir, 'predictions', n + '.npz') for n in names], stack, table='mask')
        try:
            import nibabel  # noqa: F401
        except ImportError:
            return
        host = stack.cpu().numpy()
        for k, n in enumerate(names):
            _save_nifti_copy(host[k], os.path.join(case_dir, 'predictions', n + '.nii.gz'))
        return
    host = stack.cpu().numpy()
    os.makedirs(os.path.join(case_dir, 'predictions'), exist_ok=True)
    for k, n in enumerate(names):
        np.savez_compressed(os.path.join(case_dir, 'predictions', n + '.npz'), host[k])
        _save_nifti_copy(host[k], os.path.join(case_dir, 'predictions', n + '.nii.gz'))


def write_raw(case_dir, raw_dict, names):
    if not names:
        return
    host = torch.stack([raw_dict[n] for n in names]).cpu().numpy()
    os.makedirs(os.path.join(case_dir, 'predictions_raw'), exist_ok=True)
    for k, n in enumerate(names):
        np.savez_compressed(os.path.join(case_dir, 'predictions_raw', n + '.npz'), host[k])
        _save_nifti_copy(host[k], os.path.join(case_dir, 'predictions_raw', n + '.nii.gz'))


def measure_lesions(pred_dict, class_list, names, spacing, case_id, min_voxels=1):
    """The lesions.csv rows of one case: one inference.lesion_table call over the lesion planes of `names` (mask > 0), and per lesion class with
    sub-segment planes in pred_dict one locate_lesions call."""
    from .inference.lesions import lesion_csv_rows, lesion_table, locate_lesions, segment_classes
    lesions = [n for n in names if 'lesion' in n]
    if not lesions:
        return []
    table = lesion_table(torch.stack([(pred_dict[n] > 0).to(torch.uint8) for n in lesions]), spacing=spacing, min_voxels=min_voxels, return_labels=True)
    rows = []
    for p, n in enumerate(lesions):
        segs = [c for c in segment_classes(n, class_list) if c in pred_dict]
        loc = None
        if segs and table.count(p):
            loc = locate_lesions(table.plane(p), torch.stack([pred_dict[c] > 0 for c in segs]), segs)
        rows += lesion_csv_rows(table, case_id, n, loc, plane=p)
    return rows


def main(argv=None, config_root=None):
    """Returns the list of predicted case ids and the seconds per stage {'read', 'predict', 'postprocess', 'measure', 'write'}."""
    import yaml
    from .hip import lib
    from .inference import postprocess_npz, predict_nifti_case, save_nifti_masks
    from .inference.nifti import NiftiVolume
    from .inference.scoring import score_case
    from .train_ddp import load_old_classes
    args = get_parser(argv, config_root)
    if argv is None and not torch.cuda.is_initialized():       # the command line picks its device; an in-process caller keeps its own
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    os.makedirs(args.save_path, exist_ok=True)
    print('Save path: %s' % args.save_path)
    with open(args.class_list, 'r') as f:
        class_list = sorted(yaml.load(f, Loader=yaml.SafeLoader))
    args.class_list, args.classes = class_list, len(class_list)
    old_classes = load_old_classes(args)
    ids = list_ids(args)
    if args.parts > 1:
        ids = split_into_parts(ids, args.parts, args.current_part)
    if args.score and args.overwrite and (args.parts == 1 or args.current_part == 0):       # start the CSVs afresh, as the scorers do
        for path in csv_paths(args.save_path, 'binary') + csv_paths(args.save_path, 'auc'):
            if os.path.exists(path):
                os.remove(path)
    scored = ()
    if args.score and args.not_save_binary and not args.overwrite and os.path.exists(csv_paths(args.save_path, 'binary')[0]):
        scored = set(read_ids(csv_paths(args.save_path, 'binary')[0]))
    names = saved_classes(class_list, args)
    ids = filter_already_predicted(ids, args.save_path, names, args.overwrite, scored)
    times = dict.fromkeys(('read', 'predict', 'postprocess', 'measure', 'write'), 0.0)
    if not ids:
        print('Nothing to predict.')
        return [], times
    lib.require_device()
    spacings = read_spacing_csv(args.spacing_csv)
    models = init_model(args, class_list, old_classes)
    want_raw = args.save_probabilities or args.save_probabilities_lesions
    done = []

    def clock(key, t0):
        torch.cuda.synchronize()
        times[key] += time.perf_counter() - t0
        return time.perf_counter()

    with ThreadPoolExecutor(max_workers=1) as reader:
        nxt = reader.submit(load_case, args, ids[0], class_list)
        for k, img_name in enumerate(ids):
            case_id = case_id_of(img_name)
            t = time.perf_counter()
            hu, pancreas = nxt.result()
            if k + 1 < len(ids):
                nxt = reader.submit(load_case, args, ids[k + 1], class_list)
            t = clock('read', t)
            geom = None
            if isinstance(hu, NiftiVolume):
                pred_dict, raw, geom = predict_nifti_case(models, hu, args, class_list, return_raw=True)
            else:
                pred_dict, raw = predict_one(models, hu, pancreas, args, class_list)
            t = clock('predict', t)
            raw_dict = postprocess_npz(raw, class_list, args) if want_raw else None
            all_planes = pred_dict
            pred_dict = {n: pred_dict[n] for n in names}
            if raw_dict is not None:
                raw_dict = {n: raw_dict[n] for n in names}
            t = clock('postprocess', t)
            case_dir = os.path.join(args.save_path, case_id)
            if args.score:
                row, rows = score_case(pred_dict, raw_dict, names, spacings.get(case_id, (1.0, 1.0, 1.0) if geom is None else geom.spacing[::-1]),
                                       th=args.th, case_id=case_id)
                append_rows(args.save_path, row, rows)
                t = clock('measure', t)
            if args.lesion_table:
                from .inference.lesions import append_csv
                append_csv(os.path.join(args.save_path, 'lesions.csv'),
                           measure_lesions(all_planes, class_list, names, spacings.get(case_id, (1.0, 1.0, 1.0) if geom is None else geom.spacing[::-1]),
                                           case_id, args.lesion_min_voxels))
                t = clock('measure', t)
            if not args.not_save_binary or want_raw:
                os.makedirs(case_dir, exist_ok=True)
            if not args.not_save_binary and geom is not None:
                save_nifti_masks(case_dir, pred_dict, names, geom)
            elif not args.not_save_binary:
                write_binary(case_dir, pred_dict, names, args.packed, args.device_compress)
            if raw_dict is not None:
                write_raw(case_dir, raw_dict, names if args.save_probabilities else [n for n in names if any(w in n for w in LESION_WORDS)])
            clock('write', t)
            done.append(case_id)
            print(f'{img_name} finished.')
    return done, times


if __name__ == '__main__':
    main()
