"""3-D inference helpers mirroring rsuper_train/inference: forward-only reuse of the HIP conv stack, plus the prediction
post-processing of predict_abdomenatlas.py, the detection volumes of eval_AUC.py and test_with_reports.py on the device, and the whole-case flow of predict_abdomenatlas.py
(preprocess -> prediction -> unpad_img -> resample_image_with_gpu -> postprocess_npz) under the reference's names, with a NIfTI front and back
end (read, reorient, B-spline resample, masks back as .nii.gz) that needs neither SimpleITK nor nibabel."""
from .utils import get_inference, split_idx  # noqa: F401
from .inference3d import inference_whole_image, inference_sliding_window  # noqa: F401
from .postprocess import prediction, postprocess_npz, keep_largest_component  # noqa: F401
from .detection import detection, detection_binary, zoom_shape  # noqa: F401
from .preprocess import normalize_ct, pad_to_training_size, unpad_img, preprocess_array  # noqa: F401
from .resample import resample_image_with_gpu, predict_case  # noqa: F401
from .scoring import score_case  # noqa: F401
from .npz_writer import deflate_device, savez_compressed_device, save_planes_npz, gzip_device  # noqa: F401
from .nifti import read_nifti, affine, orientation_plan, nifti1_header, resample_axis_table  # noqa: F401
from .nifti_device import load_nifti_device, predict_nifti_case, save_nifti_masks  # noqa: F401
from .lesions import (LesionTable, lesion_table, match_lesions, locate_lesions, lesion_report_rows, compare_with_report,  # noqa: F401
                      lesion_csv_rows)
