"""3-D inference helpers mirroring rsuper_train/inference: forward-only reuse of the HIP conv stack, plus the prediction
post-processing of predict_abdomenatlas.py and the detection volumes of eval_AUC.py on the device."""
from .utils import get_inference, split_idx  # noqa: F401
from .inference3d import inference_whole_image, inference_sliding_window  # noqa: F401
from .postprocess import prediction, postprocess_npz, keep_largest_component  # noqa: F401
from .detection import detection, zoom_shape  # noqa: F401
