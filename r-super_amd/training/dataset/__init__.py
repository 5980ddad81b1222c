"""Host-side data formats of the training hot path: bit-packed label ingestion, epoch/rank sharding."""
from .packed import pack_bits, unpack_bits_device, ingest_packed_batch, PackedBits, pack_bits_device, upload_label  # noqa: F401
from .sampler import ChunkedSampler  # noqa: F401
from .synthetic import SyntheticUFODataset  # noqa: F401
from .augmented import AugmentedCropDataset, save_crop, estimate_tumor_volume  # noqa: F401
from .whole_volume import DeviceCropper  # noqa: F401
