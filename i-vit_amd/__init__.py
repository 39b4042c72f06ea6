"""i-vit_amd: MI355X-native integer-only ViT inference path.

Public surface mirrors the reference's `models` package for the I-ViT path
(/root/reference/models/__init__.py): the quantised operator modules, the DeiT/ViT and Swin factories and
freeze_model/unfreeze_model.  Everything computes through hand-written HIP kernels behind the C ABI of
include/ivit_hip.h; there is no PyTorch or CPU fallback."""
from .quantization_utils import *  # noqa: F401,F403
from .vit_quant import *  # noqa: F401,F403
from .swin_quant import *  # noqa: F401,F403
from .model_utils import freeze_model, unfreeze_model  # noqa: F401
from .knn import FeatureBank, knn_classify, retrieval_ap  # noqa: F401
from .probe import BankStats, LinearProbe, LogisticTrainer, fit_logistic  # noqa: F401
from .dense import DenseProbe, miou, patch_labels  # noqa: F401
from .propagate import davis_measures, mask_scores, upsample_argmax  # noqa: F401
from .discover import boxes_to_pixels, corloc, discover_objects, token_degrees  # noqa: F401
from .cluster import KMeans, partition_scores  # noqa: F401
