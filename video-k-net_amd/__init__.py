"""video_k_net_amd — MI355X-native kernel-update head for Video K-Net (directory `video-k-net_amd/`).

Importing this package registers `KernelUpdator` (TRANSFORMER_LAYER) and `KernelUpdateHead`, `VideoKernelUpdateHead`,
`KernelIterHead`, `VideoKernelIterHead`, `ConvKernelHead`, `SemanticFPNWrapper` (HEADS; mmdet's NECKS where that name is free) — into mmcv/mmdet's registries when they are importable, else into the bundled
ones — `MSDeformAttnPixelDecoder` into `NECKS` and `SwinTransformerDIY` into `BACKBONES`, so the reference's config dicts build these classes unchanged.  All arithmetic runs in
`lib/libvkn.so` (hand-written HIP for gfx950, C ABI in include/vkn.h); there is no CPU fallback.
"""
from . import _lib, configs, ops, registry  # noqa: F401
from ._lib import VknError, VknLibraryError, build  # noqa: F401
from .kernel_updator import KernelUpdator  # noqa: F401
from .kernel_update_head import KernelUpdateHead, VideoKernelUpdateHead  # noqa: F401
from .kernel_iter_head import KernelIterHead, VideoKernelIterHead  # noqa: F401
from .semantic_fpn import SemanticFPNWrapper, SinePositionalEncoding  # noqa: F401
from .kernel_head import ConvKernelHead, ConvKernelHeadVideo  # noqa: F401
from .msdeform_decoder import MSDeformAttnPixelDecoder  # noqa: F401
from .swin import SwinTransformerDIY  # noqa: F401
from .knet_vis import KernelFrameIterHeadVideo, KernelIterHeadVideo, KernelUpdateHeadVideo  # noqa: F401
from .mask_hungarian_assigner import MaskHungarianAssigner, MaskHungarianAssignerVideo  # noqa: F401
from .qd_tracker import QuasiDenseEmbedTracker, build_tracker  # noqa: F401
from .track_heads import QuasiDenseMaskEmbedHeadGTMask  # noqa: F401
from .track_tail import TrackTail  # noqa: F401
from .track_train_tail import TrackTrainTail  # noqa: F401
from .gt_prep import GtPrep  # noqa: F401
from .seg_tail import SegLossTail  # noqa: F401
from .stq_meter import STQMeter  # noqa: F401
from .vpq_meter import VPQMeter  # noqa: F401
from .mask_rle import MaskRLE, encode_mask_results  # noqa: F401
from .mask_ap_meter import MaskAPMeter  # noqa: F401
from .registry import BACKBONES, HEADS, NECKS, TRANSFORMER_LAYER, build_backbone, build_head, build_neck, build_transformer_layer  # noqa: F401
from . import autograd, losses  # noqa: F401
from .mask_pseudo_sampler import MaskPseudoSampler  # noqa: F401

registry._register_training_components()

__all__ = ['KernelUpdator', 'KernelUpdateHead', 'VideoKernelUpdateHead', 'KernelIterHead', 'VideoKernelIterHead', 'ConvKernelHead', 'SemanticFPNWrapper', 'MSDeformAttnPixelDecoder', 'SwinTransformerDIY', 'MaskHungarianAssigner', 'MaskHungarianAssignerVideo',
           'BACKBONES', 'HEADS', 'NECKS', 'TRANSFORMER_LAYER', 'build_backbone', 'build_head', 'build_neck', 'build_transformer_layer', 'ops', 'build', 'VknError',
           'VknLibraryError']
