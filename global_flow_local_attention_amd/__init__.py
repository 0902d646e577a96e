"""MI355X (gfx950) implementation of the Global-Flow-Local-Attention feature-warping hot path.

Public surface = the reference's: BlockExtractor, LocalAttnReshape, Resample2d (+ their autograd
Functions) and ExtractorAttn; `install()` wires them into an unmodified reference checkout.
All compute is in libgfla_hip.so (csrc/, C ABI in include/gfla_hip.h); there is no CPU path.
"""
from ._lib import TUNING_KEYS, build, exported_symbols, path_count, set_tuning, tuned  # noqa: F401
globals().update(TUNING_KEYS)   # TUNE_*: the keys of set_tuning / tuned (include/gfla_hip.h: enum gfla_tuning_key)
from .block_extractor import BlockExtractor, BlockExtractorFunction  # noqa: F401
from .local_attn_reshape import LocalAttnReshape, LocalAttnReshapeFunction  # noqa: F401
from .resample2d import Resample2d, Resample2dFunction  # noqa: F401
from .extractor_attn import (BlockExtractorUnfoldFunction, ExtractorAttn, FcTailFunction, GraphedCall,  # noqa: F401
                             LocalAttnAggregateFunction, graphed_inference, patch_reference_extractor_attn)
from .losses import (AdversarialLoss, AffineRegFunction, AffineRegularizationLoss, GramL1Function,  # noqa: F401
                     MultiAffineRegularizationLoss, PerceptualLoss, StyleContentLoss, StyleLoss, VGGLoss, gan_generator_term,
                     gram_l1)
from .correctness import CorrectnessMapFunction, MaxCosineFunction, PerceptualCorrectness, max_cosine_similarity  # noqa: F401
from .flow_warp import BilinearSamplingBlock, FlowWarp, FlowWarpFunction, flow_warp  # noqa: F401
from .vgg import Conv3x3ReluFunction, MaxPool2x2Function, VGG19Features, conv3x3_relu, maxpool2x2  # noqa: F401
from .instance_norm import (InstanceNormAct, InstanceNormActFunction, fuse_instance_norm_act,  # noqa: F401
                            instance_norm_act)
from .head_conv import (HeadConv3x3, HeadConv3x3Function, flow_mask_heads, fuse_output_heads, head_conv3x3,  # noqa: F401
                        patch_reference_flow_heads, torch_head_conv3x3)
from .gen_conv import (Conv1x1Function, GenConvFunction, InferenceConv, conv1x1, conv3x3, conv4x4_down,  # noqa: F401
                       conv_transpose3x3_up, fuse_inference_convs, patch_reference_convs, torch_conv1x1, torch_gen_conv)
from .spectral_norm import (AvgPoolFrames, SpectralConv, SpectralConv3d, SpectralConvTranspose, SpectralHead,  # noqa: F401
                            SpectralNormFunction, fuse_spectral_norm, patch_reference_discriminators,
                            patch_reference_generators, spectral_normalize, torch_spectral_normalize)
from .conv3d import (AvgPoolFramesFunction, Conv3dFramesFunction, avg_pool_frames, conv3d_frames,  # noqa: F401
                     from_frames_major, to_frames_major, torch_avg_pool_frames, torch_conv3d_frames)
from .adam import FusedAdam  # noqa: F401
from .pose_inputs import (PoseInputs, normalize_images, pose_cords, pose_maps, torch_normalize_images,  # noqa: F401
                          torch_pose_cords, torch_pose_maps)
from .image_inputs import (affine_images, augmentation_matrices, resize_images, torch_affine_images,  # noqa: F401
                           torch_resize_images)
from .recon_metrics import (ReconstructionMetrics, images_to_uint8, reconstruction_metrics,  # noqa: F401
                            torch_images_to_uint8, torch_reconstruction_metrics)
from .install import install  # noqa: F401
from .trainer import TrainerShell, load_reference_checkpoint  # noqa: F401
from .face_step import (DualStreamAttn, MaskBlendFunction, face_target_forward, generate_frames,  # noqa: F401
                        patch_reference_face_target_net)

__version__ = "0.1.0"
