"""Make the UNMODIFIED reference network code consume these ops.

The reference imports its ops by path (base_function.py:10,12,13; external_function.py:5-7;
generator.py:6):
    model.networks.block_extractor.block_extractor          -> BlockExtractor
    model.networks.local_attn_reshape.local_attn_reshape    -> LocalAttnReshape
    model.networks.resample2d_package.resample2d            -> Resample2d
`install()` registers this package's modules under those names in sys.modules (plus light stubs
for packages the reference imports at module scope but that the hot path never calls), so that
`import model.networks.generator` from a reference checkout picks them up with no source change.
See INTEGRATION.md.
"""
import importlib
import os
import sys
import types

from . import block_extractor, local_attn_reshape, resample2d
from .extractor_attn import patch_reference_extractor_attn

_ALIASES = {
    "model.networks.block_extractor.block_extractor": block_extractor,
    "model.networks.local_attn_reshape.local_attn_reshape": local_attn_reshape,
    "model.networks.resample2d_package.resample2d": resample2d,
}


def _namespace(name, path=None):
    mod = sys.modules.get(name)
    if mod is None:
        mod = types.ModuleType(name)
        mod.__path__ = [path] if path else []
        sys.modules[name] = mod
    return mod


def _bind_vgg(cls, vgg):
    """`cls` with `vgg` as its default feature extractor: the reference constructs its losses without arguments."""
    def __init__(self, *args, **kwargs):
        kwargs.setdefault("vgg", vgg)
        cls.__init__(self, *args, **kwargs)
    return type(cls.__name__, (cls,), {"__init__": __init__, "__doc__": cls.__doc__})


def install(reference_root=None, fuse_extractor_attn=True, stub_missing=True, allow_vendor_fallback=None,
            dual_stream_face=False, strict_mfma=None, vgg=None, bilinear_sampling_block=False, fuse_instance_norm=False,
            fuse_heads=False, inference_convs=False, train_convs=False, discriminator_convs=False, pointwise_convs=False,
            generator_spectral=False, temporal_convs=False):
    """Alias the three op modules; optionally patch the reference's ExtractorAttn with the fused
    forward.  `reference_root` (a checkout of the reference) is only needed if `model` is not
    already importable.  Returns the reference's `model.networks.base_function` module when it
    could be imported, else None.

    strict_mfma: an ExtractorAttn configuration this library's own MFMA kernels do not take (float32 with kernel_size
    other than 3 / 5 -- the reference's constructor default is 4 --, float32 maps too large for the LDS tiles; float64
    features, gradcheck included, run on the FP64 matrix cores) runs its FC layers through rocBLAS / MIOpen, with ONE warning per module, and every such call is counted
    (extractor_attn.vendor_fallback_calls): a drop-in must not turn a working reference configuration into a failure.
    strict_mfma=True (or GFLA_STRICT_MFMA=1 in the environment) makes it RAISE extractor_attn.VendorFallbackError instead
    -- what a benchmark or a deployment that must not ship vendor kernels by accident wants (bench.py sets it).  None
    leaves the process-wide policy as it is, so a second install() never flips it silently.  allow_vendor_fallback is the
    round-4 spelling: True = "warn", False = "error".

    dual_stream_face: also patch the reference's FaceTargetNet.forward (generator.py:480-505) so that the two ExtractorAttn
    of an attention layer (previous frame / reference frame) run on two HIP streams (face_step.py).  Imports the
    reference's generator module.

    vgg: a feature extractor (image -> {layer name: feature map}, e.g. the reference's VGG19 with its weights loaded).  When
    given, the reference's external_function.VGGLoss / StyleLoss / PerceptualLoss are replaced by this package's (losses.py:
    the Gram term on csrc/gram_l1.hip instead of bmm), constructed around it; imports the reference's external_function
    module.  None (the default) leaves them alone.

    bilinear_sampling_block: True replaces the reference's base_function.BilinearSamplingBlock by this package's
    (flow_warp.py: the warp on csrc/flow_warp.hip instead of a normalised grid and grid_sample; it also drops the
    reference's unconditional `.cuda()`).  False (the default) leaves the reference's class alone.

    fuse_instance_norm: True wraps the constructors of the reference's base_function block classes that build a
    `norm_layer(C) -> nonlinearity` sequence (EncoderBlock, ResBlock, ResBlockDecoder, ResBlockEncoder and every other
    class there that takes `norm_layer`), so that a network built AFTER install() has each nn.InstanceNorm2d + LeakyReLU /
    ReLU pair as one InstanceNormAct (instance_norm.py: csrc/instance_norm.hip instead of batch_norm on a reshaped view
    plus an activation launch).  Module indices, state-dict keys and the Parameter objects are unchanged, so reference
    checkpoints load as before.  False (the default) leaves the classes alone.

    fuse_heads: True (or "auto" / "torch", the `impl` of head_conv.py) closes the generators' tails on csrc/head_conv3x3.hip:
    the constructor of base_function.Output is wrapped so that an image head built AFTER install() is one HeadConv3x3
    (LeakyReLU -> ReflectionPad2d(1) -> Conv2d(ngf, 3, 3) -> Tanh; state-dict keys `conv1.*` and `model.2.*` and the
    Parameter objects unchanged), and `attn_output` of PoseFlowNet / FaceFlowNet / ShapeNetFlowNet computes the flow field
    and its sigmoid mask in one launch (head_conv.flow_mask_heads).  Imports the reference's generator module.  Heads built
    with spectral norm (unless generator_spectral is set: see there) or coordinate convolutions keep the reference's modules.  False (the default) changes nothing.

    inference_convs: True (or "auto" / "torch", the `impl` of gen_conv.py) wraps the constructors of the reference's
    EncoderBlock, ResBlock, ResBlockDecoder and Jump so that a generator built AFTER install() has its 3x3, 4x4 stride-2 and
    transposed 3x3 convolutions as InferenceConv (gen_conv.py: csrc/gen_conv.hip under eval() / torch.no_grad(), the torch
    composition whenever a gradient could be asked for), and replaces ResBlock.forward / ResBlockDecoder.forward by versions
    that add the residual in the last convolution's epilogue.  Indices, state-dict keys and the Parameter objects are
    unchanged.  Composes with fuse_instance_norm and fuse_heads.  False (the default) changes nothing.

    train_convs: with inference_convs, True makes those InferenceConv run the library's own gradient kernels as well
    (gen_conv.GenConvFunction, grad="kernels": csrc/gen_conv_bwd.hip and csrc/gen_conv_wgrad.hip) whenever a gradient is
    needed on a GPU map of float32 / float16 / bfloat16, so a training step of the generators' bodies calls no vendor
    convolution.  False (the default) keeps the torch composition for training.  Without inference_convs or
    discriminator_convs it raises ValueError.

    discriminator_convs: True (or "auto" / "torch", the `impl` of spectral_norm.py) wraps the constructors of the reference's
    ResDiscriminator, PatchDiscriminator and TemporalDiscriminator (discriminator.py) so that one built AFTER install() has
    every Conv2d under torch's spectral_norm hook as a SpectralConv: all normalisations of a forward are one batched call on
    csrc/spectral_norm.hip, and the 3x3 and 4x4 stride-2 convolutions run through gen_conv.py (with train_convs on its
    gradient kernels as well; the 1x1 convolutions keep F.conv2d on the normalised weight unless pointwise_convs is set,
    the k 4, s 1 ones always).
    ResBlockEncoder.forward hands shortcut(x) to the last convolution's epilogue.  Indices, state-dict keys, Parameter and
    buffer objects are unchanged.  Imports the reference's discriminator module.  False (the default) changes nothing.

    pointwise_convs: with inference_convs and / or discriminator_convs, True puts the 1x1 convolutions on gen_conv.conv1x1
    (csrc/conv1x1.hip) as well: the learnable shortcut of a generator's ResBlock (fuse_inference_convs(pointwise=True)),
    and in the discriminators the pooled shortcut of every ResBlockEncoder -- its AvgPool2d(2) folded into the convolution
    -- and the final Conv2d(C, 1, 1) (fuse_spectral_norm(pointwise="kernels")).  Together with train_convs a ResDiscriminator
    then trains with no vendor convolution at all.  False (the default) changes nothing; without inference_convs or
    discriminator_convs it raises ValueError.

    temporal_convs: with discriminator_convs, True puts the two ResBlock3DEncoder of a TemporalDiscriminator built AFTER
    install() on the library's own kernels as well (fuse_spectral_norm(temporal="kernels"), conv3d.py): the network
    converts its input to frames-major (B,L,C,H,W) once, the Conv3d of both blocks run as 2-D convolutions over a sliding
    window of three frames (csrc/conv3d.hip), the AvgPool3d((3,2,2), (1,2,2)) on csrc/avg_pool_frames.hip, the 1x1x1 bypass
    on csrc/conv1x1.hip, and their spectral norms join the one batched call.  With train_convs and pointwise_convs a
    TemporalDiscriminator then trains with no vendor convolution or pool.  State-dict keys, Parameter and buffer objects are
    unchanged.  False (the default) changes nothing; without discriminator_convs it raises ValueError.

    generator_spectral: True (or "auto" / "torch", the `impl` of spectral_norm.py) wraps the constructors of the reference's
    PoseGenerator, PoseFlowNetGenerator, DanceGenerator, FaceGenerator, ShapeNetGenerator and ShapeNetFlowNetGenerator
    (generator.py) so that one built AFTER install() with spectral norm (the pose model's default, --use_spect_g) has every
    hooked convolution on the library: Conv2d as SpectralConv, ConvTranspose2d (normalised along dim 1) as
    SpectralConvTranspose, every Jump as a reflect-padded SpectralConv, the Output head as a SpectralHead
    (fuse_spectral_norm(generator=True)) -- one batched normalisation per forward of the whole generator -- and ResBlock /
    ResBlockDecoder add their residual in the last convolution's epilogue.  With train_convs the convolutions train on the
    library's gradient kernels, with pointwise_convs the 1x1 shortcuts run gen_conv.conv1x1; either accepts
    generator_spectral as the flag it needs.  CoordConv and ExtractorAttn keep the reference's modules.  Indices,
    state-dict keys, Parameter and buffer objects are unchanged.  Composes with fuse_instance_norm.  Imports the reference's
    generator module.  False (the default) changes nothing."""
    if temporal_convs and not discriminator_convs:
        raise ValueError("install: temporal_convs=True needs discriminator_convs")
    if pointwise_convs and not (inference_convs or discriminator_convs or generator_spectral):
        raise ValueError("install: pointwise_convs=True needs inference_convs, discriminator_convs or generator_spectral")
    if train_convs and not (inference_convs or discriminator_convs or generator_spectral):
        raise ValueError("install: train_convs=True needs inference_convs%s"
                         % ("" if not discriminator_convs else " or discriminator_convs"))
    from . import extractor_attn as _ea
    if strict_mfma is None and allow_vendor_fallback is not None:
        strict_mfma = not allow_vendor_fallback
    if strict_mfma is None and os.environ.get("GFLA_STRICT_MFMA"):
        strict_mfma = os.environ["GFLA_STRICT_MFMA"] not in ("0", "")
    if strict_mfma is not None:
        _ea.VENDOR_FALLBACK = "error" if strict_mfma else "warn"
    if reference_root:
        # a bare namespace for `model` skips model/__init__.py (which pulls in skimage etc.)
        _namespace("model", os.path.join(reference_root, "model"))
        _namespace("model.networks", os.path.join(reference_root, "model", "networks"))
        if reference_root not in sys.path:
            sys.path.insert(0, reference_root)
    for pkg in ("model.networks.block_extractor", "model.networks.local_attn_reshape",
                "model.networks.resample2d_package"):
        if reference_root or pkg.rsplit(".", 1)[0] in sys.modules:
            _namespace(pkg)
    for name, mod in _ALIASES.items():
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        if parent in sys.modules:
            setattr(sys.modules[parent], leaf, mod)
    if stub_missing:
        for missing in ("imageio", "natsort"):
            try:
                importlib.import_module(missing)
            except ImportError:
                stub = types.ModuleType(missing)
                if missing == "natsort":
                    stub.natsorted = sorted
                sys.modules[missing] = stub
    base_function = None
    if "model.networks" in sys.modules:
        try:
            base_function = importlib.import_module("model.networks.base_function")
        except ImportError:
            base_function = None
    if base_function is not None and fuse_extractor_attn and hasattr(base_function, "ExtractorAttn"):
        patch_reference_extractor_attn(base_function.ExtractorAttn)
    if base_function is not None and dual_stream_face:
        from .face_step import patch_reference_face_target_net
        generator = importlib.import_module("model.networks.generator")
        patch_reference_face_target_net(generator.FaceTargetNet)
    if base_function is not None and bilinear_sampling_block:
        from .flow_warp import BilinearSamplingBlock
        base_function.BilinearSamplingBlock = BilinearSamplingBlock
    if base_function is not None and fuse_instance_norm:
        from .instance_norm import patch_reference_blocks
        patch_reference_blocks(base_function)
    if base_function is not None and fuse_heads:
        from .head_conv import patch_reference_flow_heads, patch_reference_outputs
        impl = fuse_heads if isinstance(fuse_heads, str) else "auto"
        patch_reference_outputs(base_function, impl)
        patch_reference_flow_heads(importlib.import_module("model.networks.generator"), impl)
    if base_function is not None and inference_convs:
        from .gen_conv import patch_reference_convs
        patch_reference_convs(base_function, inference_convs if isinstance(inference_convs, str) else "auto",
                              "kernels" if train_convs else "torch", bool(pointwise_convs))
    if base_function is not None and discriminator_convs:
        from .spectral_norm import patch_reference_discriminators
        patch_reference_discriminators(importlib.import_module("model.networks.discriminator"), base_function,
                                       discriminator_convs if isinstance(discriminator_convs, str) else "auto",
                                       "kernels" if train_convs else "torch",
                                       "kernels" if pointwise_convs else "torch",
                                       "kernels" if temporal_convs else "torch")
    if base_function is not None and generator_spectral:
        from .spectral_norm import patch_reference_generators
        patch_reference_generators(importlib.import_module("model.networks.generator"), base_function,
                                   generator_spectral if isinstance(generator_spectral, str) else "auto",
                                   "kernels" if train_convs else "torch", "kernels" if pointwise_convs else "torch")
    if vgg is not None:
        from . import losses
        external_function = importlib.import_module("model.networks.external_function")
        for cls in (losses.VGGLoss, losses.StyleLoss, losses.PerceptualLoss):
            setattr(external_function, cls.__name__, _bind_vgg(cls, vgg))
    return base_function
