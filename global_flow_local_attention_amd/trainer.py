"""One-process-per-GPU training shell around the UNMODIFIED reference generators.

The reference trains through `BaseModel` (model/base_model.py) + `nn.DataParallel` (model/face_model.py:81-93):
one Python process scatters the batch over the GPUs, gathers outputs and reduces gradients through GPU 0.  Here every
GPU has its own process (torch.distributed over RCCL), owns a slice of the batch, and the gradients are averaged by a
bucketed all-reduce launched from autograd hooks (dist.GradBucketReducer), overlapping the rest of backward.

* `load_reference_checkpoint(net, path)` -- the outcome of `BaseModel.load_networks` (base_model.py:154-197) as a key
  normalisation: strip / add the `module.` prefix DataParallel checkpoints carry, intersect with the network's keys,
  keep shape-matching entries; returns the top-level submodules that kept values of their own.
* `TrainerShell` -- one `optimize_parameters` step (pose_model.py:186-196) for one rank: shard, forward, loss terms,
  backward (reducer hooks), optimizer step.  The VGG style/content term needs a pretrained VGG19 and is injected as a
  callable (stubbed to zero by default, as BASELINE config 4 prescribes); the L1 reconstruction, sampling-correctness and
  affine-regularisation terms use this package's ops.  With `net_D=` the step is the reference's whole GAN step: the
  discriminator's update, then the generator's against the updated discriminator.
  `amp="fp16"` / `"bf16"` runs the generator and the losses under torch.autocast (fp16 with a GradScaler).
"""
import contextlib

import torch
import torch.nn as nn

from . import dist as gdist
from .adam import FusedAdam
from .losses import AdversarialLoss


_DP_PREFIX = "module."   # what nn.DataParallel / DistributedDataParallel put in front of every key


def _strip_prefix(key):
    return key[len(_DP_PREFIX):] if key.startswith(_DP_PREFIX) else key


def load_reference_checkpoint(net, path_or_state, map_location="cpu"):
    """Load a reference `<epoch>_net_G.pth` into `net` with the outcome `BaseModel.load_networks` has
    (base_model.py:154-197): an exact checkpoint loads as is; a checkpoint written from (or into) a DataParallel wrapper
    is matched modulo the `module.` prefix; surplus checkpoint entries are ignored; entries whose shape differs from the
    network's, and network entries the checkpoint lacks, keep the network's own values.  Returns the sorted top-level
    submodule names that kept at least one own value (empty list = every tensor came from the checkpoint).

    Implemented as key normalisation: both key sets are reduced to their prefix-free form, intersected, filtered by
    shape, and the survivors are written into the network's own state dict."""
    state = torch.load(path_or_state, map_location=map_location) if isinstance(path_or_state, str) else path_or_state
    own = net.state_dict()
    # network key -> checkpoint tensor, matching on the prefix-free name; an exact-name match wins over a normalised one
    # (the reference only falls back to prefix juggling when no key matches literally)
    by_plain = {}
    for key, tensor in state.items():
        by_plain.setdefault(_strip_prefix(key), tensor)
    literal_hits = sum(1 for key in own if key in state)
    chosen, kept_own = {}, set()
    for key, current in own.items():
        if literal_hits:
            candidate = state.get(key)
        else:
            candidate = by_plain.get(_strip_prefix(key))
        if candidate is not None and tuple(candidate.shape) == tuple(current.shape):
            chosen[key] = candidate
        else:
            kept_own.add(_strip_prefix(key).split(".")[0])
    merged = dict(own)
    merged.update(chosen)
    net.load_state_dict(merged)
    return sorted(kept_own)


class TrainerShell(object):
    """net_G: the reference generator (e.g. PoseGenerator built after gfla.install()); its forward is called as
    net_G(*inputs) and must return (generated, flow_fields, masks) like generator.py:13-36.
    lambdas: weights of the loss terms (pose_model.py:34-41 defaults).  gan_loss / style_content_loss: callables
    (generated, target) -> scalar; None = 0 (stubbed).
    amp: None (float32 step, the default), "fp16" -- the forward and the loss terms under torch.autocast("cuda",
    float16), the backward through a torch.amp.GradScaler -- or "bf16" (autocast bfloat16, no scaler).  With the scaler the
    bucketed all-reduce carries SCALED gradients: an inf / NaN on any rank reaches every rank through the sum, so every
    rank's scaler skips the same step.
    optimizer: "torch" (the default) steps with torch.optim.Adam; "kernels" with adam.FusedAdam at the same lr and betas:
    one launch for all parameters, and under amp="fp16" the scaler's unscale and skip inside that launch.

    net_D: a discriminator (e.g. ResDiscriminator built after gfla.install()).  None (the default): the generator's step
    alone, as above.  With one, `optimize_parameters` is the reference's whole step (pose_model.py:125-196): the generator
    forward once; `backward_D()` -- D(target) and D(generated.detach()), 0.5 * (loss(D_real, True, True) + loss(D_fake,
    False, True)) with AdversarialLoss(gan_mode), backward -- and a step of optimizer_D, the same class as optimizer_G at
    lr * ratio_g2d and the same betas; then `backward_G()`, in which the UPDATED D, frozen as gan_generator_term freezes it,
    judges the generated image and lambda_g * loss(D(generated), True, False) joins the sum as `ad_gen`; then the step of
    optimizer_G.  Under amp="fp16" D has a GradScaler of its own (`scaler_D`, `skipped_steps_D`): a skipped D step never
    skips G's.  Distributed runs reduce D's gradients through a second GradBucketReducer.  gan_loss= together with net_D=
    raises ValueError.  Not offered: the face model's second (video) discriminator, gan_mode "wgangp" (its penalty needs
    a double backward), learning-rate schedules."""

    AMP_DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
    OPTIMIZERS = {"torch": torch.optim.Adam, "kernels": FusedAdam}

    def __init__(self, net_G, lr=1e-4, betas=(0.0, 0.999), lambda_rec=5.0, lambda_correct=5.0, lambda_regularization=0.0025,
                 correctness=None, regularization=None, gan_loss=None, style_content_loss=None, attn_layer=(2, 3),
                 bucket_mb=32.0, amp=None, optimizer="torch", net_D=None, gan_mode="lsgan", lambda_g=2.0, ratio_g2d=0.1):
        if optimizer not in self.OPTIMIZERS:
            raise ValueError("TrainerShell: optimizer must be 'torch' or 'kernels' (got %r)" % (optimizer,))
        if amp is not None and amp not in self.AMP_DTYPES:
            raise ValueError("TrainerShell: amp must be None, 'fp16' or 'bf16' (got %r)" % (amp,))
        if net_D is not None and gan_loss is not None:
            raise ValueError("TrainerShell: gan_loss= is the adversarial term of a discriminator nobody updates; with "
                             "net_D= the shell computes the term itself -- pass one of the two")
        self.amp = amp
        self.scaler = torch.amp.GradScaler("cuda") if amp == "fp16" else None
        self.skipped_steps = 0   # steps the scaler skipped (inf / NaN in the gradients)
        self.net_G = net_G
        self.optimizer_G = self.OPTIMIZERS[optimizer]([p for p in net_G.parameters() if p.requires_grad], lr=lr, betas=betas)
        self.l1 = nn.L1Loss()
        self.lambdas = dict(rec=lambda_rec, correct=lambda_correct, regularization=lambda_regularization, g=lambda_g)
        self.correctness, self.regularization = correctness, regularization
        self.gan_loss, self.style_content_loss = gan_loss, style_content_loss
        self.attn_layer = list(attn_layer)
        self.reducer = gdist.GradBucketReducer(list(net_G.parameters()), bucket_mb=bucket_mb)
        self.net_D, self.gan_mode = net_D, gan_mode
        self.gan = AdversarialLoss(gan_mode)     # also checks gan_mode
        if net_D is not None:
            self.params_D = [p for p in net_D.parameters() if p.requires_grad]
            self.optimizer_D = self.OPTIMIZERS[optimizer](self.params_D, lr=lr * ratio_g2d, betas=betas)
            self.scaler_D = torch.amp.GradScaler("cuda") if amp == "fp16" else None
            self.skipped_steps_D = 0
            self.reducer_D = gdist.GradBucketReducer(list(net_D.parameters()), bucket_mb=bucket_mb)
        self.losses = {}
        self._log = {}

    def shard(self, *tensors):
        """This rank's slice of a global batch (DataParallel's scatter along dim 0)."""
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            return tensors
        r, w = torch.distributed.get_rank(), torch.distributed.get_world_size()
        return tuple(gdist.shard_batch(t, r, w) for t in tensors)

    def _autocast(self):
        return (torch.autocast("cuda", dtype=self.AMP_DTYPES[self.amp]) if self.amp is not None
                else contextlib.nullcontext())

    def forward(self, inputs, target, source=None):
        """The generator's forward on this rank's batch (pose_model.py:125-127); what the two backwards work on."""
        self.target, self.source = target, source
        with self._autocast():
            self.generated, self.flow_fields, _masks = self.net_G(*inputs)

    def backward_D(self):
        """pose_model.py:130-152: the discriminator's loss on the target and on the detached generated image, and its
        backward.  Leaves D's gradients (scaled ones under amp="fp16") in .grad and the loss in `loss_dis_img_gen`."""
        for p in self.params_D:                               # base_function._unfreeze
            p.requires_grad_(True)
        with self._autocast():
            d_real = self.net_D(self.target)
            d_fake = self.net_D(self.generated.detach())
            d_loss = (self.gan(d_real, True, True) + self.gan(d_fake, False, True)) * 0.5
        if self.scaler_D is not None:
            self.scaler_D.scale(d_loss).backward()
        else:
            d_loss.backward()
        self.reducer_D.finish()
        self.loss_dis_img_gen = d_loss.detach()
        self._log["dis_img_gen"] = self.loss_dis_img_gen

    def _judge(self, generated):
        """net_D(generated) with D frozen as gan_generator_term freezes it: no gradient reaches D's parameters, and their
        flags come back as they were found"""
        params = list(self.net_D.parameters())
        flags = [p.requires_grad for p in params]
        for p in params:
            p.requires_grad_(False)
        try:
            return self.net_D(generated)
        finally:
            for p, flag in zip(params, flags):
                p.requires_grad_(flag)

    def backward_G(self):
        """pose_model.py:154-183: the generator's loss terms and their backward (scaled under amp="fp16"), through the
        reducer's hooks."""
        generated, target, source, flow_fields = self.generated, self.target, self.source, self.flow_fields
        with self._autocast():
            terms = {"app_gen": self.l1(generated, target) * self.lambdas["rec"]}                   # pose_model.py:165
            if self.correctness is not None and source is not None:                                  # :158-159
                terms["correctness_gen"] = (self.correctness(target, source, flow_fields, self.attn_layer)
                                            * self.lambdas["correct"])
            if self.regularization is not None:                                                      # :161-162
                terms["regularization"] = self.regularization(flow_fields) * self.lambdas["regularization"]
            if self.gan_loss is not None:                                                            # :150-153
                terms["ad_gen"] = self.gan_loss(generated, target)
            elif self.net_D is not None:                                                             # :165-167
                terms["ad_gen"] = self.gan(self._judge(generated), True, False) * self.lambdas["g"]
            if self.style_content_loss is not None:                                                  # :168-176
                terms["style_content_gen"] = self.style_content_loss(generated, target)
            total = sum(terms.values())
        if self.scaler is not None:
            self.scaler.scale(total).backward()   # scaled gradients through the reducer's hooks
        else:
            total.backward()      # the reducer's hooks launch each bucket's all-reduce as soon as it is complete
        self.reducer.finish()
        self._log.update((k, v.detach()) for k, v in terms.items())

    def _step(self, optimizer, scaler):
        """the optimizer's step; True if the scaler skipped it (inf / NaN in the gradients)"""
        if scaler is None:
            optimizer.step()
            return False
        scale = scaler.get_scale()
        scaler.step(optimizer)    # unscales; skips the step if any gradient is inf / NaN
        scaler.update()
        return scaler.get_scale() < scale

    def optimize_parameters(self, inputs, target, source=None):
        """One step on THIS rank's (already sharded) batch: the generator's, and before it the discriminator's when there
        is one.  Returns the loss terms as floats, under the reference's names."""
        self._log = {}
        self.forward(inputs, target, source)
        if self.net_D is not None:
            self.optimizer_D.zero_grad(set_to_none=True)
            self.backward_D()
            self.skipped_steps_D += int(self._step(self.optimizer_D, self.scaler_D))
        self.optimizer_G.zero_grad(set_to_none=True)
        self.backward_G()
        self.skipped_steps += int(self._step(self.optimizer_G, self.scaler))
        self.losses = {k: float(v) for k, v in self._log.items()}
        return self.losses
