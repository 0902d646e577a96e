"""Shared by the CPU and GPU tests of TrainerShell's GAN step: a generator with PoseGenerator's call convention that runs on
any device and in any dtype, a batch for it, and pose_model.py:125-196 written out by hand as the reference to compare the
shell with."""
import torch
from torch import nn

import discriminator_util as du

STRUCTURE_NC = 2


class TinyGenerator(nn.Module):
    """(source, source_B, target_B) -> (generated, [], []): two convolutions and a tanh"""

    def __init__(self, width=6):
        super(TinyGenerator, self).__init__()
        self.body = nn.Sequential(nn.Conv2d(3 + 2 * STRUCTURE_NC, width, 3, 1, 1), nn.LeakyReLU(0.1),
                                  nn.Conv2d(width, 3, 3, 1, 1), nn.Tanh())

    def forward(self, source, source_B, target_B):
        return self.body(torch.cat((source, source_B, target_B), 1)), [], []


def batch(dtype=torch.float64, seed=3, shape=du.IMAGE):
    g = torch.Generator().manual_seed(seed)
    B, _, H, W = shape
    source = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    target = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    source_B, target_B = torch.rand(B, STRUCTURE_NC, H, W, generator=g), torch.rand(B, STRUCTURE_NC, H, W, generator=g)
    return tuple(t.to(dtype) for t in (source, target, source_B, target_B))


def networks(dtype=torch.float64, copies=2, seed=7):
    """`copies` pairs (generator, hooked discriminator) with equal parameters and buffers, in train() mode"""
    torch.manual_seed(seed)
    g0, d0 = TinyGenerator(), du.Discriminator()
    pairs = []
    for _ in range(copies):
        g, d = TinyGenerator(), du.Discriminator()
        g.load_state_dict(g0.state_dict())
        d.load_state_dict(d0.state_dict())
        pairs.append((g.to(dtype).train(), d.to(dtype).train()))
    return pairs


def hand_step(net_G, net_D, gan, inputs, target, lr=1e-3, betas=(0.0, 0.999), lambda_rec=5.0, lambda_g=2.0, ratio_g2d=0.1,
              optimizers=None):
    """pose_model.py:186-196 with the L1 and adversarial terms alone, operation by operation.  Returns the two losses, D's
    gradients as backward_D left them, and the optimizers (pass them back in for a second step)."""
    if optimizers is None:
        optimizers = (torch.optim.Adam([p for p in net_G.parameters() if p.requires_grad], lr=lr, betas=betas),
                      torch.optim.Adam([p for p in net_D.parameters() if p.requires_grad], lr=lr * ratio_g2d, betas=betas))
    optimizer_G, optimizer_D = optimizers
    img_gen, _flow_fields, _masks = net_G(*inputs)                            # forward()
    optimizer_D.zero_grad()
    for p in net_D.parameters():                                              # _unfreeze
        p.requires_grad = True
    D_real = net_D(target)
    D_real_loss = gan(D_real, True, True)
    D_fake = net_D(img_gen.detach())
    D_fake_loss = gan(D_fake, False, True)
    D_loss = (D_real_loss + D_fake_loss) * 0.5
    D_loss.backward()
    d_grads = {k: p.grad.clone() for k, p in net_D.named_parameters()}
    optimizer_D.step()
    optimizer_G.zero_grad()
    loss_app_gen = torch.nn.L1Loss()(img_gen, target) * lambda_rec
    for p in net_D.parameters():                                              # _freeze
        p.requires_grad = False
    D_fake = net_D(img_gen)
    loss_ad_gen = gan(D_fake, True, False) * lambda_g
    total_loss = 0
    for loss in (loss_app_gen, loss_ad_gen):
        total_loss += loss
    total_loss.backward()
    optimizer_G.step()
    for p in net_D.parameters():
        p.requires_grad = True
    return {"dis_img_gen": float(D_loss.detach()), "app_gen": float(loss_app_gen.detach()),
            "ad_gen": float(loss_ad_gen.detach())}, d_grads, optimizers
