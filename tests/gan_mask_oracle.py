"""fp64 restatement of GanEngine's sub-steps with mask_padding=True (gan_ffn_amd/engine.py: train_disc / train_gen when the
batch carries key lengths), built on tests/engine_oracle.py (the unmasked sub-steps, the engine's dropout offsets and batch
layout) and tests/key_len_oracle.py (the oracle's attention with key lengths).

What changes against engine_oracle.disc_substep / gen_substep, for lengths n_b = clamp(lengths[b], 1, S):
  * every encoder pass attends over keys j < n_b of its dialogue only: the generator's and the frozen discriminator's passes of
    B dialogues with `lengths`, the discriminator's [real | fake] pass of 2B dialogues with `lengths` twice;
  * the losses are means over the real utterances: masked_bce(prob, target, column lengths) = the sum over s < n_c of the
    BCELoss terms (logs clamped at -100) divided by count = sum_c n_c.  The real and the fake half of a discriminator pass have
    the same lengths, so the one masked mean over [real | fake] with targets [1 | 0] is (BCE(real, 1) + BCE(fake, 0)) / 2 over
    real utterances.
With every length = S both are engine_oracle's sub-steps (tests/test_gan_mask_oracle_cpu.py)."""
import math

import torch

import engine_oracle as EO
from key_len_oracle import masked_attention, valid_rows


def clamp_lengths(lengths, S):
    """the kernels' clamp: a length of 0 or above S is not refused"""
    return [min(max(int(n), 1), S) for n in lengths]


def masked_bce(prob, target, lengths):
    """prob, target: (S, Bt) or (S, Bt, 1) fp64; lengths: Bt column lengths -> the mean of the BCELoss terms over s < n_c"""
    p = prob.reshape(prob.shape[0], prob.shape[1])
    y = torch.as_tensor(target, dtype=p.dtype).expand_as(p) if not torch.is_tensor(target) or target.dim() == 0 else \
        target.reshape(p.shape).to(p.dtype)
    S = p.shape[0]
    valid = valid_rows(S, clamp_lengths(lengths, S))
    assert valid.shape == p.shape, (valid.shape, p.shape)
    # max(log v, -100) written as log(max(v, e^-100)): the same value, and under autograd a saturated probability (an fp64
    # sigmoid that reached exactly 0 or 1, at a padded row for instance) contributes a gradient of 0 instead of 0 * inf = NaN
    floor = math.exp(-100.0)
    lp = torch.log(torch.clamp(p, min=floor))
    l1p = torch.log(torch.clamp(1.0 - p, min=floor))
    terms = -(y * lp + (1.0 - y) * l1p)
    return terms[valid].sum() / float(int(valid.sum()))


def masked_bce_grad(prob, target, lengths, scale=1.0):
    """d (scale * masked_bce) / d prob as the kernel states it: scale / count * (p - y) / max(p (1 - p), 1e-12) at s < n_c, 0
    elsewhere (autograd through the clamped logs is 0 where a log is clamped; the kernel's form is BCELoss's own backward)"""
    p = prob.reshape(prob.shape[0], prob.shape[1])
    y = torch.as_tensor(target, dtype=p.dtype).expand_as(p) if not torch.is_tensor(target) or target.dim() == 0 else \
        target.reshape(p.shape).to(p.dtype)
    S = p.shape[0]
    valid = valid_rows(S, clamp_lengths(lengths, S))
    g = scale / float(int(valid.sum())) * (p - y) / torch.clamp(p * (1.0 - p), min=1e-12)
    return torch.where(valid, g, torch.zeros_like(g)).reshape(prob.shape)


def disc_targets(S, B, dtype=torch.float64):
    """targets of a [real | fake] pass: (S, 2B), 1 on the real half"""
    return torch.cat((torch.ones(S, B, dtype=dtype), torch.zeros(S, B, dtype=dtype)), dim=1)


def disc_substep(D, G, x_real, x_partner, seed, b, i, lengths, fake=None, relu_masks=None):
    """engine.train_disc with mask_padding: dict(loss, prob, fake, grads) as engine_oracle.disc_substep"""
    S, B = x_real.shape[:2]
    lengths = [int(n) for n in lengths]
    assert len(lengths) == B
    a = b + EO.ADDS_PER_SUBSTEP * i
    if fake is None:
        with torch.no_grad(), masked_attention(lengths):
            fake = G.forward(x_partner, seed, a + EO.G_ENC, a + EO.G_HEAD, False)
    fake = fake.detach().to(torch.float64)
    xr = x_real.to(torch.float64)
    if "object.weight" in D.P:
        xr = xr @ D.P["object.weight"].T + D.P["object.bias"]
    with masked_attention(lengths + lengths):
        prob = D.forward(torch.cat((xr, fake), dim=1), seed, a + EO.D_ENC, a + EO.D_HEAD, True, relu_masks)
    loss = masked_bce(prob, disc_targets(S, B), lengths + lengths)
    grads = torch.autograd.grad(loss, [D.P[k] for k in D.trained])
    return dict(loss=float(loss.detach()), prob=prob.detach(), fake=fake, grads=dict(zip(D.trained, grads)))


def gen_substep(G, D, x, seed, b, i, lengths, relu_masks_G=None, relu_masks_D=None):
    """engine.train_gen with mask_padding: dict(loss, out, grads) as engine_oracle.gen_substep"""
    lengths = [int(n) for n in lengths]
    a = b + EO.ADDS_PER_SUBSTEP * i
    with masked_attention(lengths):
        out = G.forward(x.to(torch.float64), seed, a + EO.G_ENC, a + EO.G_HEAD, True, relu_masks_G)
        prob = D.forward(out, seed, a + EO.D_ENC, a + EO.D_HEAD, False, relu_masks_D)
    loss = masked_bce(prob, 1.0, lengths)
    grads = torch.autograd.grad(loss, [G.P[k] for k in G.trained])
    return dict(loss=float(loss.detach()), out=out.detach(), grads=dict(zip(G.trained, grads)))
