"""fp64 restatement of GanEngine's sub-steps with causal=True (gan_ffn_amd/engine.py: train_disc / train_gen when the
generators run under the causal mask), built on tests/engine_oracle.py (the sub-steps, the engine's dropout offsets and batch
layout), tests/causal_oracle.py (the oracle's attention with the causal mask) and tests/gan_mask_oracle.py (key lengths and the
masked BCE of mask_padding).

What changes against engine_oracle.disc_substep / gen_substep:
  * every GENERATOR pass — the eval-mode forward that makes the fake of a discriminator sub-step, the train-mode forward (and
    with it the backward) of a generator sub-step — runs inside causal_attention(lengths or None): query i attends to keys
    j <= i, and j < clamp(lengths[b], 1, S) when lengths are given;
  * every DISCRIMINATOR pass stays bidirectional: plain without lengths; with lengths inside masked_attention(lengths + lengths)
    for the [real | fake] pass of 2B dialogues and masked_attention(lengths) for the frozen pass of B dialogues, exactly as
    gan_mask_oracle has them;
  * the loss is the stock BCE mean without lengths and gan_mask_oracle.masked_bce with them.
lengths=None is GanEngine(causal=True), a list is GanEngine(causal=True, mask_padding=True).  At S = 1 the causal mask removes
nothing, so both sub-steps are engine_oracle's (tests/test_gan_causal_oracle_cpu.py)."""
import contextlib

import torch

import engine_oracle as EO
from causal_oracle import causal_attention
from gan_mask_oracle import disc_targets, masked_bce
from key_len_oracle import masked_attention
from oracle import ganffn_oracle as O


def _disc_attention(lengths):
    """the attention a discriminator pass runs under: the oracle's own without lengths, over the real keys with them"""
    return contextlib.nullcontext() if lengths is None else masked_attention(lengths)


def generator_eval(G, x, seed, b, i, lengths=None):
    """the fake a discriminator sub-step feeds its discriminator: G in eval mode under the causal mask"""
    a = b + EO.ADDS_PER_SUBSTEP * i
    with torch.no_grad(), causal_attention(lengths):
        return G.forward(x.to(torch.float64), seed, a + EO.G_ENC, a + EO.G_HEAD, False)


def disc_substep(D, G, x_real, x_partner, seed, b, i, lengths=None, fake=None, relu_masks=None):
    """engine.train_disc with causal=True: dict(loss, prob, fake, grads) as engine_oracle.disc_substep"""
    S, B = x_real.shape[:2]
    lengths = None if lengths is None else [int(n) for n in lengths]
    assert lengths is None or len(lengths) == B
    a = b + EO.ADDS_PER_SUBSTEP * i
    if fake is None:
        fake = generator_eval(G, x_partner, seed, b, i, lengths)
    fake = fake.detach().to(torch.float64)
    xr = x_real.to(torch.float64)
    if "object.weight" in D.P:
        xr = xr @ D.P["object.weight"].T + D.P["object.bias"]
    with _disc_attention(None if lengths is None else lengths + lengths):
        prob = D.forward(torch.cat((xr, fake), dim=1), seed, a + EO.D_ENC, a + EO.D_HEAD, True, relu_masks)
    if lengths is None:
        ones = torch.ones_like(prob[:, :B])
        loss = (O.bce_mean(prob[:, :B], ones) + O.bce_mean(prob[:, B:], torch.zeros_like(ones))) / 2.0
    else:
        loss = masked_bce(prob, disc_targets(S, B), lengths + lengths)
    grads = torch.autograd.grad(loss, [D.P[k] for k in D.trained])
    return dict(loss=float(loss.detach()), prob=prob.detach(), fake=fake, grads=dict(zip(D.trained, grads)))


def gen_substep(G, D, x, seed, b, i, lengths=None, relu_masks_G=None, relu_masks_D=None):
    """engine.train_gen with causal=True: dict(loss, out, grads) as engine_oracle.gen_substep; the frozen D is not causal"""
    lengths = None if lengths is None else [int(n) for n in lengths]
    a = b + EO.ADDS_PER_SUBSTEP * i
    with causal_attention(lengths):
        out = G.forward(x.to(torch.float64), seed, a + EO.G_ENC, a + EO.G_HEAD, True, relu_masks_G)
    with _disc_attention(lengths):
        prob = D.forward(out, seed, a + EO.D_ENC, a + EO.D_HEAD, False, relu_masks_D)
    loss = O.bce_mean(prob, torch.ones_like(prob)) if lengths is None else masked_bce(prob, 1.0, lengths)
    grads = torch.autograd.grad(loss, [G.P[k] for k in G.trained])
    return dict(loss=float(loss.detach()), out=out.detach(), grads=dict(zip(G.trained, grads)))
