"""fp64 restatement of one GanEngine sub-step in TRAIN mode (gan_ffn_amd/engine.py: train_disc / train_gen), with the
engine's own dropout offsets and batch layout.  Built from the oracle's pieces (oracle/ganffn_oracle.py: encoder_stack,
bce_mean, the dropout sites); the oracle's own train_disc / train_gen restate the REFERENCE (D(real) and D(fake) as two
passes) and stay as they are — tests/test_engine_oracle_cpu.py pins this restatement to them.

What the engine does, and this module restates:
  train_disc(who, partner), sub-step i of an iteration whose block of dropout offsets starts at b:
    fake  = G_partner(x_partner) in eval mode (no dropout, nothing saved);
    real' = object(x_who) for a discriminator with an `object` layer, x_who otherwise;
    prob  = D_who([real' | fake]) in train mode: ONE pass over 2B dialogues (token row t = s * 2B + col), encoder masks at
            offset b + 4i + 2, head masks at b + 4i + 3;
    loss  = (BCE(prob[:, :B], 1) + BCE(prob[:, B:], 0)) / 2 over every padded position; gradients to every D parameter.
  train_gen(who, partner):
    out   = G_who(x_who) in train mode, encoder masks at b + 4i, head masks at b + 4i + 1;
    prob  = D_partner(out) in eval mode (frozen);
    loss  = BCE(prob, 1); gradients to G only.
Dropout probabilities are the network's own (engine.NetState p_pe / p_enc / p_head)."""
import math

import numpy as np
import torch

from oracle import ganffn_oracle as O

# dropout offsets of sub-step i relative to the iteration's block (engine.ADDS_PER_SUBSTEP = 4)
G_ENC, G_HEAD, D_ENC, D_HEAD = 0, 1, 2, 3
ADDS_PER_SUBSTEP = 4


class Net:
    """fp64 parameters of one network (reference state_dict names) and the dropout probabilities it runs with."""

    def __init__(self, kind, P, H, p_pe, p_enc, p_head, requires_grad=True):
        self.kind, self.H = kind, H
        self.p_pe, self.p_enc, self.p_head = float(p_pe), float(p_enc), float(p_head)
        self.P = {}
        for k, v in P.items():
            t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().to(torch.float64).clone()
            if requires_grad and k != "position_encoding.pe" and not k.startswith("encoder_layer."):
                t.requires_grad_(True)
            self.P[k] = t
        self.trained = [k for k, v in self.P.items() if v.requires_grad]

    @classmethod
    def from_state(cls, st, slab, requires_grad=True):
        """an engine.NetState's network from a host copy of its parameter slab"""
        P = {}
        for k, (off, shape) in st.named.items():
            n = int(np.prod(shape))
            P[k] = slab[off:off + n].view(*shape)
        P["position_encoding.pe"] = st.pe.detach().cpu()
        return cls("gen" if st.kind == 0 else "disc", P, st.H, st.p_pe, st.p_enc, st.p_head, requires_grad)

    def enc_rng(self, seed, offset, train):
        if not train or (self.p_pe == 0.0 and self.p_enc == 0.0):
            return None
        # the oracle's encoder sites draw at the reference's fixed probabilities (PositionalEncoding 0.2, encoder layers 0.1)
        assert (self.p_pe, self.p_enc) == (O.PE_DROPOUT, O.ENC_DROPOUT), (self.p_pe, self.p_enc)
        return O.Rng(seed, offset, True)

    def head(self, h, rng):
        """generator: gelu(drop(fc2(gelu(drop(fc1(drop(gelu(h)))))))); discriminator: sigmoid(drop(fc3(...)))"""
        P, p = self.P, self.p_head
        t = O.gelu(h)
        if self.kind == "gen":
            t = O._drop(t, p, O.SITE_HEAD0, rng)
        t = O.gelu(O._drop(t @ P["fc1.weight"].T + P["fc1.bias"], p, O.SITE_HEAD1, rng))
        t = O.gelu(O._drop(t @ P["fc2.weight"].T + P["fc2.bias"], p, O.SITE_HEAD2, rng))
        if self.kind == "gen":
            return t
        return torch.sigmoid(O._drop(t @ P["fc3.weight"].T + P["fc3.bias"], p, O.SITE_HEAD3, rng))

    def forward(self, x, seed, enc_off, head_off, train, relu_masks=None):
        h = O.encoder_stack(x, self.P, self.H, self.enc_rng(seed, enc_off, train), relu_masks=relu_masks)
        r = O.Rng(seed, head_off, True) if (train and self.p_head > 0.0) else None
        return self.head(h, r)


def disc_substep(D, G, x_real, x_partner, seed, b, i, fake=None, relu_masks=None):
    """engine.train_disc: returns dict(loss, prob, fake, grads={name: dL/dparam}) for the discriminator D.
    fake: the generator's eval-mode output to feed D (default: computed here from G); relu_masks: per-layer (S, 2B, 2048)
    patterns for D's encoder (default: its own)."""
    B = x_real.shape[1]
    if fake is None:
        with torch.no_grad():
            fake = G.forward(x_partner, seed, b + ADDS_PER_SUBSTEP * i + G_ENC, b + ADDS_PER_SUBSTEP * i + G_HEAD, False)
    fake = fake.detach().to(torch.float64)
    xr = x_real.to(torch.float64)
    if "object.weight" in D.P:
        xr = xr @ D.P["object.weight"].T + D.P["object.bias"]
    a = b + ADDS_PER_SUBSTEP * i
    prob = D.forward(torch.cat((xr, fake), dim=1), seed, a + D_ENC, a + D_HEAD, True, relu_masks)
    ones = torch.ones_like(prob[:, :B])
    loss = (O.bce_mean(prob[:, :B], ones) + O.bce_mean(prob[:, B:], torch.zeros_like(ones))) / 2.0
    grads = torch.autograd.grad(loss, [D.P[k] for k in D.trained])
    return dict(loss=float(loss.detach()), prob=prob.detach(), fake=fake, grads=dict(zip(D.trained, grads)))


def gen_substep(G, D, x, seed, b, i, relu_masks_G=None, relu_masks_D=None):
    """engine.train_gen: returns dict(loss, out, grads) for the generator G; D is frozen, in eval mode."""
    a = b + ADDS_PER_SUBSTEP * i
    out = G.forward(x.to(torch.float64), seed, a + G_ENC, a + G_HEAD, True, relu_masks_G)
    prob = D.forward(out, seed, a + D_ENC, a + D_HEAD, False, relu_masks_D)
    loss = O.bce_mean(prob, torch.ones_like(prob))
    grads = torch.autograd.grad(loss, [G.P[k] for k in G.trained])
    return dict(loss=float(loss.detach()), out=out.detach(), grads=dict(zip(G.trained, grads)))


def adam(p, g, m, v, t, lr, b1, b2, eps=1e-8):
    """torch.optim.Adam's step t (weight decay 0) in fp64 on numpy arrays; returns (p, m, v)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps), m, v
