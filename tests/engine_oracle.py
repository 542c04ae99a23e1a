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
Dropout probabilities are the network's own (engine.NetState p_pe / p_enc / p_head).

The classifier step runners (see the section below): Phase2Engine.step (phase2_step: generators -> sum -> fc -> weighted
MaskedNLLLoss) and DrnnEngine._step (drnn_step: generators -> sum -> the CPU fp64 BiModel of gan_ffn_amd/dialogue_rnn.py
with the engine's masks -> weighted MaskedNLLLoss); both with L2-coupled Adam (adam_wd)."""
import math

import numpy as np
import torch

from oracle import ganffn_oracle as O
from oracle import philox

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


def adam_wd(p, g, m, v, t, lr, b1, b2, wd, eps=1e-8):
    """torch.optim.Adam's step t with L2-coupled weight decay (g += wd * p before the moments; train_IEMOCAP.py:661,
    train_IEMOCAP_DialogueRNN.py:746); returns (p, m, v)"""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    return adam(p, g + wd * p, m, v, t, lr, b1, b2, eps)


# ================================================================================================================
# The classifier step runners: Phase2Engine.step (phase 2 of train_IEMOCAP.py) and DrnnEngine._step (configuration 5,
# GAN_FFN_DialogueRNN).  Both draw ONE block of offsets per step from the device allocator (b = rng.next_add(8 | 10)):
#   generators, in GEN_KEYS order: encoder b + 2j, head b + 2j + 1;
#   DrnnEngine only: the recurrence b + 6 (sites 8 + 4z + {0 global, 1 party, 2 emotion, 3 listener}, z = direction), the
#   head b + 7 (site 5: the forward half of the emotions, 6: the reversed backward half, 7: the hidden layer).
# ================================================================================================================
GEN_KEYS = ("acoustic", "visual", "text")
PHASE2_ADDS, DRNN_ADDS = 8, 10
A_REC, A_HEAD = 6, 7
SITE_JOIN_F, SITE_JOIN_B, SITE_HIDDEN = 5, 6, 7
SITE_REC = 8


def gen_adds(b):
    """{generator: (encoder offset, head offset)} of a step whose block starts at b"""
    return {k: (b + 2 * j, b + 2 * j + 1) for j, k in enumerate(GEN_KEYS)}


def generators(gens, xs, seed, adds, relu_masks=None):
    """{k: G_k(x_k)}: train mode at the offsets `adds` ({k: (enc, head)}), eval mode when adds is None; relu_masks: {k: the
    per-layer (S, B, 2048) patterns of that generator} (default: the oracle's own)"""
    out = {}
    for k in GEN_KEYS:
        a0, a1 = adds[k] if adds is not None else (0, 0)
        out[k] = gens[k].forward(xs[k].to(torch.float64), seed, a0, a1, adds is not None,
                                 None if relu_masks is None else relu_masks[k])
    return out


def generator_grads(gens, outs, d_fusion):
    """{k: {name: dL/dparam}} of each generator from dL/dfusion (fusion = the sum of the outputs: each gets all of it)"""
    res = {}
    for k in GEN_KEYS:
        g = torch.autograd.grad(outs[k], [gens[k].P[n] for n in gens[k].trained], d_fusion, retain_graph=True)
        res[k] = dict(zip(gens[k].trained, g))
    return res


def phase2_head(fusion, fc_w, fc_b, label, umask, class_w=None):
    """log_softmax(fc(fusion)) and the weighted MaskedNLLLoss (model.py:1448-1449, :62-81) -> dict(log_prob, loss, d_fusion,
    grad_fc_weight, grad_fc_bias); every input is taken as a constant fp64 tensor"""
    f = torch.as_tensor(fusion).detach().to(torch.float64).requires_grad_(True)
    w = torch.as_tensor(fc_w).detach().to(torch.float64).requires_grad_(True)
    b = torch.as_tensor(fc_b).detach().to(torch.float64).requires_grad_(True)
    lp = torch.log_softmax(f @ w.T + b, dim=2)
    cw = None if class_w is None else torch.as_tensor(class_w, dtype=torch.float64)
    loss = O.masked_nll(lp, label, umask.to(torch.float64), cw)
    df, gw, gb = torch.autograd.grad(loss, [f, w, b])
    return dict(log_prob=lp.detach(), loss=float(loss.detach()), d_fusion=df, grad_fc_weight=gw, grad_fc_bias=gb)


def phase2_step(gens, fc_w, fc_b, batch, seed, adds, relu_masks=None, class_w=None):
    """Phase2Engine.step chained end to end: the three generators (EO.Net), fusion = their sum, the classifier head, and
    the gradients of every parameter -> dict(fusion, log_prob, loss, grad_fc_weight, grad_fc_bias, grads={k: {name: g}})"""
    outs = generators(gens, batch, seed, adds, relu_masks)
    fusion = outs["acoustic"] + outs["visual"] + outs["text"]
    head = phase2_head(fusion.detach(), fc_w, fc_b, batch["label"], batch["umask"], class_w)
    res = dict(head, fusion=fusion.detach(), grads=generator_grads(gens, outs, head["d_fusion"]))
    return res


# ---- configuration 5 --------------------------------------------------------------------------------------------------
class MaskSeq(torch.nn.Module):
    """stands in for a dropout module: multiplies by the next prepared (already 1/(1-p)-scaled) mask"""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.i = list(masks), 0

    def forward(self, x):
        m = self.masks[self.i]
        self.i += 1
        return x * m


def _keep(R, C, p, site, seed, offset):
    return torch.from_numpy(philox.keep_mask(R, C, p, site, seed, offset)).to(torch.float64) / (1.0 - p)


def rec_masks(S, B, H, He, p, seed, offset, z, listener):
    """the dropout calls of DialogueRNNCell (model.py:862-926) of direction z, step by step, as the HIP recurrence draws
    them: rows t * B + b in the direction's OWN time order (the reverse direction's step t is utterance len_b - 1 - t);
    g (B, H) site 8 + 4z; the party update qs (B, 2, H) site 9 + 4z, one row for both parties; with listener state ql
    (B, 2, H) site 11 + 4z, one row of 2H per (t, b); e (B, He) site 10 + 4z"""
    s0 = SITE_REC + 4 * z
    kg, kp = _keep(S * B, H, p, s0, seed, offset).view(S, B, H), _keep(S * B, H, p, s0 + 1, seed, offset).view(S, B, H)
    ke = _keep(S * B, He, p, s0 + 2, seed, offset).view(S, B, He)
    kl = _keep(S * B, 2 * H, p, s0 + 3, seed, offset).view(S, B, 2, H) if listener else None
    out = []
    for t in range(S):
        out += [kg[t], kp[t].unsqueeze(1).expand(-1, 2, -1)] + ([kl[t]] if listener else []) + [ke[t]]
    return out


def drnn_masks(bm, S, B, seed, a_rec, a_head):
    """every train-mode dropout mask of BiModel in the engine's layout (1/(1-p) folded in).  The head's masks are over
    FORWARD-time rows s * B + b: the reversed half of the emotions gets its mask after it is put back in forward order
    (model.py:1037-1041 applies dropout_rec to emotions_f and to reverse(emotions_b))"""
    cf = bm.dialog_rnn_f.dialogue_cell
    p_rec, p_join, p_hid = float(cf.dropout.p), float(bm.dropout_rec.p), float(bm.dropout.p)
    H, He, Dh2 = cf.D_g, cf.D_e, bm.linear.weight.shape[0]
    return dict(rec=[rec_masks(S, B, H, He, p_rec, seed, a_rec, z, cf.listener_state) for z in range(2)],
                join_f=_keep(S * B, He, p_join, SITE_JOIN_F, seed, a_head).view(S, B, He),
                join_b=_keep(S * B, He, p_join, SITE_JOIN_B, seed, a_head).view(S, B, He),
                hidden=_keep(S * B, Dh2, p_hid, SITE_HIDDEN, seed, a_head).view(S, B, Dh2))


def drnn_head(bm, fusion, qmask, umask, label, class_w=None, masks=None, hidden_pattern=None):
    """BiModel.forward (model.py:1008-1062; gan_ffn_amd/dialogue_rnn.py, fp64 on the CPU) + MaskedNLLLoss from a given
    fusion.  masks: drnn_masks(...) (train mode) or None (eval mode, no dropout); hidden_pattern: the 0/1 ReLU pattern of
    the hidden layer (S, B, 2 D_h) to use instead of the oracle's own.
    -> dict(log_prob, loss, d_fusion, grads={BiModel parameter name: g}, e_f, e_b (reverse time), emotions, pre, hidden)"""
    S, B = fusion.shape[:2]
    um = torch.as_tensor(umask).to(torch.float64)
    qm = torch.as_tensor(qmask).to(torch.float64)
    assert int(um.sum(1).max()) == S, "the longest dialogue must fill the batch (pad_sequence; the engine reverses over S)"
    U = torch.as_tensor(fusion).detach().to(torch.float64).requires_grad_(True)
    cells = (bm.dialog_rnn_f.dialogue_cell, bm.dialog_rnn_r.dialogue_cell)
    saved = [c.dropout for c in cells]
    try:
        for z, c in enumerate(cells):
            c.dropout = MaskSeq(masks["rec"][z]) if masks is not None else torch.nn.Identity()
        e_f, _ = bm.dialog_rnn_f(U, qm)
        e_b, _ = bm.dialog_rnn_r(bm._reverse_seq(U, um), bm._reverse_seq(qm, um))
        if masks is not None:
            assert all(c.dropout.i == len(c.dropout.masks) for c in cells)
    finally:
        for c, d in zip(cells, saved):
            c.dropout = d
    ef, eb = e_f, bm._reverse_seq(e_b, um)
    if masks is not None:
        ef, eb = ef * masks["join_f"], eb * masks["join_b"]
    emotions = torch.cat([ef, eb], dim=-1)
    att, _ = bm.matchatt.general2_all_queries(emotions, um)
    pre = bm.linear(att)
    hidden = pre * (hidden_pattern.to(torch.float64) if hidden_pattern is not None else (pre > 0).to(torch.float64))
    if masks is not None:
        hidden = hidden * masks["hidden"]
    lp = torch.log_softmax(bm.smax_fc(hidden), 2)
    cw = None if class_w is None else torch.as_tensor(class_w, dtype=torch.float64)
    loss = O.masked_nll(lp, torch.as_tensor(label), um, cw)
    names = [n for n, p in bm.named_parameters() if p.requires_grad]
    params = dict(bm.named_parameters())
    g = torch.autograd.grad(loss, [U] + [params[n] for n in names], allow_unused=True)
    grads = {n: (x if x is not None else torch.zeros_like(params[n])) for n, x in zip(names, g[1:])}
    return dict(log_prob=lp.detach(), loss=float(loss.detach()), d_fusion=g[0], grads=grads, e_f=e_f.detach(),
                e_b=e_b.detach(), emotions=emotions.detach(), pre=pre.detach(), hidden=hidden.detach())


def drnn_step(gens, bm, batch, seed, base, train=True, relu_masks=None, hidden_pattern=None, class_w=None):
    """DrnnEngine._step chained end to end from the raw modalities: generators at their offsets of the block starting at
    `base` (train) or without dropout (eval), fusion = their sum, BiModel with the engine's masks (recurrence at base + 6,
    head at base + 7), weighted MaskedNLLLoss, and the gradients of every generator parameter
    -> drnn_head's dict + fusion + gen_grads={k: {name: g}}"""
    S, B = batch["text"].shape[:2]
    outs = generators(gens, batch, seed, gen_adds(base) if train else None, relu_masks)
    fusion = outs["acoustic"] + outs["visual"] + outs["text"]
    masks = drnn_masks(bm, S, B, seed, base + A_REC, base + A_HEAD) if train else None
    head = drnn_head(bm, fusion.detach(), batch["qmask"], batch["umask"], batch["label"], class_w, masks, hidden_pattern)
    return dict(head, fusion=fusion.detach(), gen_grads=generator_grads(gens, outs, head["d_fusion"]))
