"""fp64 restatement of the causal DialogueRNN classifier head (gan_ffn_amd/dialogue_rnn.py UniModel), written as the loop the
definition is: one forward DialogueRNN, dropout_rec on its emotions, then for every step t ONE MatchingAttention.forward call on
the TRUNCATED sequence — memory emotions[:t+1], candidate emotions[t], mask umask[:, :t+1] — so that step t cannot see a later
step by construction; linear + ReLU + dropout, class log-probabilities, weighted MaskedNLLLoss.  Nothing here calls
general2_all_queries(causal=True) or a HIP kernel: it is what they are compared with.

Dropout is given as explicit masks in the style of engine_oracle.drnn_head (1/(1-p) folded in), drawn from the engine's Philox
contract: the recurrence's sites of direction 0 at the step's offset b + 6, the join (SITE_JOIN_F: dropout_rec on e_f) and the
hidden layer (SITE_HIDDEN) at b + 7."""
import torch

import engine_oracle as EO
from oracle import ganffn_oracle as O


def uni_masks(um, S, B, seed, a_rec, a_head):
    """every train-mode dropout mask of UniModel in DrnnEngine's layout: rows s * B + b in forward time"""
    cf = um.dialog_rnn_f.dialogue_cell
    p_rec, p_join, p_hid = float(cf.dropout.p), float(um.dropout_rec.p), float(um.dropout.p)
    H, He, Dh = cf.D_g, cf.D_e, um.linear.weight.shape[0]
    return dict(rec=EO.rec_masks(S, B, H, He, p_rec, seed, a_rec, 0, cf.listener_state),
                join_f=EO._keep(S * B, He, p_join, EO.SITE_JOIN_F, seed, a_head).view(S, B, He),
                hidden=EO._keep(S * B, Dh, p_hid, EO.SITE_HIDDEN, seed, a_head).view(S, B, Dh))


def causal_general2(matchatt, M, um):
    """[matchatt(M[:t+1], M[t], um[:, :t+1]) for t]: pooled (S, B, D), alpha (B, S, S) zero-filled above the diagonal"""
    S, B = M.shape[:2]
    att, alpha = [], M.new_zeros(B, S, S)
    for t in range(S):
        a_t, w_t = matchatt(M[:t + 1], M[t], um[:, :t + 1])
        att.append(a_t)
        alpha[:, t, :t + 1] = w_t[:, 0, :].detach()
    return torch.stack(att, 0), alpha


def uni_head(um, fusion, qmask, umask, label=None, class_w=None, masks=None, hidden_pattern=None):
    """UniModel.forward (fp64 on the CPU, the per-step torch cell) + MaskedNLLLoss from a given fusion.  masks: uni_masks(...)
    (train mode) or None (eval mode, no dropout); hidden_pattern: the 0/1 ReLU pattern of the hidden layer (S, B, D_h) to use
    instead of the oracle's own; label None: no loss, no gradients.
    -> dict(log_prob, alpha, emotions, pre, hidden [, loss, d_fusion, grads={UniModel parameter name: g}])"""
    mask = torch.as_tensor(umask).to(torch.float64)
    qm = torch.as_tensor(qmask).to(torch.float64)
    U = torch.as_tensor(fusion).detach().to(torch.float64).requires_grad_(True)
    cell = um.dialog_rnn_f.dialogue_cell
    saved = cell.dropout
    try:
        cell.dropout = EO.MaskSeq(masks["rec"]) if masks is not None else torch.nn.Identity()
        e_f, _ = um.dialog_rnn_f(U, qm)
        if masks is not None:
            assert cell.dropout.i == len(cell.dropout.masks)
    finally:
        cell.dropout = saved
    emotions = e_f * masks["join_f"] if masks is not None else e_f
    att, alpha = causal_general2(um.matchatt, emotions, mask)
    pre = um.linear(att)
    hidden = pre * (hidden_pattern.to(torch.float64) if hidden_pattern is not None else (pre > 0).to(torch.float64))
    if masks is not None:
        hidden = hidden * masks["hidden"]
    lp = torch.log_softmax(um.smax_fc(hidden), 2)
    res = dict(log_prob=lp.detach(), alpha=alpha, emotions=emotions.detach(), pre=pre.detach(), hidden=hidden.detach())
    if label is None:
        return res
    cw = None if class_w is None else torch.as_tensor(class_w, dtype=torch.float64)
    loss = O.masked_nll(lp, torch.as_tensor(label), mask, cw)
    names = [n for n, p in um.named_parameters() if p.requires_grad]
    params = dict(um.named_parameters())
    g = torch.autograd.grad(loss, [U] + [params[n] for n in names], allow_unused=True)
    grads = {n: (x if x is not None else torch.zeros_like(params[n])) for n, x in zip(names, g[1:])}
    return dict(res, loss=float(loss.detach()), d_fusion=g[0], grads=grads)


def uni_step(gens, um, batch, seed, base, train=True, relu_masks=None, hidden_pattern=None, class_w=None):
    """DrnnEngine._step on a causal net chained end to end from the raw modalities (call it under causal_oracle's
    causal_attention context, which makes the generators causal): generators at their offsets of the block starting at `base`,
    fusion = their sum, UniModel with the engine's masks -> uni_head's dict + fusion + gen_grads"""
    S, B = batch["text"].shape[:2]
    outs = EO.generators(gens, batch, seed, EO.gen_adds(base) if train else None, relu_masks)
    fusion = outs["acoustic"] + outs["visual"] + outs["text"]
    masks = uni_masks(um, S, B, seed, base + EO.A_REC, base + EO.A_HEAD) if train else None
    head = uni_head(um, fusion.detach(), batch["qmask"], batch["umask"], batch["label"], class_w, masks, hidden_pattern)
    return dict(head, fusion=fusion.detach(), gen_grads=EO.generator_grads(gens, outs, head["d_fusion"]))
