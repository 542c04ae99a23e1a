"""TEST INFRASTRUCTURE — fp64 restatement of the causal MELD classifier (dialogue_rnn.MELDLSTMModel(causal=True), an extension the
reference does not have) and of one engine.MeldEngine step on it; the product never imports this module.

  * the LSTM is forward-only: lstm_packed_oracle.lstm_direction(reverse=False) per layer (with every length S it is the padded
    run), the layers chained, nn.LSTM's inter-layer dropout over [S x B x H] through oracle.ganffn_oracle's Philox helpers (site
    SITE_LSTM + l, one offset per call) exactly as lstm_packed_oracle.lstm_forward does for two directions;
  * the general2 attention is causal, written out here: query step t attends to memory steps j <= t,
        s_tj = tanh((x_t . m_j) u_j) u_j,   a_tj = e^{s_tj} u_j [j <= t] / sum_{k <= t} e^{s_tk} u_k
    — MatchingAttention.forward(M[:t+1], M[t], umask[:, :t+1]) for every t (model.py:80-88 on a prefix); a row whose allowed keys
    are all masked has weights 0;
  * hardswish(emotions + hardswish(att)), smax_fc, log-softmax, MaskedNLLLoss and the gradients by autograd: meld_step_oracle's.
tests/test_meld_causal_cpu.py pins the layer and the stack to torch.nn.LSTM(bidirectional=False) and the forward to the module
on the CPU."""
import numpy as np
import torch

import lstm_packed_oracle as PO
import meld_step_oracle as MO
from oracle import ganffn_oracle as O

N_LAYERS = MO.N_LAYERS
SITE_LSTM = PO.SITE_LSTM
LSTM_KEYS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def trained_names(n_layers=N_LAYERS):
    """the parameters the causal step trains, in the engine's slab order: the LSTM's 4 L tensors (no _reverse), then the head"""
    return ["lstm.%s_l%d" % (k, l) for l in range(n_layers) for k in LSTM_KEYS] + MO.TRAINED_TAIL


def lstm_layer(x, P, l=0, lengths=None, prefix=""):
    """one forward-only layer: x (S, B, In) -> (S, B, H); lengths None: every dialogue runs all S steps"""
    S, B, _ = x.shape
    lengths = [S] * B if lengths is None else lengths
    return PO.lstm_direction(x, lengths, *[P[prefix + "%s_l%d" % (k, l)] for k in LSTM_KEYS], False)


def lstm_forward(x, P, num_layers, p_drop=0.0, rng=None, prefix="", offsets=None, lengths=None):
    """nn.LSTM(bidirectional=False, num_layers, dropout=p_drop)(x)[0] (packed at `lengths` when given); rng: O.Rng"""
    h = x
    for l in range(num_layers):
        h = lstm_layer(h, P, l, lengths, prefix)
        if l + 1 < num_layers and rng is not None and rng.train and p_drop > 0.0:
            off = offsets[l] if offsets is not None else rng.offset + l
            h = O._drop(h, p_drop, SITE_LSTM + l, rng.at(off))
    return h


def causal_general2(xq, mem, umask):
    """xq, mem (S, B, D), umask (B, S) -> att (S, B, D), alpha (B, S query, S memory), exact zeros at j > t"""
    S = mem.shape[0]
    u = umask.to(mem.dtype).unsqueeze(1)                                      # (B, 1, S memory)
    raw = torch.bmm(xq.transpose(0, 1), mem.permute(1, 2, 0))                 # (B, S query, S memory): x_t . m_j
    s = torch.tanh(raw * u) * u
    allowed = torch.tril(torch.ones(S, S, dtype=mem.dtype)).unsqueeze(0) * u  # [j <= t] u_j
    e = torch.exp(s) * allowed
    den = e.sum(2, keepdim=True)
    alpha = torch.where(den > 0, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
    return torch.bmm(alpha, mem.transpose(0, 1)).transpose(0, 1), alpha


def forward(P, text, umask, label=None, p_drop=0.0, seed=0, offsets=None, train=False, class_w=None, lengths=None):
    """P: name -> fp64 tensor.  -> (loss or None, log_prob (S, B, C), alpha (B, S, S))"""
    rng = O.Rng(seed, offsets[0] if offsets else 0, train)
    em = lstm_forward(text, P, N_LAYERS, p_drop, rng, prefix="lstm.", offsets=offsets, lengths=lengths)
    xq = em @ P["matchatt.transform.weight"].T + P["matchatt.transform.bias"]
    att, alpha = causal_general2(xq, em, umask)
    hidden = MO.hardswish(em + MO.hardswish(att))
    log_prob = torch.log_softmax(hidden @ P["smax_fc.weight"].T + P["smax_fc.bias"], 2)
    if label is None:
        return None, log_prob, alpha
    lp = log_prob.transpose(0, 1).reshape(-1, log_prob.shape[2])
    y, m = label.reshape(-1), umask.reshape(-1).to(lp.dtype)
    w = class_w[y] if class_w is not None else torch.ones_like(m)
    loss = -(w * m * lp.gather(1, y.unsqueeze(1))[:, 0]).sum() / (w * m).sum()
    return loss, log_prob, alpha


def step(P, text, umask, label, p_drop=0.0, seed=0, offsets=None, train=True, class_w=None, lengths=None):
    """one step's forward and gradients.  P: name -> array-like (any float dtype); -> dict(loss, log_prob, alpha, grads)"""
    trained = set(trained_names())
    Pd = {k: torch.as_tensor(np.asarray(v, np.float64)).clone().requires_grad_(k in trained) for k, v in P.items()}
    t = torch.as_tensor(np.asarray(text, np.float64))
    um, lab = torch.as_tensor(np.asarray(umask, np.float64)), torch.as_tensor(np.asarray(label, np.int64))
    cw = torch.as_tensor(np.asarray(class_w, np.float64)) if class_w is not None else None
    loss, log_prob, alpha = forward(Pd, t, um, lab, p_drop, seed, offsets, train, cw, lengths)
    names = [k for k in trained_names() if k in Pd]
    grads = torch.autograd.grad(loss, [Pd[k] for k in names])
    return dict(loss=float(loss.detach()), log_prob=log_prob.detach().numpy(), alpha=alpha.detach().numpy(),
                grads={k: g.numpy() for k, g in zip(names, grads)})
