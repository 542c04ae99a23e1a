"""fp64 restatement of one engine.MeldEngine step (train_MELD.py:63-87 on MELDLSTMModel's att2 branch, model.py:546-561), with
the engine's own Philox masks: the LSTM stack of oracle/lstm_oracle.py (inter-layer dropout sites SITE_LSTM + l at the offsets
the engine drew: base + l), matchatt.transform, the masked general2 attention weights of gan_ffn_amd/dialogue_rnn.general2_scores
(device-agnostic torch, pinned to the reference by tests/test_dialogue_rnn_cpu.py), hardswish(emotions + hardswish(att)),
smax_fc, log-softmax, MaskedNLLLoss (model.py:62-81; optional class weights), gradients by autograd in fp64, and L2-coupled
Adam (engine_oracle.adam_wd).  tests/test_meld_step_cpu.py pins it to the reference-made fixture (eval arithmetic)."""
import numpy as np
import torch

import engine_oracle as EO
from oracle import ganffn_oracle as O
from oracle import lstm_oracle as LO

N_LAYERS = 4
TRAINED_TAIL = ["matchatt.transform.weight", "matchatt.transform.bias", "smax_fc.weight", "smax_fc.bias"]


def trained_names(n_layers=N_LAYERS):
    """the parameters the step trains, in the engine's slab order (nn.LSTM's named_parameters order, then the head)"""
    out = []
    for l in range(n_layers):
        for suf in ("", "_reverse"):
            out += ["lstm.%s_l%d%s" % (k, l, suf) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return out + TRAINED_TAIL


def hardswish(x):
    return x * torch.clamp(x + 3.0, 0.0, 6.0) / 6.0


def forward(P, text, umask, label, p_drop=0.0, seed=0, offsets=None, train=False, class_w=None):
    """P: name -> fp64 tensor.  -> (loss, log_prob (S, B, C), alpha (B, S, S))"""
    from gan_ffn_amd.dialogue_rnn import general2_scores
    rng = O.Rng(seed, offsets[0] if offsets else 0, train)
    em = LO.lstm_forward(text, P, N_LAYERS, p_drop, rng, prefix="lstm.", offsets=offsets)
    xq = em @ P["matchatt.transform.weight"].T + P["matchatt.transform.bias"]
    alpha = general2_scores(xq.transpose(0, 1), em, umask)                      # (B, S query, S memory)
    att = torch.bmm(alpha, em.transpose(0, 1)).transpose(0, 1)
    hidden = hardswish(em + hardswish(att))
    log_prob = torch.log_softmax(hidden @ P["smax_fc.weight"].T + P["smax_fc.bias"], 2)
    lp = log_prob.transpose(0, 1).reshape(-1, log_prob.shape[2])
    y, m = label.reshape(-1), umask.reshape(-1)
    w = class_w[y] if class_w is not None else torch.ones_like(m)
    loss = -(w * m * lp.gather(1, y.unsqueeze(1))[:, 0]).sum() / (w * m).sum()
    return loss, log_prob, alpha


def step(P, text, umask, label, p_drop=0.0, seed=0, offsets=None, train=True, class_w=None):
    """one step's forward and gradients.  P: name -> array-like (any float dtype); -> dict(loss, log_prob, alpha, grads)"""
    Pd = {k: torch.as_tensor(np.asarray(v, np.float64)).clone().requires_grad_(k in set(trained_names())) for k, v in P.items()}
    t = torch.as_tensor(np.asarray(text, np.float64))
    um, lab = torch.as_tensor(np.asarray(umask, np.float64)), torch.as_tensor(np.asarray(label, np.int64))
    cw = torch.as_tensor(np.asarray(class_w, np.float64)) if class_w is not None else None
    loss, log_prob, alpha = forward(Pd, t, um, lab, p_drop, seed, offsets, train, cw)
    names = [k for k in trained_names() if k in Pd]
    grads = torch.autograd.grad(loss, [Pd[k] for k in names])
    return dict(loss=float(loss.detach()), log_prob=log_prob.detach().numpy(), alpha=alpha.detach().numpy(),
                grads={k: g.numpy() for k, g in zip(names, grads)})


def adam_steps(P, text, umask, label, n_steps, lr, wd, betas=(0.9, 0.999)):
    """n_steps consecutive eval-arithmetic (dropout 0) train steps with L2-coupled Adam on the trained parameters; every other
    entry of P (linear.*) is left alone, as torch.optim.Adam leaves parameters without a gradient.
    -> (list of step() results, final P as fp64 arrays)"""
    P = {k: np.asarray(v, np.float64).copy() for k, v in P.items()}
    M = {k: np.zeros_like(P[k]) for k in trained_names()}
    V = {k: np.zeros_like(P[k]) for k in trained_names()}
    outs = []
    for t in range(1, n_steps + 1):
        r = step(P, text, umask, label, 0.0, train=False)
        outs.append(r)
        for k, g in r["grads"].items():
            P[k], M[k], V[k] = EO.adam_wd(P[k], g, M[k], V[k], t, lr, betas[0], betas[1], wd)
    return outs, P
