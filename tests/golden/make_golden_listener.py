"""Generate tests/golden/dialogue_rnn_listener.npz by running the REFERENCE itself (on the CPU).

    python tests/golden/make_golden_listener.py        # needs the reference sources, located as make_golden.py does

The reference's BiModel with context_attention = "general" and listener_state = True (the configuration of
train_IEMOCAP_DialogueRNN.py --active-listener, :594,716), eval mode, formula weights, on the inputs of make_golden.py
(imported, not edited):
  general_listener/*  ragged (7, 3) batch of drnn_inputs(): log-probabilities, the attention maps, dU and every parameter
                      gradient (sampled above 4096 elements), l_cell included;
  big_listener/*      summaries at (94, 30) (drnn_big_inputs()), like make_golden.dialogue_rnn_big().
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import formula as F_  # noqa: E402
import make_golden as MG  # noqa: E402  (puts the reference on sys.path)
from make_golden import ref  # noqa: E402

CASE = dict(context_attention="general", listener_state=True)


def _model():
    torch.manual_seed(0)
    m = ref.BiModel(**MG.DRNN_DIMS, **CASE).eval()
    sd = F_.formula_state_dict({k: v for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def small():
    out, tag = {}, "general_listener"
    U, qmask, umask = MG.drnn_inputs()
    m = _model()
    Ut = torch.from_numpy(U).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask), torch.from_numpy(umask))
    gy = torch.from_numpy(F_.formula_input("drnn.grad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy).sum().backward()
    out["%s/log_prob" % tag] = lp.detach().numpy()
    out["%s/alpha" % tag] = torch.stack(alpha, 0).detach().numpy()
    for name, al in (("alpha_f", alpha_f), ("alpha_b", alpha_b)):
        for t, a in enumerate(al):
            out["%s/%s/%d" % (tag, name, t)] = a.detach().numpy()
        out["%s/%s/n" % (tag, name)] = np.array(len(al))
    out["%s/dU" % tag] = Ut.grad.numpy()
    for k, p_ in m.named_parameters():
        if p_.grad is not None:
            out["%s/grad/%s" % (tag, k)] = p_.grad.numpy() if p_.grad.numel() <= 4096 else \
                p_.grad.reshape(-1)[F_.sample_indices(p_.grad.numel())].numpy()
    return out


def big():
    out = {}
    U, qmask, umask = MG.drnn_big_inputs()
    m = _model()
    Ut = torch.from_numpy(U).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask), torch.from_numpy(umask))
    gy = torch.from_numpy(F_.formula_input("drnn.biggrad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy).sum().backward()
    MG.put(out, "big_listener/log_prob", lp)
    MG.put(out, "big_listener/alpha", torch.stack(alpha, 0))
    MG.put(out, "big_listener/alpha_f_last", alpha_f[-1])
    MG.put(out, "big_listener/alpha_b_last", alpha_b[-1])
    MG.put(out, "big_listener/dU", Ut.grad)
    for k, p_ in m.named_parameters():
        if p_.grad is not None:
            MG.put(out, "big_listener/grad/" + k, p_.grad)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "dialogue_rnn_listener.npz"), **small(), **big())
    print("written", os.path.join(HERE, "dialogue_rnn_listener.npz"))
