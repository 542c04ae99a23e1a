"""Generate tests/golden/dialogue_rnn_context*.npz by running the REFERENCE itself (on the CPU).

    python tests/golden/make_golden_context.py         # needs the reference sources, located as make_golden.py does

The reference's BiModel with the other context attention types of train_IEMOCAP_DialogueRNN.py --attention (:586; D_a = 100,
:641), eval mode, formula weights, on the inputs of make_golden.py (imported, not edited):
  <case>/*      ragged (7, 3) batch of drnn_inputs(): log-probabilities, the attention maps, dU and every parameter gradient
                (sampled above 4096 elements) — cases general2, concat, dot (D_g = D_p = 100: the reference asserts
                D_m == D_g), general2_listener, concat_listener;
  big_<case>/*  summaries at (94, 30) (drnn_big_inputs()) for general2 and concat, like make_golden.dialogue_rnn_big().
Small cases go to dialogue_rnn_context.npz, the summaries to dialogue_rnn_context_big.npz.
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

CASES = {
    "general2": dict(context_attention="general2"),
    "concat": dict(context_attention="concat"),
    "dot": dict(context_attention="dot", D_g=100, D_p=100),
    "general2_listener": dict(context_attention="general2", listener_state=True),
    "concat_listener": dict(context_attention="concat", listener_state=True),
}
BIG_CASES = ("general2", "concat")


def dims(case):
    d = dict(MG.DRNN_DIMS)
    d.update(CASES[case])
    return d


def _model(case):
    torch.manual_seed(0)
    m = ref.BiModel(**dims(case)).eval()
    sd = F_.formula_state_dict({k: v for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def small(tag):
    out = {}
    U, qmask, umask = MG.drnn_inputs()
    m = _model(tag)
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


def big(case):
    out, tag = {}, "big_" + case
    U, qmask, umask = MG.drnn_big_inputs()
    m = _model(case)
    Ut = torch.from_numpy(U).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask), torch.from_numpy(umask))
    gy = torch.from_numpy(F_.formula_input("drnn.biggrad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy).sum().backward()
    MG.put(out, tag + "/log_prob", lp)
    MG.put(out, tag + "/alpha", torch.stack(alpha, 0))
    MG.put(out, tag + "/alpha_f_last", alpha_f[-1])
    MG.put(out, tag + "/alpha_b_last", alpha_b[-1])
    MG.put(out, tag + "/dU", Ut.grad)
    for k, p_ in m.named_parameters():
        if p_.grad is not None:
            MG.put(out, tag + "/grad/" + k, p_.grad)
    return out


if __name__ == "__main__":
    s, b = {}, {}
    for c in CASES:
        s.update(small(c))
    for c in BIG_CASES:
        b.update(big(c))
    np.savez_compressed(os.path.join(HERE, "dialogue_rnn_context.npz"), **s)
    np.savez_compressed(os.path.join(HERE, "dialogue_rnn_context_big.npz"), **b)
    print("written", os.path.join(HERE, "dialogue_rnn_context.npz"), os.path.join(HERE, "dialogue_rnn_context_big.npz"))
