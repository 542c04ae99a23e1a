"""Generate tests/golden/dialogue_rnn_parties.npz by running the REFERENCE itself (on the CPU).

    python tests/golden/make_golden_parties.py        # needs the reference sources, located as make_golden.py does

The reference's BiModel (model.py:975-1062, DialogueRNNCell :861-926 with qmask [S x B x P]), eval mode, formula weights,
dims make_golden.DRNN_DIMS (make_golden.py is imported, not edited), on multi-party batches in closed form (party_qmask):
  <case>/P<P>/*   the ragged (7, 3) batch of make_golden.drnn_inputs() with P parties — party P - 1 never speaks (P >= 3),
                  dialogue 1 has a single speaker, padded steps have zero rows: log-probabilities, the attention maps, dU
                  and every parameter gradient (sampled above 4096 elements), qmask and umask;
  big_parties/*   summaries at a MELD-like size, (33, 32) with P = 9, general attention without listener state (and its
                  qmask / umask).
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

CASES = {"general": dict(context_attention="general", listener_state=False),
         "general_listener": dict(context_attention="general", listener_state=True),
         "concat_listener": dict(context_attention="concat", listener_state=True),
         "simple": dict(context_attention="simple", listener_state=False)}
RUNS = [("general", 1), ("general", 9), ("general_listener", 3), ("concat_listener", 9), ("simple", 3)]    # (file < 1 MB)
BIG_S, BIG_B, BIG_P = 33, 32, 9


def party_qmask(umask, P):
    """one-hot speakers [S x B x P] in closed form: speaker (3t + 5b + t // 2) mod (P - 1) for P >= 3 (party P - 1 never
    speaks), mod P below; dialogue 1 is spoken by one party only; zero rows on padding"""
    B, S = umask.shape
    n = P - 1 if P >= 3 else P
    t, b = np.arange(S)[:, None], np.arange(B)[None, :]
    spk = (3 * t + 5 * b + t // 2) % n
    if B > 1:
        spk[:, 1] = 1 % n
    return np.eye(P, dtype=np.float32)[spk] * umask.T[:, :, None]


def big_inputs():
    """ragged (33, 32) batch: dialogue 0 full length, the others 5 .. 33 utterances; U = formula_input('drnn.partiesU')"""
    S, B = BIG_S, BIG_B
    lens = [S] + [5 + (b * 11) % 29 for b in range(1, B)]
    umask = np.zeros((B, S), np.float32)
    for b, L in enumerate(lens):
        umask[b, :L] = 1
    U = F_.formula_input("drnn.partiesU", S, B, 100) * umask.T[:, :, None]
    return U, party_qmask(umask, BIG_P), umask


def _model(case):
    torch.manual_seed(0)
    m = ref.BiModel(**MG.DRNN_DIMS, **CASES[case]).eval()
    sd = F_.formula_state_dict({k: v for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def small():
    out = {}
    U, _, umask = MG.drnn_inputs()
    for case, P in RUNS:
        tag = "%s/P%d" % (case, P)
        qmask = party_qmask(umask, P)
        m = _model(case)
        Ut = torch.from_numpy(U).requires_grad_(True)
        lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask), torch.from_numpy(umask))
        gy = torch.from_numpy(F_.formula_input("drnn.grad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
        (lp * gy).sum().backward()
        out["%s/qmask" % tag], out["%s/umask" % tag] = qmask, umask
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
    U, qmask, umask = big_inputs()
    m = _model("general")
    Ut = torch.from_numpy(U).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask), torch.from_numpy(umask))
    gy = torch.from_numpy(F_.formula_input("drnn.partiesgrad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy).sum().backward()
    out["big_parties/qmask"], out["big_parties/umask"] = qmask, umask
    MG.put(out, "big_parties/log_prob", lp)
    MG.put(out, "big_parties/alpha", torch.stack(alpha, 0))
    MG.put(out, "big_parties/alpha_f_last", alpha_f[-1])
    MG.put(out, "big_parties/alpha_b_last", alpha_b[-1])
    MG.put(out, "big_parties/dU", Ut.grad)
    for k, p_ in m.named_parameters():
        if p_.grad is not None:
            MG.put(out, "big_parties/grad/" + k, p_.grad)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "dialogue_rnn_parties.npz"), **small(), **big())
    print("written", os.path.join(HERE, "dialogue_rnn_parties.npz"))
