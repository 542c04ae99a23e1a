"""Generate tests/golden/recurrence_batch.npz by running the REFERENCE itself (on the CPU) on batches above 32 dialogues:

    python tests/golden/make_golden_batch.py        # needs the reference sources, located as make_golden.py does

The batch sizes a reference user reaches with --batch-size (train_IEMOCAP_DialogueRNN.py:580, train_MELD.py:114; BASELINE.json
configs[3] names 256): 33 and 100 are neither multiples of 32 nor of 16, 64 and 256 are whole tiles of the HIP recurrences.

  drnn/<tag>/*   the reference's BiModel (model.py:975-1062), eval mode, formula weights, dims make_golden.DRNN_DIMS, under its
                 MaskedNLLLoss with the class weights of train_IEMOCAP_DialogueRNN.py:738: the loss, and summaries (fixed-index
                 samples + sum + l2 + max-abs) of the log-probabilities, dU and every parameter gradient.  Cases DRNN_CASES:
                 general attention at (20, 33, P = 2) and (94, 64, 2), listener state + concat at (33, 100, 9), general at
                 (33, 256, 9).
  meld/<tag>/*   the reference's MELDLSTMModel(600, 300, 600, 7, dropout = 0).train() under MaskedNLLLoss() and
                 optim.Adam(lr = 3e-4, weight_decay = 1e-4) (train_MELD.py:111-112,154-157), formula weights, N_STEPS = 2 steps
                 on one batch: the losses, log-probability summaries per step and every parameter after the last step (sampled).
                 Cases MELD_CASES: (12, 33), (33, 64), (33, 100).

Ragged lengths in closed form (lengths): dialogue 0 full length, dialogue 2 of length 1.  Only data is stored; the inputs are
regenerated from the formulas below, which the tests import too.  Importing this module does not need the reference; running it
does.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import formula as F_  # noqa: E402

DRNN_MODELS = {"general": dict(context_attention="general", listener_state=False),
               "concat_listener": dict(context_attention="concat", listener_state=True)}
# tag -> (model, S, B, P)
DRNN_CASES = {"general_s20b33p2": ("general", 20, 33, 2), "general_s94b64p2": ("general", 94, 64, 2),
              "concat_listener_s33b100p9": ("concat_listener", 33, 100, 9), "general_s33b256p9": ("general", 33, 256, 9)}
CLASS_W = [1.2, 0.60072, 0.38066, 0.94019, 0.67924, 0.34332]            # train_IEMOCAP_DialogueRNN.py:738
MELD_CASES = {"s12b33": (12, 33, 7), "s33b64": (33, 64, 7), "s33b100": (33, 100, 7)}
N_STEPS = 2
LR, L2 = 3e-4, 1e-4                      # train_MELD.py:111-112
SAMPLE_ABOVE, SAMPLE_K = 256, 256        # final MELD parameters (as make_golden_meld_step.py)


def lengths(S, B):
    """ragged dialogue lengths in closed form: dialogue 0 is S long, dialogue 2 one utterance, the others 2 .. S"""
    L = [2 + (b * 7 + 3) % (S - 1) for b in range(B)]
    L[0], L[2] = S, 1
    return L


def umask_of(S, B):
    um = np.zeros((B, S), np.float32)
    for b, n in enumerate(lengths(S, B)):
        um[b, :n] = 1
    return um


def party_qmask(umask, P):
    """one-hot speakers [S x B x P] (make_golden_parties.party_qmask): speaker (3t + 5b + t // 2) mod (P - 1) for P >= 3 (party
    P - 1 never speaks), mod P below; dialogue 1 is spoken by one party only; zero rows on padding"""
    B, S = umask.shape
    n = P - 1 if P >= 3 else P
    t, b = np.arange(S)[:, None], np.arange(B)[None, :]
    spk = (3 * t + 5 * b + t // 2) % n
    spk[:, 1] = 1 % n
    return np.eye(P, dtype=np.float32)[spk] * umask.T[:, :, None]


def drnn_inputs(tag):
    """-> U (S, B, 100) float32 zero on padding, qmask (S, B, P), umask (B, S), label (B, S) int64"""
    _, S, B, P = DRNN_CASES[tag]
    umask = umask_of(S, B)
    U = F_.formula_input("batch.U." + tag, S, B, 100) * umask.T[:, :, None]
    s, b = np.arange(S)[None, :], np.arange(B)[:, None]
    label = ((s * 5 + b * 3 + s // 3) % 6).astype(np.int64) * umask.astype(np.int64)
    return U.astype(np.float32), party_qmask(umask, P), umask, label


def meld_inputs(tag):
    """-> text (S, B, 600) float32 zero on padding, umask (B, S), label (B, S) int64"""
    S, B, C = MELD_CASES[tag]
    umask = umask_of(S, B)
    U = F_.formula_input("batch.meldU." + tag, S, B, 600) * umask.T[:, :, None]
    s, b = np.arange(S)[None, :], np.arange(B)[:, None]
    label = ((s * 5 + b * 3 + s // 3) % C).astype(np.int64) * umask.astype(np.int64)
    return U.astype(np.float32), umask, label


def sample(t):
    t = np.asarray(t, np.float32).reshape(-1)
    return t if t.size <= SAMPLE_ABOVE else t[F_.sample_indices(t.size, SAMPLE_K)]


def put(d, prefix, t):
    t = np.asarray(t, np.float32)
    for k, v in F_.summarize(t).items():
        d[prefix + "/" + k] = v
    d[prefix + "/maxabs"] = np.float64(np.abs(t).max())


def drnn_case(ref, MG, torch, tag):
    name, S, B, P = DRNN_CASES[tag]
    torch.manual_seed(0)
    m = ref.BiModel(**MG.DRNN_DIMS, **DRNN_MODELS[name]).eval()
    sd = F_.formula_state_dict({k: v for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    U, qmask, umask, label = drnn_inputs(tag)
    Ut = torch.from_numpy(U).requires_grad_(True)
    um = torch.from_numpy(umask)
    lp = m(Ut, torch.from_numpy(qmask), um)[0]
    loss = ref.MaskedNLLLoss(torch.tensor(CLASS_W))(lp.transpose(0, 1).contiguous().view(-1, lp.size(2)), torch.from_numpy(label).view(-1), um)
    loss.backward()
    out = {"loss": np.float64(loss.item())}
    put(out, "log_prob", lp.detach().numpy())
    put(out, "dU", Ut.grad.numpy())
    for k, p_ in m.named_parameters():
        if p_.grad is not None:
            put(out, "grad/" + k, p_.grad.numpy())
    return out


def meld_case(ref, torch, tag):
    S, B, C = MELD_CASES[tag]
    torch.manual_seed(2)
    m = ref.MELDLSTMModel(600, 300, 600, n_classes=C, dropout=0.0).train()
    sd = F_.formula_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=L2)
    loss_function = ref.MaskedNLLLoss()
    U, umask, label = meld_inputs(tag)
    Ut, um, lab = torch.from_numpy(U), torch.from_numpy(umask), torch.from_numpy(label)
    out, losses = {}, []
    for i in range(N_STEPS):                 # train_MELD.py:63-87 on one batch
        opt.zero_grad()
        log_prob = m(Ut, None, um)[0]
        loss = loss_function(log_prob.transpose(0, 1).contiguous().view(-1, log_prob.size()[2]), lab.view(-1), um)
        loss.backward()
        losses.append(loss.item())
        put(out, "log_prob%d" % i, log_prob.detach().numpy())
        opt.step()
    out["loss"] = np.asarray(losses, np.float64)
    for k, p in m.named_parameters():
        out["param/" + k] = sample(p.detach().numpy())
    return out


def main():
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    import torch
    import make_golden as MG             # puts the reference on sys.path
    from make_golden import ref
    torch.set_num_threads(8)
    out = {}
    for tag in DRNN_CASES:
        for k, v in drnn_case(ref, MG, torch, tag).items():
            out["drnn/%s/%s" % (tag, k)] = v
        print("drnn", tag, "loss", float(out["drnn/%s/loss" % tag]), flush=True)
    for tag in MELD_CASES:
        for k, v in meld_case(ref, torch, tag).items():
            out["meld/%s/%s" % (tag, k)] = v
        print("meld", tag, "losses", out["meld/%s/loss" % tag], flush=True)
    path = os.path.join(HERE, "recurrence_batch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
