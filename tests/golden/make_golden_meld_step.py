"""Generate tests/golden/meld_step.npz by running the REFERENCE's own MELD trainer pieces (CPU, where the reference is):

    python tests/golden/make_golden_meld_step.py

The reference's MELDLSTMModel(600, 300, 600, n_classes, dropout=0.0).train() under its MaskedNLLLoss() (no class weights:
train_MELD.py:154) and optim.Adam(lr=3e-4, weight_decay=1e-4) (train_MELD.py:111-112,155-157), formula weights (formula.py,
unscaled), 4 consecutive steps of train_MELD.py:63-87 on one batch with a ragged prefix mask.  Cases: (S, B) = (7, 3) with 7 and
with 3 classes, (33, 32) with 7 classes.

Stored per case `<tag>/...`: loss (4), log_prob (4, S, B, C), alpha of step 0 (S, B, S: the per-query list stacked), per step
every parameter's gradient `grad<i>/<name>` and after step 4 every parameter `param/<name>`, and `linear_untouched`: whether
linear.weight / linear.bias (no part of the att2 forward: .grad None, skipped by Adam, undecayed) came out bit-identical to
their initial values.  Tensors above SAMPLE_ABOVE elements are sampled with formula.sample_indices(n, SAMPLE_K): 36 tensors x
(4 gradients + 1 parameter set) x 3 cases must fit one file below 1 MB, which the 1024-sample density of make_golden.py
(18 weights x 1024 + 16 biases x 1200 floats per set) does not.

Only data is stored; inputs are regenerated from the formulas below (`case_inputs`), which the tests import too.
Importing this module does not need the reference; running it does.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import formula as F_  # noqa: E402

CASES = {"s7b3c7": (7, 3, 7), "s7b3c3": (7, 3, 3), "s33b32c7": (33, 32, 7)}
N_STEPS = 4
LR, L2 = 3e-4, 1e-4                      # train_MELD.py:111-112
SAMPLE_ABOVE, SAMPLE_K = 256, 256


def case_lengths(S, B):
    """ragged dialogue lengths 2 .. S, one of them S (pad-collate makes the longest dialogue S long)"""
    if (S, B) == (7, 3):
        return [7, 4, 6]
    L = [2 + (b * 7 + 3) % (S - 1) for b in range(B)]
    L[B // 2] = S
    return L


def case_inputs(S, B, C, tag="meld_step"):
    """-> text (S, B, 600) float32 (zero on padding), umask (B, S) float32 prefix mask, label (B, S) int64"""
    L = case_lengths(S, B)
    U = F_.formula_input(tag + ".U", S, B, 600)
    umask = np.zeros((B, S), np.float32)
    for b, n in enumerate(L):
        umask[b, :n] = 1
        U[n:, b] = 0
    s, b = np.arange(S)[None, :], np.arange(B)[:, None]
    label = ((s * 5 + b * 3 + s // 3) % C).astype(np.int64) * umask.astype(np.int64)
    return U, umask, label


def sample(t):
    t = np.asarray(t, np.float32).reshape(-1)
    return t if t.size <= SAMPLE_ABOVE else t[F_.sample_indices(t.size, SAMPLE_K)]


def run_steps(model, loss_function, optimizer, U, umask, label, torch):
    """train_MELD.py:63-87 on one batch, N_STEPS times; -> dict of arrays"""
    out = {"loss": [], "log_prob": []}
    Ut, um, lab = torch.from_numpy(U), torch.from_numpy(umask), torch.from_numpy(label)
    for i in range(N_STEPS):
        optimizer.zero_grad()
        log_prob, alpha, alpha_f, alpha_b = model(Ut, None, um)
        lp_ = log_prob.transpose(0, 1).contiguous().view(-1, log_prob.size()[2])
        loss = loss_function(lp_, lab.view(-1), um)
        loss.backward()
        out["loss"].append(loss.item())
        out["log_prob"].append(log_prob.detach().numpy().copy())
        if i == 0:
            out["alpha"] = torch.stack(alpha, 0).detach().numpy().copy()
        for k, p in model.named_parameters():
            if p.grad is not None:
                out["grad%d/%s" % (i, k)] = sample(p.grad.numpy())
        optimizer.step()
    out["loss"], out["log_prob"] = np.asarray(out["loss"], np.float64), np.stack(out["log_prob"], 0)
    for k, p in model.named_parameters():
        out["param/" + k] = sample(p.detach().numpy())
    return out


def main():
    sys.path.insert(0, "/root/reference")
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    import torch
    import model as ref          # the reference
    torch.set_num_threads(8)
    out = {}
    for tag, (S, B, C) in CASES.items():
        torch.manual_seed(2)
        m = ref.MELDLSTMModel(600, 300, 600, n_classes=C, dropout=0.0).train()
        sd = F_.formula_state_dict(m.state_dict())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        lin0 = (m.linear.weight.detach().clone(), m.linear.bias.detach().clone())
        opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=L2)
        U, umask, label = case_inputs(S, B, C)
        r = run_steps(m, ref.MaskedNLLLoss(), opt, U, umask, label, torch)
        r["linear_untouched"] = np.asarray(torch.equal(m.linear.weight, lin0[0]) and torch.equal(m.linear.bias, lin0[1])
                                           and m.linear.weight.grad is None)
        for k, v in r.items():
            out["%s/%s" % (tag, k)] = v
        print(tag, "losses", r["loss"], "linear untouched", bool(r["linear_untouched"]))
    path = os.path.join(HERE, "meld_step.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
