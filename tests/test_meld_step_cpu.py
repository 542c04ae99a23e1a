"""The MELD train step on the CPU: tests/golden/meld_step.npz (made by the REFERENCE's MELDLSTMModel, MaskedNLLLoss and
optim.Adam: tests/golden/make_golden_meld_step.py) against (a) the mirror's MELDLSTMModel under the stock loss and optimizer —
pins the fixture to the mirror —, (b) the fp64 restatement of the whole step that the GPU tests use as their oracle
(tests/meld_step_oracle.py); and the data side of engine.MeldEngine: write_synthetic_meld_pickle -> MELDDataset ->
get_MELD_loaders -> to_meld_batch.

Bounds.  Step 0: log_prob and alpha 5e-5, gradients 5e-4 of the tensor's scale — what tests/test_dialogue_rnn_cpu.check_meld
holds the same model to against the same reference.  Steps 1-3: the reference's own fp32 and fp64 runs stay within 2.3e-7 of each
other over all four steps on these (unscaled) formula weights, i.e. the trajectory is not chaotic; a path that differs from the
reference by fp32 summation order only (the mirror batches the attention queries) or by precision only (the fp64 oracle) is held
to the step-0 bounds throughout, the loss to 2e-5 relative.  Final parameters: an Adam update is lr * m_hat / (sqrt(v_hat) + eps),
at most ~lr per step whatever the gradient, so two paths can differ by at most 2 lr per step on an element whose (near-zero)
gradient changes sign: |delta| <= 2 lr N_STEPS; the parameters' distance is printed."""
import numpy as np
import pytest
import torch

import formula as F_
import make_golden_meld_step as MG
from util import golden


def close(a, ref, rtol, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(a - ref).max()
    assert a.shape == ref.shape and err <= rtol * scale, "%s: max err %.3e vs scale %.3e" % (what, err, scale)
    return err / scale


def mirror(C, dev="cpu", dropout=0.0):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(2)
    m = DR.MELDLSTMModel(600, 300, 600, n_classes=C, dropout=dropout)
    sd = F_.formula_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).train()


def check_case(g, tag, res, final, rt_lp=5e-5, rt_g=5e-4):
    """res: per step dicts(loss, log_prob (S,B,C), alpha (query, B, memory) for step 0, grads name -> array); final: name -> array"""
    worst = 0.0
    for i, r in enumerate(res):
        assert abs(r["loss"] - g[tag + "/loss"][i]) <= 2e-5 * abs(g[tag + "/loss"][i]), (tag, i, r["loss"], g[tag + "/loss"][i])
        close(r["log_prob"], g[tag + "/log_prob"][i], rt_lp, "%s step %d log_prob" % (tag, i))
        if i == 0:
            close(r["alpha"], g[tag + "/alpha"], rt_lp, tag + " alpha")
        for k, gr in r["grads"].items():
            worst = max(worst, close(MG.sample(gr), g["%s/grad%d/%s" % (tag, i, k)], rt_g, "%s step %d grad %s" % (tag, i, k)))
    dp = 0.0
    for k, p in final.items():
        ref = g["%s/param/%s" % (tag, k)]
        d = float(np.abs(MG.sample(p).astype(np.float64) - ref).max())
        assert d <= 2 * MG.LR * MG.N_STEPS, (tag, k, d)
        dp = max(dp, d)
    print("%s: worst gradient distance %.2e of scale, worst final-parameter distance %.2e" % (tag, worst, dp))
    assert bool(g[tag + "/linear_untouched"])


@pytest.mark.parametrize("tag", list(MG.CASES))
def test_mirror_under_stock_loss_and_adam_reproduces_the_reference_fixture(tag):
    from gan_ffn_amd import model as M
    g = golden("meld_step")
    S, B, C = MG.CASES[tag]
    m = mirror(C)
    lin0 = (m.linear.weight.detach().clone(), m.linear.bias.detach().clone())
    opt = torch.optim.Adam(m.parameters(), lr=MG.LR, weight_decay=MG.L2)
    U, umask, label = MG.case_inputs(S, B, C)
    Ut, um, lab = torch.from_numpy(U), torch.from_numpy(umask), torch.from_numpy(label)
    loss_fn = M.MaskedNLLLoss()
    res = []
    for i in range(MG.N_STEPS):
        opt.zero_grad()
        lp, alpha, _, _ = m(Ut, None, um)
        loss = loss_fn(lp.transpose(0, 1).contiguous().view(-1, C), lab.view(-1), um)
        loss.backward()
        res.append(dict(loss=loss.item(), log_prob=lp.detach().numpy().copy(), alpha=torch.stack(alpha, 0).detach().numpy(),
                        grads={k: p.grad.numpy().copy() for k, p in m.named_parameters() if p.grad is not None}))
        opt.step()
    assert set(res[0]["grads"]) == {k for k, _ in m.named_parameters() if not k.startswith("linear.")}
    check_case(g, tag, res, {k: p.detach().numpy() for k, p in m.named_parameters()})
    assert torch.equal(m.linear.weight, lin0[0]) and torch.equal(m.linear.bias, lin0[1]) and m.linear.weight.grad is None


@pytest.mark.parametrize("tag", list(MG.CASES))
def test_fp64_step_oracle_reproduces_the_reference_fixture(tag):
    import meld_step_oracle as MO
    g = golden("meld_step")
    S, B, C = MG.CASES[tag]
    m = mirror(C)
    P = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    assert MO.trained_names() == [k for k, _ in m.named_parameters() if not k.startswith("linear.")][:32] + MO.TRAINED_TAIL
    U, umask, label = MG.case_inputs(S, B, C)
    outs, final = MO.adam_steps(P, U, umask, label, MG.N_STEPS, MG.LR, MG.L2)
    res = [dict(loss=r["loss"], log_prob=r["log_prob"], alpha=r["alpha"].transpose(1, 0, 2), grads=r["grads"]) for r in outs]
    check_case(g, tag, res, final)
    assert np.array_equal(final["linear.weight"], P["linear.weight"].astype(np.float64))


def test_oracle_train_mode_masks_follow_the_offsets():
    """dropout 0.6 with explicit offsets: a different offset block gives different masks, the same block the same result"""
    import meld_step_oracle as MO
    m = mirror(3)
    P = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    U, umask, label = MG.case_inputs(7, 3, 3)
    a = MO.step(P, U, umask, label, 0.6, seed=11, offsets=[5, 6, 7], train=True)
    b = MO.step(P, U, umask, label, 0.6, seed=11, offsets=[5, 6, 7], train=True)
    c = MO.step(P, U, umask, label, 0.6, seed=11, offsets=[8, 9, 10], train=True)
    e = MO.step(P, U, umask, label, 0.6, seed=11, offsets=[5, 6, 7], train=False)
    assert a["loss"] == b["loss"] and a["loss"] != c["loss"] and a["loss"] != e["loss"]
    assert np.isfinite(a["log_prob"]).all()


def test_synthetic_meld_pickle_round_trips_through_the_loaders(tmp_path):
    from gan_ffn_amd import data as D
    path = str(tmp_path / "meld.pkl")
    train_ids, test_ids = D.write_synthetic_meld_pickle(path, n_train=9, n_test=4, seed=5)
    again = str(tmp_path / "meld2.pkl")
    D.write_synthetic_meld_pickle(again, n_train=9, n_test=4, seed=5)
    assert open(path, "rb").read() == open(again, "rb").read()              # seeded content
    for classify, n_cls in (("emotion", 7), ("sentiment", 3)):
        ds = D.MELDDataset(path, classify, True)
        assert len(ds) == 9 and len(D.MELDDataset(path, classify, False)) == 4
        text, audio, spk, um, lab, vid = ds[0]
        L = text.shape[0]
        assert text.shape == (L, 600) and audio.shape == (L, 300) and spk.shape == (L, 9) and um.shape == (L,) and 1 <= L <= 33
        assert bool((spk.sum(1) == 1).all()) and int(lab.max()) < n_cls and lab.dtype == torch.int64 and vid == train_ids[0]
        tr, va, te = D.get_MELD_loaders(path, batch_size=4, valid=0.0, classify=classify)
        assert len(va) == 0 and len(te) == 1 and len(tr) == 3
        seen = 0
        for collated in list(tr) + list(te):
            b = D.to_meld_batch(collated, "cpu")
            S, B = b["text"].shape[:2]
            seen += B
            assert b["text"].shape == (S, B, 600) and b["text"].dtype == torch.float32 and b["text"].is_contiguous()
            assert b["acoustic"].shape == (S, B, 300) and b["qmask"].shape == (S, B, 9)
            assert b["umask"].shape == (B, S) and b["umask"].dtype == torch.float32 and b["label"].shape == (B, S)
            assert b["label"].dtype == torch.int64 and len(b["vids"]) == B
            lens = b["umask"].sum(1).long()
            assert int(lens.max()) == S
            for j in range(B):                                               # prefix masks, zero padding
                assert bool((b["umask"][j, :lens[j]] == 1).all()) and bool((b["text"][lens[j]:, j] == 0).all())
        assert seen == 13


def test_train_or_eval_model_keeps_its_default_batch_maker():
    import inspect
    from gan_ffn_amd import artifacts as A
    sig = inspect.signature(A.train_or_eval_model)
    assert list(sig.parameters)[:4] == ["engine", "loader", "train", "device"] and sig.parameters["to_batch"].default is None
    assert callable(A.run_meld_training)
