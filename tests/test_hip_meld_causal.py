"""The causal MELD classifier on the device — dialogue_rnn.MELDLSTMModel(causal=True) (the module path) and engine.MeldEngine on
it — against the fp64 restatement tests/meld_causal_oracle.py (pinned to the module on the CPU by tests/test_meld_causal_cpu.py):
eval and train steps, train mode with the engine's own Philox masks, that neither path ever looks ahead (bit for bit), that
padding cannot matter, that packed composes, that a default engine is unmoved by a causal one in the same process, the refusals,
and the trainer.  Bounds are those of tests/test_hip_meld_engine.py; every compared distance is printed before it is asserted."""
import copy

import numpy as np
import pytest
import torch

import meld_causal_oracle as CO

pytestmark = pytest.mark.gpu

LR, L2 = 3e-4, 1e-4
SEED = 20261021
SMALL, MELD = (16, 8, 8), (600, 300, 300)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def dist(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def model(dims=SMALL, dropout=0.0, seed=2, causal=True, packed=False, C_=7):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    if causal:
        return DR.MELDLSTMModel(*dims, n_classes=C_, dropout=dropout, packed=packed, causal=True).cuda().train()
    return DR.MELDLSTMModel(*dims, n_classes=C_, dropout=dropout, packed=packed).cuda().train()


def batch(S, B, D_m, lengths=None, seed=5, C_=7):
    g = torch.Generator().manual_seed(seed)
    lengths = [S] * B if lengths is None else lengths
    umask = torch.arange(S).unsqueeze(0).lt(torch.tensor(lengths).unsqueeze(1)).float()
    text = (torch.rand(S, B, D_m, generator=g) - 0.5) * umask.t().unsqueeze(-1)
    label = torch.randint(0, C_, (B, S), generator=g)
    return {"text": text.contiguous().cuda(), "umask": umask.cuda(), "label": label.cuda()}


def ragged(S, B):
    """prefix lengths: a full dialogue, a one-utterance one, the rest in between"""
    return [(S, 1, S // 2 + 1, S - 1)[b % 4] for b in range(B)]


def module_step(m, b):
    from gan_ffn_amd import model as M
    lp, alpha, _, _ = m(b["text"], None, b["umask"])
    loss = M.MaskedNLLLoss()(lp.transpose(0, 1).contiguous().view(-1, lp.shape[2]), b["label"].view(-1), b["umask"])
    if m.training:
        loss.backward()
    return loss.detach(), lp.detach(), torch.stack(alpha, 1).detach()


def engine_named(eng):
    names = {id(p): k for k, p in eng.module.named_parameters()}
    return [names[id(p)] for p in eng._params]


def engine_grads(eng):
    return {k: eng._p(i, True).view_as(eng._params[i]).detach().cpu().numpy().copy() for i, k in enumerate(engine_named(eng))}


def host_params(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------------------------------
# 1. the module path against the oracle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,dims", [(9, 3, SMALL), (6, 3, MELD)])
def test_module_path_matches_the_oracle_in_eval(S, B, dims):
    m = model(dims).eval()
    b = batch(S, B, dims[0], ragged(S, B))
    with torch.no_grad():
        loss, lp, alpha = module_step(m, b)
    o_loss, o_lp, o_alpha = CO.forward(host_params(m), b["text"].cpu().double(), b["umask"].cpu().double(), b["label"].cpu())
    d = (rel(lp, o_lp), rel(alpha, o_alpha), abs(float(loss) - float(o_loss)) / abs(float(o_loss)))
    print("causal module eval (%d, %d) %s: log_prob %.2e alpha %.2e loss %.2e" % (S, B, dims, *d))
    assert d[0] < 1e-4 and d[1] < 1e-4 and d[2] < 2e-5
    assert float(alpha.triu(1).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------
# 2. the engine against the module path under autograd
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,max_dialogues", [(9, 3, 32), (5, 40, 64)])
def test_engine_step_matches_module_path_autograd(S, B, max_dialogues):
    """dropout 0: loss 2e-5 relative, log_prob and alpha 1e-4, every gradient tensor 2e-3 of its scale; eval changes nothing"""
    from gan_ffn_amd import engine as E
    net = model(SMALL, seed=3)
    ref = copy.deepcopy(net)
    b = batch(S, B, SMALL[0], ragged(S, B))
    eng = E.MeldEngine(net, lr=LR, weight_decay=L2, max_dialogues=max_dialogues)
    assert eng.causal and eng.ndir == 1 and len(eng._params) == 20 and engine_named(eng) == CO.trained_names()
    # eval first: no parameter, moment or step-count change
    before = eng.slab.clone()
    loss_e, lp_e = eng.step(b, train=False)
    ref.eval()
    with torch.no_grad():
        loss_m, lp_m, alpha_m = module_step(ref, b)
    d = (abs(float(loss_e) - float(loss_m)), rel(lp_e, lp_m), rel(eng.alpha, alpha_m))
    print("causal engine eval (%d, %d): loss %.3e log_prob %.2e alpha %.2e" % (S, B, *d))
    assert d[0] < 2e-5 * max(1.0, abs(float(loss_m))) and d[1] < 1e-4 and d[2] < 1e-4
    assert torch.equal(eng.slab, before) and int(eng.step_count.item()) == 0
    # one train step
    ref.train()
    loss_ref, lp_ref, alpha_ref = module_step(ref, b)
    loss, lp = eng.step(b, train=True)
    torch.cuda.synchronize()
    d = (abs(float(loss) - float(loss_ref)), rel(lp, lp_ref), rel(eng.alpha, alpha_ref))
    print("causal engine train (%d, %d): loss %.3e log_prob %.2e alpha %.2e" % (S, B, *d))
    assert d[0] < 2e-5 * max(1.0, abs(float(loss_ref))) and d[1] < 1e-4 and d[2] < 1e-4
    refp = dict(ref.named_parameters())
    worst = (0.0, "")
    for i, k in enumerate(engine_named(eng)):
        assert refp[k].grad is not None, k
        r = rel(eng._p(i, True).view_as(refp[k]), refp[k].grad)
        worst = max(worst, (r, k))
        assert r < 2e-3, (k, r)
    print("causal engine train (%d, %d): worst gradient %.2e %s" % (S, B, *worst))
    assert refp["linear.weight"].grad is None and int(eng.step_count.item()) == 1


# ------------------------------------------------------------------------------------------------------------------
# 3. train mode against the fp64 oracle with the engine's own masks
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_train_mode_step_matches_fp64_oracle_with_the_engines_masks(packed):
    """dropout 0.6, two consecutive steps: the inter-layer masks are Philox sites 64 + l over [S B x D_e] at offsets base + l of the
    block the engine drew; log_prob, the loss and every gradient tensor at 1e-3 of the tensor's scale"""
    from gan_ffn_amd import engine as E, ops
    S, B = 9, 3
    lengths = [9, 4, 1]
    net = model(SMALL, dropout=0.6, seed=7, packed=packed)
    b = batch(S, B, SMALL[0], lengths, seed=9)
    ops.manual_seed(SEED)
    eng = E.MeldEngine(net, lr=LR, weight_decay=L2, packed=packed)
    names = engine_named(eng)
    text, umask, label = b["text"].cpu().numpy(), b["umask"].cpu().numpy(), b["label"].cpu().numpy()
    prev_base = None
    for i in range(2):
        P = {k: eng._p(j).view_as(eng._params[j]).detach().cpu().numpy().copy() for j, k in enumerate(names)}
        loss, lp = eng.step(b, train=True)
        torch.cuda.synchronize()
        base = eng._base_add
        offsets = [base + l for l in range(eng.L - 1)]
        assert eng.n_adds == eng.L - 1 and ops.DeviceRng.get(eng.dev).counter == base + eng.n_adds
        assert prev_base is None or base == prev_base + eng.n_adds
        prev_base = base
        seed, dev_off = [int(v) for v in ops.DeviceRng.get(eng.dev).state.cpu()]
        assert dev_off == 0
        o = CO.step(P, text, umask, label, 0.6, seed=seed, offsets=offsets, train=True, lengths=lengths if packed else None)
        d_lp, d_loss = dist(lp.cpu().numpy(), o["log_prob"]), abs(float(loss) - o["loss"]) / abs(o["loss"])
        d_al = dist(eng.alpha.cpu().numpy(), o["alpha"])
        print("causal train oracle step %d packed=%s: log_prob %.2e loss %.2e alpha %.2e" % (i, packed, d_lp, d_loss, d_al))
        assert d_lp <= 1e-3 and d_loss <= 1e-3 and d_al <= 1e-3
        g_e = engine_grads(eng)
        worst = (0.0, "")
        for k in names:
            d = dist(g_e[k], o["grads"][k])
            worst = max(worst, (d, k))
            assert d <= 1e-3, (i, k, d)
        print("causal train oracle step %d: worst gradient %.2e of scale (%s)" % (i, *worst))
    # a different mask block gives a different step: the masks are really applied
    o2 = CO.step(P, text, umask, label, 0.6, seed=seed, offsets=[off + 100 for off in offsets], train=True,
                 lengths=lengths if packed else None)
    assert abs(o2["loss"] - o["loss"]) > 1e-6


# ------------------------------------------------------------------------------------------------------------------
# 4. never looks ahead, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lookahead():
    from gan_ffn_amd import engine as E
    S, B = 9, 3
    net = model(SMALL, seed=11).eval()
    eng = E.MeldEngine(net)
    b = batch(S, B, SMALL[0])
    with torch.no_grad():
        _, lp_m, alpha_m = module_step(net, b)
    _, lp_e = eng.step(b, train=False)
    return net, eng, b, lp_m.clone(), alpha_m.clone(), lp_e.clone(), eng.alpha.clone()


@pytest.mark.parametrize("t", [0, 4, 8])
def test_neither_path_looks_ahead(lookahead, t):
    net, eng, b, lp_m, alpha_m, lp_e, alpha_e = lookahead
    S, B, D_m = b["text"].shape
    b2 = dict(b)
    text = b["text"].clone()
    if t + 1 < S:
        junk = torch.randn(S - t - 1, B, D_m, generator=torch.Generator().manual_seed(t))
        junk[:, 0] *= 1e3                                               # magnitudes up to ~1e3 among them
        text[t + 1:] = junk.cuda()
    b2["text"] = text
    with torch.no_grad():
        _, lp2, alpha2 = module_step(net, b2)
    assert torch.equal(lp2[:t + 1], lp_m[:t + 1]) and torch.equal(alpha2[:, :t + 1], alpha_m[:, :t + 1])
    _, lp3 = eng.step(b2, train=False)
    assert torch.equal(lp3[:t + 1], lp_e[:t + 1]) and torch.equal(eng.alpha[:, :t + 1], alpha_e[:, :t + 1])
    if t + 1 < S:
        assert not torch.equal(lp2[t + 1:], lp_m[t + 1:]) and not torch.equal(lp3[t + 1:], lp_e[t + 1:])


# ------------------------------------------------------------------------------------------------------------------
# 5. padding cannot matter; packed composes; a default engine is unmoved
# ------------------------------------------------------------------------------------------------------------------
def _one_train_step(b, packed, seed=13):
    from gan_ffn_amd import engine as E, ops
    net = model(SMALL, dropout=0.6, seed=seed, packed=packed)
    ops.manual_seed(SEED)
    eng = E.MeldEngine(net, lr=LR, weight_decay=L2, packed=packed)
    loss, lp = eng.step(b, train=True)
    torch.cuda.synchronize()
    return eng.slab.clone(), loss.clone(), lp.clone()


def test_padding_cannot_matter_and_packed_composes():
    """prefix masks of lengths [9, 4, 1]; two batches that differ only at padded utterances (finite values): one train step each
    gives the same parameter slab, loss and log_prob at real positions bit for bit — without `packed`, because a forward-only
    recurrence and a causal attention never carry a later (padded) step into an earlier (real) one, and the loss masks the rest.
    packed=True gives the same bits at real positions."""
    S, B, lengths = 9, 3, [9, 4, 1]
    b = batch(S, B, SMALL[0], lengths)
    real = b["umask"].t().bool()                                        # (S, B)
    b2 = dict(b)
    junk = torch.randn(S, B, SMALL[0], generator=torch.Generator().manual_seed(1)).cuda() * 30.0
    b2["text"] = torch.where(real.unsqueeze(-1), b["text"], junk).contiguous()
    assert not torch.equal(b2["text"], b["text"])
    slab, loss, lp = _one_train_step(b, False)
    slab2, loss2, lp2 = _one_train_step(b2, False)
    assert torch.equal(slab2, slab) and torch.equal(loss2, loss) and torch.equal(lp2[real], lp[real])
    assert not torch.equal(lp2[~real], lp[~real])                       # (the padded rows did see the junk)
    slab3, loss3, lp3 = _one_train_step(b, True)
    assert torch.equal(slab3, slab) and torch.equal(loss3, loss) and torch.equal(lp3[real], lp[real])
    slab4, loss4, lp4 = _one_train_step(b2, True)
    assert torch.equal(slab4, slab) and torch.equal(loss4, loss) and torch.equal(lp4[real], lp[real])


def test_a_default_engine_is_unmoved_by_a_causal_one():
    from gan_ffn_amd import engine as E, ops
    b = batch(9, 3, 16, [9, 4, 1])

    def default_step():
        net = model((16, 8, 16), dropout=0.6, seed=17, causal=False)
        ops.manual_seed(SEED)
        eng = E.MeldEngine(net, lr=LR, weight_decay=L2)
        assert not eng.causal and eng.ndir == 2 and len(eng._params) == 36
        loss, lp = eng.step(b, train=True)
        torch.cuda.synchronize()
        return eng.slab.clone(), loss.clone(), lp.clone(), eng.alpha.clone()

    first = default_step()
    _one_train_step(b, False)
    _one_train_step(b, True)
    for a, c in zip(first, default_step()):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals; the trainer
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_are_value_errors_that_name_the_module_path():
    from gan_ffn_amd import engine as E
    m = model(SMALL)
    m.causal = False                                                   # contradicts its forward-only LSTM
    with pytest.raises(ValueError, match="module path"):
        E.MeldEngine(m)
    d = model((16, 8, 16), causal=False)
    d.causal = True                                                    # contradicts its bidirectional LSTM
    with pytest.raises(ValueError, match="module path"):
        E.MeldEngine(d)
    with pytest.raises(ValueError, match="module path"):
        E.MeldEngine(model((16, 6, 6)))                                # D_e not a multiple of 4
    with pytest.raises(ValueError, match="module path"):
        E.MeldEngine(model((16, 8, 16)))                               # smax_fc not D_e wide
    eng = E.MeldEngine(model(SMALL))
    before = eng.slab.clone()
    for S, B in ((129, 2), (5, 33)):
        b = {"text": torch.zeros(S, B, 16, device="cuda"), "umask": torch.ones(B, S, device="cuda"),
             "label": torch.zeros(B, S, dtype=torch.long, device="cuda")}
        with pytest.raises(ValueError, match="module path"):
            eng.step(b, train=True)
    assert int(eng.step_count.item()) == 0 and torch.equal(eng.slab, before)


def test_run_meld_training_causal(tmp_path):
    from gan_ffn_amd import artifacts as A, data as D
    path = str(tmp_path / "meld.pkl")
    D.write_synthetic_meld_pickle(path, n_train=20, n_test=6, seed=4)
    lines = []
    best_loss, best_f, labels, preds, masks, att = A.run_meld_training(path, n_epochs=2, batch_size=8, seed=1, log=lines.append, causal=True)
    assert np.isfinite(best_loss) and np.isfinite(best_f) and 0.0 <= best_f <= 100.0 and len(labels) == len(preds) == len(masks)
    assert len(lines) == 2 and lines[0].startswith("epoch 1 train_loss ")
