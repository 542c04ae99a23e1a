"""The fp64 restatement of the step runner's train-mode sub-steps (tests/engine_oracle.py) against the oracle: with dropout
off it is the oracle's own train_disc / train_gen (which run D(real) and D(fake) as two passes), and with dropout on it
draws, for the real and the fake half of the [real | fake] batch, exactly the rows of the 2B-dialogue Philox layout.
No GPU needed."""
import numpy as np
import pytest
import torch

import engine_oracle as EO
from oracle import philox
import formula as F_
from oracle import ganffn_oracle as O
from test_hip_modules import oracle_head
from util import DIN, DISC, GEN, NETS, formula_sd

S, B, SEED, BASE = 6, 3, 4242, 96


def _net(cls_name, p_pe, p_enc, p_head):
    kind, _, _, H, _, _ = NETS[cls_name]
    return EO.Net(kind, formula_sd(cls_name), H, p_pe, p_enc, p_head)


def _x(tag, m):
    return torch.from_numpy(F_.formula_input("eo." + tag, S, B, DIN[m], pad_from=S - 2)).double()


def _close(a, b, what, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= rtol * scale, (what, np.abs(a - b).max(), scale)


@pytest.mark.parametrize("who,partner", [("visual", "text"), ("acoustic", "visual")])
def test_disc_substep_without_dropout_is_the_oracles_train_disc(who, partner):
    D, G = _net(DISC[who], 0.0, 0.0, 0.0), _net(GEN[partner], 0.0, 0.0, 0.0)
    xr, xp = _x(who, who), _x(partner, partner)
    got = EO.disc_substep(D, G, xr, xp, SEED, BASE, 5)
    od = O.OracleNet("disc", formula_sd(DISC[who]), D.H, 0.0, torch.float64)
    og = O.OracleNet("gen", formula_sd(GEN[partner]), G.H, 0.0, torch.float64)
    opt = O.Adam(od.parameters(), 0.0)                 # lr 0: the step leaves the parameters and their gradients alone
    valid, fake = torch.ones(S, B, 1, dtype=torch.float64), torch.zeros(S, B, 1, dtype=torch.float64)
    want = O.train_disc(od, xr, og, xp, opt, valid, fake, None)
    assert abs(got["loss"] - want) <= 1e-13 * abs(want), (got["loss"], want)
    assert set(got["grads"]) == {k for k, v in od.P.items() if v.grad is not None}
    assert ("object.weight" in got["grads"]) == (who == "visual")
    for k, g in got["grads"].items():
        _close(g, od.P[k].grad, k)


@pytest.mark.parametrize("who,partner", [("text", "acoustic"), ("visual", "acoustic")])
def test_gen_substep_without_dropout_is_the_oracles_train_gen(who, partner):
    G, D = _net(GEN[who], 0.0, 0.0, 0.0), _net(DISC[partner], 0.0, 0.0, 0.0)
    x = _x(who, who)
    got = EO.gen_substep(G, D, x, SEED, BASE, 7)
    og = O.OracleNet("gen", formula_sd(GEN[who]), G.H, 0.0, torch.float64)
    od = O.OracleNet("disc", formula_sd(DISC[partner]), D.H, 0.0, torch.float64)
    opt = O.Adam(og.parameters(), 0.0)
    want = O.train_gen(og, x, od, opt, torch.ones(S, B, 1, dtype=torch.float64), None, None)
    assert abs(got["loss"] - want) <= 1e-13 * abs(want), (got["loss"], want)
    assert set(got["grads"]) == {k for k, v in og.P.items() if v.grad is not None}
    for k, g in got["grads"].items():
        _close(g, og.P[k].grad, k)


@pytest.mark.parametrize("who,partner,i", [("visual", "acoustic", 0), ("text", "visual", 8)])
def test_disc_substep_draws_the_rows_of_the_2B_layout(who, partner, i):
    """dropout on: the real half of D's one pass uses rows (s, 0..B-1) and the fake half rows (s, B..2B-1) of the masks of
    a 2B-dialogue batch at offsets b + 4i + 2 (encoder) and b + 4i + 3 (head) — checked against the oracle run on each
    half alone with `Rng(full_batch=2B, select=...)`, which slices philox.keep_mask / attn_keep_mask of that layout"""
    D, G = _net(DISC[who], 0.2, 0.1, 0.2), _net(GEN[partner], 0.2, 0.1, 0.2)
    xr, xp = _x(who, who), _x(partner, partner)
    got = EO.disc_substep(D, G, xr, xp, SEED, BASE, i)
    P = {k: v.detach() for k, v in D.P.items()}
    real = xr @ P["object.weight"].T + P["object.bias"] if "object.weight" in P else xr
    a = BASE + 4 * i
    halves = []
    for x, sel in ((real, range(B)), (got["fake"], range(B, 2 * B))):
        h = O.encoder_stack(x, P, D.H, O.Rng(SEED, a + 2, True, full_batch=2 * B, select=sel))
        on = O.OracleNet("disc", {}, D.H)
        on.P = P
        halves.append(oracle_head(on, "disc", h, O.Rng(SEED, a + 3, True, full_batch=2 * B, select=sel)))
    _close(got["prob"][:, :B], halves[0], "real half")
    _close(got["prob"][:, B:], halves[1], "fake half")
    # the masks matter: the same pass without dropout, or with the halves' masks swapped, gives other probabilities
    D0 = _net(DISC[who], 0.0, 0.0, 0.0)
    p0 = EO.disc_substep(D0, G, xr, xp, SEED, BASE, i, fake=got["fake"])["prob"]
    assert (got["prob"] - p0).abs().max() > 1e-3
    assert (got["prob"][:, :B] - halves[1]).abs().max() > 1e-3


def test_gen_substep_draws_the_generator_offsets_and_a_frozen_eval_discriminator():
    """dropout on: the generator's masks at b + 4i (encoder) and b + 4i + 1 (head) over the B layout; the frozen
    discriminator draws none"""
    i = 3
    G, D = _net(GEN["text"], 0.2, 0.1, 0.2), _net(DISC["visual"], 0.2, 0.1, 0.2)
    x = _x("text", "text")
    got = EO.gen_substep(G, D, x, SEED, BASE, i)
    P = {k: v.detach() for k, v in G.P.items()}
    on = O.OracleNet("gen", {}, G.H)
    on.P = P
    out = oracle_head(on, "gen", O.encoder_stack(x, P, G.H, O.Rng(SEED, BASE + 4 * i, True)), O.Rng(SEED, BASE + 4 * i + 1, True))
    _close(got["out"], out, "generator output")
    prob = O.discriminator_forward(out, {k: v.detach() for k, v in D.P.items()}, D.H, 0.2, None)
    want = float(O.bce_mean(prob, torch.ones_like(prob)))
    assert abs(got["loss"] - want) <= 1e-13 * abs(want)


def test_adam_restatement_is_the_oracles_adam():
    """EO.adam (numpy, one step from given moments) against O.Adam over three steps, bias corrections included"""
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(50)
    p = torch.tensor(p0, requires_grad=True)
    opt = O.Adam([p], 1.1e-4, (0.5, 0.6))
    q, m, v = p0.copy(), np.zeros(50), np.zeros(50)
    for t in range(1, 4):
        g = rng.standard_normal(50) * 10.0 ** (-t)
        p.grad = torch.tensor(g)
        opt.step()
        q, m, v = EO.adam(q, g, m, v, t, 1.1e-4, 0.5, 0.6)
        _close(q, p.detach().numpy(), "adam t=%d" % t, 1e-15)


# ---- the classifier step runners: Phase2Engine.step and DrnnEngine._step ----------------------------------------------
def _gens(p_pe=0.0, p_enc=0.0, p_head=0.0):
    return {k: _net(GEN[k], p_pe, p_enc, p_head) for k in EO.GEN_KEYS}


def test_phase2_step_without_dropout_reproduces_the_reference_fixture():
    """the phase-2 restatement (EO.Net generators -> sum -> fc -> log_softmax -> weighted MaskedNLLLoss) against the
    reference's own numbers (tests/golden/misc.npz, the bounds of test_oracle_golden.py::test_phase2_forward_and_loss)"""
    from util import check_summary, golden
    g = golden("misc")
    batch = {k: torch.from_numpy(F_.formula_input("gan." + k, 7, 2, DIN[k], pad_from=5)) for k in DIN}
    batch["umask"], batch["label"] = torch.from_numpy(g["phase2/umask"]), torch.from_numpy(g["phase2/label"])
    fc_w = torch.from_numpy(F_.formula_tensor("phase2.fc.weight", (6, 100)))
    fc_b = torch.from_numpy(F_.formula_tensor("phase2.fc.bias", (6,)))
    gens = _gens()
    res = EO.phase2_step(gens, fc_w, fc_b, batch, SEED, EO.gen_adds(BASE), class_w=O.CLASS_WEIGHTS)
    assert np.abs(res["log_prob"].numpy() - g["phase2/log_prob"]).max() <= 2e-5
    assert abs(res["loss"] - float(g["phase2/loss_weighted"])) <= 2e-5
    assert np.abs(res["grad_fc_weight"].numpy() - g["phase2/grad_fc_weight"]).max() <= 2e-6
    check_summary(g, "phase2/grad_text_fc2_weight", res["grads"]["text"]["fc2.weight"], rtol=2e-4, atol=1e-8)
    check_summary(g, "phase2/grad_visual_l0_inproj", res["grads"]["visual"]["transformer_encoder.layers.0.self_attn.in_proj_weight"],
                  rtol=2e-4, atol=1e-9)
    # the class weights matter here: the unweighted loss is another number
    assert abs(float(g["phase2/loss_weighted"]) - float(g["phase2/loss_unweighted"])) > 1e-3
    # eval mode (adds None) is the same function when every p is 0
    ev = EO.phase2_step(_gens(), fc_w, fc_b, batch, SEED, None, class_w=O.CLASS_WEIGHTS)
    assert abs(ev["loss"] - res["loss"]) <= 1e-15 * abs(res["loss"])


def test_adam_with_weight_decay_reproduces_the_reference_fixture():
    """EO.adam_wd (L2 added to the gradient before the moments) against torch.optim.Adam(lr 1e-4, weight_decay 0.008) as
    the reference ran it: tests/golden/misc.npz adam/phase2/step0..2"""
    from util import golden
    g = golden("misc")
    p = F_.formula_tensor("adam.w", (37, 11)).astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step in range(3):
        grad = F_.formula_tensor("adam.g%d" % step, (37, 11)).astype(np.float64)
        p, m, v = EO.adam_wd(p, grad, m, v, step + 1, 1e-4, 0.9, 0.999, 0.008)
        assert np.abs(p - g["adam/phase2/step%d" % step]).max() <= 2e-7, step
    # without the decay the third step is measurably elsewhere
    q, m0, v0 = F_.formula_tensor("adam.w", (37, 11)).astype(np.float64), np.zeros_like(p), np.zeros_like(p)
    for step in range(3):
        q, m0, v0 = EO.adam(q, F_.formula_tensor("adam.g%d" % step, (37, 11)).astype(np.float64), m0, v0, step + 1, 1e-4, 0.9, 0.999)
    assert np.abs(q - g["adam/phase2/step2"]).max() > 1e-6


def _bimodel(listener, seed=2, dims=None):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    d = dims or dict(D_m=100, D_g=64, D_p=64, D_e=32, D_h=24)
    bm = DR.BiModel(n_classes=6, context_attention="general", listener_state=listener, dropout_rec=0.1, dropout=0.6, **d)
    with torch.no_grad():                       # livelier recurrent weights than the default init
        for p in bm.parameters():
            p.mul_(1.5)
    return bm.double()


def _drnn_batch(S, B, seed, lens):
    from gan_ffn_amd import data as D
    b = D.synthetic_batch(B=B, S_max=S, seed=seed)
    lens = torch.tensor(lens)
    valid = (torch.arange(S).unsqueeze(1) < lens.unsqueeze(0)).float()
    out = {k: b[k][:S] * valid.unsqueeze(2) for k in ("acoustic", "visual", "text", "qmask")}
    out["umask"] = valid.t().contiguous()
    out["label"] = b["label"][:, :S] * valid.t().long()
    assert out["text"].shape[:2] == (S, B)
    return out


@pytest.mark.parametrize("listener", [False, True])
def test_drnn_step_without_dropout_is_bimodel_and_masked_nll_under_autograd(listener):
    """dropout off (train mode with every p = 0, and eval mode): log-probabilities, loss, every BiModel parameter gradient,
    dL/dfusion and every generator gradient of EO.drnn_step equal the CPU BiModel (gan_ffn_amd/dialogue_rnn.py, pinned to
    the reference fixtures by test_dialogue_rnn_cpu.py / test_drnn_listener_cpu.py) + MaskedNLLLoss with one autograd
    pass through generators and head"""
    from gan_ffn_amd import model as M
    S, B = 6, 3
    batch = {k: v.double() if v.is_floating_point() else v for k, v in _drnn_batch(S, B, 9, [6, 4, 1]).items()}
    bm = _bimodel(listener)
    for mod in bm.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    w = torch.tensor(O.CLASS_WEIGHTS, dtype=torch.float64)
    got = EO.drnn_step(_gens(), bm, batch, SEED, BASE, train=True, class_w=w)
    ev = EO.drnn_step(_gens(), bm, batch, SEED, BASE, train=False, class_w=w)
    assert abs(ev["loss"] - got["loss"]) <= 1e-14 * abs(got["loss"])
    # reference: one autograd graph from the generators' parameters to the loss
    gens = _gens()
    ref_bm = _bimodel(listener)
    ref_bm.train()
    for mod in ref_bm.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    fusion = sum(gens[k].forward(batch[k], SEED, 0, 0, False) for k in EO.GEN_KEYS)
    fusion.retain_grad()
    lp = ref_bm(fusion, batch["qmask"], batch["umask"])[0]
    loss = M.MaskedNLLLoss(w)(lp.transpose(0, 1).contiguous().view(-1, 6), batch["label"].view(-1), batch["umask"])
    loss.backward()
    loss = float(loss.detach())
    assert abs(got["loss"] - loss) <= 1e-13 * abs(loss)
    _close(got["log_prob"], lp.detach(), "log_prob")
    _close(got["d_fusion"], fusion.grad, "d_fusion")
    pr = dict(ref_bm.named_parameters())
    assert len(got["grads"]) == 32 + (8 if listener else 0)            # the engine's head slab holds these
    for k, g in got["grads"].items():
        if pr[k].grad is None:
            assert float(g.abs().max()) == 0.0, k
        else:
            _close(g, pr[k].grad, k)
    for k in EO.GEN_KEYS:
        assert set(got["gen_grads"][k]) == set(gens[k].trained)
        for n, g in got["gen_grads"][k].items():
            _close(g, gens[k].P[n].grad, (k, n), 1e-11)


def _layout_case(p_rec, p_join):
    """a hand-sized BiModel and a ragged batch: lengths 5 (= S), 2 and 1"""
    S, B, lens = 5, 3, [5, 2, 1]
    bm = _bimodel(False, seed=6, dims=dict(D_m=8, D_g=8, D_p=8, D_e=4, D_h=4))
    for c in (bm.dialog_rnn_f.dialogue_cell, bm.dialog_rnn_r.dialogue_cell):
        c.dropout.p = p_rec
    bm.dropout_rec.p, bm.dropout.p = p_join, 0.0
    b = _drnn_batch(S, B, 4, lens)
    U = b["text"][:, :, :8].double()
    masks = EO.drnn_masks(bm, S, B, SEED, BASE + EO.A_REC, BASE + EO.A_HEAD)
    res = EO.drnn_head(bm, U, b["qmask"].double(), b["umask"], b["label"], masks=masks)
    return S, B, lens, bm, U, b, res


def test_drnn_join_masks_the_reversed_half_at_forward_time_rows():
    """emotions = cat(drop_5(e_f), drop_6(reverse(e_b))): the mask of the second half is drawn for the FORWARD-time row
    s * B + b of the position the reversed emotion lands on (model.py:1037-1041 reverses first, then applies
    dropout_rec) — for a dialogue shorter than S the reverse direction's step t is utterance len - 1 - t, so masking e_b at
    its own rows would move the mask; a length-1 dialogue has one row, s = t = 0"""
    S, B, lens, bm, U, b, res = _layout_case(0.0, 0.5)
    De = 4
    kf = philox.keep_mask(S * B, De, 0.5, 5, SEED, BASE + 7).reshape(S, B, De) * 2.0
    kb = philox.keep_mask(S * B, De, 0.5, 6, SEED, BASE + 7).reshape(S, B, De) * 2.0
    e_f, e_b, em = res["e_f"].numpy(), res["e_b"].numpy(), res["emotions"].numpy()
    _close(em[..., :De], e_f * kf, "forward half")
    want, moved = np.zeros((S, B, De)), np.zeros((S, B, De))
    for bb, L in enumerate(lens):
        for s in range(L):
            want[s, bb] = e_b[L - 1 - s, bb] * kb[s, bb]
            moved[s, bb] = e_b[L - 1 - s, bb] * kb[L - 1 - s, bb]        # the mask drawn at the reverse direction's own row
    _close(em[..., De:], want, "reversed half")
    assert np.abs(em[:, 1, De:] - moved[:, 1]).max() > 1e-3            # len 2 < S: the two layouts differ
    assert (em[1:, 2, De:] == 0).all() and np.abs(em[0, 2, De:]).max() > 0   # len 1: one row, zeros beyond it


def test_drnn_reverse_recurrence_masks_are_indexed_in_its_own_reversed_time():
    """the reverse DialogueRNN's step t processes utterance len - 1 - t and draws its masks at row t * B + b, sites
    9 + 4 (party update) and 10 + 4 (emotion): its first emotion, restated by hand from the GRU cells, for the length-2 and
    the length-1 dialogue"""
    S, B, lens, bm, U, b, res = _layout_case(0.5, 0.0)
    cr = bm.dialog_rnn_r.dialogue_cell
    H, He = 8, 4
    kp = philox.keep_mask(S * B, H, 0.5, 13, SEED, BASE + 6) * 2.0
    ke = philox.keep_mask(S * B, He, 0.5, 14, SEED, BASE + 6) * 2.0

    def first_emotion(bb, row):
        u = U[lens[bb] - 1, bb].unsqueeze(0)                   # the dialogue's last utterance comes first
        with torch.no_grad():
            qs = cr.p_cell(torch.cat([u, torch.zeros(1, H, dtype=u.dtype)], 1), torch.zeros(1, H, dtype=u.dtype))
            qs = qs * torch.from_numpy(kp[row])                  # one mask row for both parties; the speaker's is selected
            return (cr.e_cell(qs, torch.zeros(1, He, dtype=u.dtype)) * torch.from_numpy(ke[row]))[0].numpy()

    for bb in (1, 2):
        _close(res["e_b"][0, bb].numpy(), first_emotion(bb, 0 * B + bb), "first reverse emotion of dialogue %d" % bb)
    # the row of the utterance's forward position (s = 1 for the length-2 dialogue) is another mask
    assert np.abs(res["e_b"][0, 1].numpy() - first_emotion(1, 1 * B + 1)).max() > 1e-3
