"""The other context attention types of the DialogueRNN (dot, general2, concat; model.py:134-194) on the HIP recurrence
(csrc/dialogue_rnn.hip through ganffn_drnn_att_fwd / _bwd), with and without listener state: against the fp64 torch
restatement on the CPU in eval mode and in train mode with the same Philox masks, BiModel against the reference's own
fixtures, the proof that the HIP path (not the per-step torch cell) runs, and DrnnEngine for all five types."""
import copy

import pytest
import torch

from oracle import philox
from test_hip_drnn_kernel import _MaskSeq, compare, make_inputs, philox_masks
from test_hip_drnn_listener import listener_masks

pytestmark = pytest.mark.gpu

CASES = {
    "dot": dict(context_attention="dot", D_m=100, D_g=100, D_p=100, D_e=100),
    "general2": dict(context_attention="general2", D_m=100, D_g=500, D_p=500, D_e=100),
    "concat": dict(context_attention="concat", D_m=100, D_g=500, D_p=500, D_e=100, D_a=100),
    "general2_listener": dict(context_attention="general2", listener_state=True, D_m=100, D_g=500, D_p=500, D_e=100),
    "concat_listener": dict(context_attention="concat", listener_state=True, D_m=100, D_g=500, D_p=500, D_e=100, D_a=100),
}


def build(case, seed=7, dropout=0.1):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    m = DR.DialogueRNN(dropout=dropout, **CASES[case])
    with torch.no_grad():                       # livelier recurrent weights than the default init
        for n, p in m.named_parameters():
            p.mul_(1.5)
            if n == "dialogue_cell.attention.transform.weight" and CASES[case]["context_attention"] == "general2":
                p.mul_(4.0)                     # general2's init (std 0.01) leaves the scores near 0: make the tanh bend
    return m


@pytest.mark.parametrize("S,B", [(7, 3), (23, 5), (94, 30), (33, 40), (1, 2), (110, 4)])
@pytest.mark.parametrize("case", list(CASES))
def test_eval_mode_matches_torch_restatement(case, S, B):
    from gan_ffn_amd import ops
    U, qmask = make_inputs(S, B, seed=S * 100 + B + 2)
    m_cpu = build(case).double().eval()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().eval()
    listener = CASES[case].get("listener_state", False)
    assert ops.dialogue_rnn_listener_supported(m_gpu.dialogue_cell, U.cuda(), qmask.cuda()) == listener
    assert ops.dialogue_rnn_supported(m_gpu.dialogue_cell, U.cuda(), qmask.cuda()) == (not listener)
    compare(m_gpu, m_cpu, U, qmask)          # emotions, alpha, dU, every parameter gradient (the attention's included)
    names = [k for k, _ in m_gpu.named_parameters() if ".attention." in k]
    assert len(names) == {"dot": 0, "general2": 2, "concat": 2}[case.split("_")[0]], names


@pytest.mark.parametrize("S,B", [(9, 4), (94, 30)])
@pytest.mark.parametrize("case", list(CASES))
def test_train_mode_matches_torch_restatement_with_the_same_philox_masks(case, S, B):
    from gan_ffn_amd import ops
    U, qmask = make_inputs(S, B, seed=S + B + 2)
    p, seed = 0.1, 20261016
    m_cpu = build(case, dropout=p).double().train()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().train()
    H = CASES[case]["D_g"]
    if CASES[case].get("listener_state", False):
        m_cpu.dialogue_cell.dropout = _MaskSeq(listener_masks(S, B, H, 100, p, seed, 0))
    else:
        m_cpu.dialogue_cell.dropout = _MaskSeq(philox_masks(S, B, H, 100, p, seed, 0))
    ops.manual_seed(seed)                       # the call below takes rng offset 0
    compare(m_gpu, m_cpu, U, qmask)


@pytest.mark.parametrize("case", ["general2", "concat", "dot", "general2_listener", "concat_listener"])
def test_bimodel_matches_reference_fixture_small(case):
    import test_drnn_context_cpu as X
    X.check_small(X.context_model(case).cuda(), case, "cuda", lp_tol=5e-5, du_tol=2e-4, g_tol=5e-4)


@pytest.mark.parametrize("case", ["general2", "concat"])
def test_bimodel_matches_reference_fixture_at_configuration_5_size(case):
    import test_drnn_context_cpu as X
    X.check_big(X.context_model(case).cuda(), case, "cuda", rtol=1e-4, grtol=1e-3)


@pytest.mark.parametrize("case", list(CASES))
def test_hip_path_is_taken(case, monkeypatch):
    """with the per-step torch cell disabled, a BiModel of every type still runs forward and backward on CUDA"""
    from gan_ffn_amd import dialogue_rnn as DR

    def refuse(*a, **k):
        raise AssertionError("DialogueRNNCell.forward called: the recurrence ran on torch ops")
    torch.manual_seed(4)
    c = CASES[case]
    m = DR.BiModel(D_h=100, n_classes=6, dropout_rec=0.1, dropout=0.6, **c).cuda().train()
    monkeypatch.setattr(DR.DialogueRNNCell, "forward", refuse)
    U, qmask = make_inputs(13, 4, seed=9)
    umask = (qmask.sum(2) > 0).float().t().contiguous()
    Ug = U.cuda().requires_grad_(True)
    lp = m(Ug, qmask.cuda(), umask.cuda())[0]
    lp.sum().backward()
    assert torch.isfinite(Ug.grad).all() and float(Ug.grad.abs().max()) > 0
    att = dict(m.dialog_rnn_r.dialogue_cell.attention.named_parameters())
    assert len(att) == {"dot": 0, "general2": 2, "concat": 2}[case.split("_")[0]]
    for n, p in att.items():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, n


ENGINE_CASES = {
    "general": dict(context_attention="general"),
    "simple": dict(context_attention="simple"),
    "dot": dict(context_attention="dot", D_g=100, D_p=100),
    "general2": dict(context_attention="general2"),
    "concat": dict(context_attention="concat"),
    "simple_listener": dict(context_attention="simple", listener_state=True),
    "dot_listener": dict(context_attention="dot", D_g=100, D_p=100, listener_state=True),
    "general2_listener": dict(context_attention="general2", listener_state=True),
    "concat_listener": dict(context_attention="concat", listener_state=True),
}
N_ATT = {"general": 1, "simple": 1, "dot": 0, "general2": 2, "concat": 2}


def _engine_net(case, seed=3, dropout_off=False):
    from gan_ffn_amd import model as M
    from test_hip_drnn_engine import DIMS as EDIMS
    d = dict(EDIMS)
    d.update(ENGINE_CASES[case])
    d.setdefault("listener_state", False)
    torch.manual_seed(seed)
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                dropout_rec=0.1, dropout=0.6, **d)
    if dropout_off:
        for mod in net.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        for g in (net.acoustic_generator, net.visual_generator, net.text_generator):
            g.transformer_encoder.enc_dropout = 0.0
    return net.cuda().train()


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_builds_for_every_attention_type(case):
    from gan_ffn_amd import engine as E
    net = _engine_net(case)
    eng = E.DrnnEngine(net)
    att = ENGINE_CASES[case]["context_attention"]
    listener = ENGINE_CASES[case].get("listener_state", False)
    assert eng.att == att and eng.listener == listener
    assert len(eng._hparams) == 2 * (12 + N_ATT[att]) + 6 + (8 if listener else 0)


def test_engine_refuses_what_the_kernels_cannot_run():
    from gan_ffn_amd import engine as E
    # (dot with D_m != D_g cannot be built: MatchingAttention asserts it, as the reference does)
    with pytest.raises(ValueError, match="got concat attention"):
        E.DrnnEngine(_bad_net(dict(context_attention="concat", D_a=102)))
    with pytest.raises(ValueError, match="got concat attention"):
        E.DrnnEngine(_bad_net(dict(context_attention="concat", D_a=516)))
    with pytest.raises(ValueError, match="D_g = 516"):
        E.DrnnEngine(_bad_net(dict(context_attention="general2", D_g=516, D_p=516)))
    with pytest.raises(ValueError, match="D_p = 400"):
        E.DrnnEngine(_bad_net(dict(context_attention="dot", D_g=100, D_p=400)))


def _bad_net(kw):
    from gan_ffn_amd import model as M
    from test_hip_drnn_engine import DIMS as EDIMS
    d = dict(EDIMS)
    d.update(kw)
    return M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                 listener_state=False, dropout_rec=0.1, dropout=0.6, **d).cuda()


@pytest.mark.parametrize("S,B", [(13, 4), (94, 30)])
@pytest.mark.parametrize("case", [c for c in ENGINE_CASES if c != "general"])
def test_engine_step_matches_module_path_autograd(case, S, B):
    """dropout off: the engine step's loss, log-probabilities and every head gradient (the attention tensors included)
    equal the module path's autograd results, and Adam moves the attention tensors state_dict() sees"""
    from gan_ffn_amd import data as D, engine as E, model as M
    from test_hip_drnn_engine import W, rel
    net = _engine_net(case, dropout_off=True)
    ref = copy.deepcopy(net)
    b = D.synthetic_batch(B=B, S_max=S, seed=5, device="cuda")
    lp = ref(b["acoustic"], b["visual"], b["text"], b["qmask"], b["umask"])[0]
    loss_ref = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))(lp.transpose(0, 1).contiguous().view(-1, 6), b["label"].view(-1),
                                                               b["umask"])
    loss_ref.backward()
    keys = [k for k in net.state_dict() if ".dialogue_cell.attention." in k]
    att = ENGINE_CASES[case]["context_attention"]
    assert len(keys) == 2 * N_ATT[att]
    before = {k: v.detach().clone() for k, v in net.state_dict().items() if k in keys}
    eng = E.DrnnEngine(net)
    loss, log_prob = eng.step(b, train=True)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 2e-5 * max(1.0, abs(float(loss_ref)))
    assert rel(log_prob, lp) < 1e-4
    refp = dict(ref.named_parameters())
    names = {id(p): n for n, p in net.named_parameters()}
    for i, p in enumerate(eng._hparams):
        g_ref = refp[names[id(p)]].grad
        assert g_ref is not None, names[id(p)]
        assert rel(eng._hp(i, True).view_as(p), g_ref) < 2e-3, names[id(p)]
    after = net.state_dict()
    for k in keys:
        assert float((after[k] - before[k]).abs().max()) > 0, k


@pytest.mark.parametrize("S,B", [(13, 4), (94, 30)])
@pytest.mark.parametrize("case", ["general2", "concat", "concat_listener"])
def test_engine_train_step_with_dropout_matches_fp64_oracle(case, S, B):
    """dropout on: the engine step against tests/engine_oracle.drnn_step (the cell's own torch-op path in fp64 with the
    engine's Philox masks), on the engine's ReLU patterns"""
    import engine_oracle as EO
    from gan_ffn_amd import engine as E, ops
    from test_hip_classifier_engines_train_oracle import DRNN_L2, DRNN_LR, SEED, W, _batch, _close, _host_batch
    from util import relu_masks
    net = _engine_net(case)
    eng = E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W)
    bm = copy.deepcopy(net.bi_model).cpu().double()
    pre = {k: eng.G[k].slab.cpu().clone() for k in EO.GEN_KEYS}
    batch = _batch(S, B, 100 * S + B)
    ops.manual_seed(SEED)
    loss, _ = eng.step(batch, train=True)
    torch.cuda.synchronize()
    b = eng._base_add
    T, f = S * B, eng._f
    hb = _host_batch(batch)
    gens = {k: EO.Net.from_state(eng.G[k], pre[k]) for k in EO.GEN_KEYS}
    masks_g = {k: relu_masks(eng.pass_G[k], eng.pass_G[k].cfg_train, S, B) for k in EO.GEN_KEYS}
    pattern = f["hidden"][:T * eng.Dh2].view(S, B, eng.Dh2).cpu().double() > 0
    ch = EO.drnn_step(gens, bm, hb, SEED, b, True, relu_masks=masks_g, hidden_pattern=pattern, class_w=W)
    tag = "%s (%d, %d)" % (case, S, B)
    assert abs(float(loss) - ch["loss"]) < 2e-5 * abs(ch["loss"]), (float(loss), ch["loss"])
    _close("log_prob", f["log_prob"][:T * 6].view(S, B, 6).cpu().double(), ch["log_prob"], 1e-4, 0.0, tag + " log_prob")
    hg = eng.h_grad.cpu()
    names = {id(p): n for n, p in net.named_parameters()}
    n_att = 0
    for o, p in zip(eng._hoffs, eng._hparams):
        n = names[id(p)][len("bi_model."):]
        _close("head gradient", hg[o:o + p.numel()].view(p.shape).double(), ch["grads"][n], 1e-3, 1e-12, "%s grad %s" % (tag, n))
        n_att += ".attention." in n and "matchatt" not in n
    assert n_att == 4
