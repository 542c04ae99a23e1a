"""The listener-state DialogueRNN (listener_state = True, model.py:899-921; train_IEMOCAP_DialogueRNN.py --active-listener) on
the HIP recurrence (csrc/dialogue_rnn.hip, ganffn_drnn_listener_fwd / _bwd): against the fp64 torch restatement on the CPU in
eval mode and in train mode with the same Philox masks (site 11 + 4 * direction for the listener), BiModel against the
reference's own fixture, and the proof that the HIP path (not the per-step torch cell) is what runs."""
import copy

import pytest
import torch

from oracle import philox
from test_hip_drnn_kernel import DIMS, _MaskSeq, compare, make_inputs

pytestmark = pytest.mark.gpu


def build(seed=7, dropout=0.1):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    m = DR.DialogueRNN(context_attention="general", listener_state=True, dropout=dropout, **DIMS)
    with torch.no_grad():                       # livelier recurrent weights than the default init
        for p in m.parameters():
            p.mul_(1.5)
    return m


def listener_masks(S, B, H, He, p, seed, offset, direction=0):
    """the cell's dropout calls per step in order: g (B,H), qs (B,P,H), ql (B,P,H) — the listener's own site — and e (B,He)"""
    def keep(cols, site):
        return torch.from_numpy(philox.keep_mask(S * B, cols, p, site + 4 * direction, seed, offset)).double() / (1 - p)
    kg, kp = keep(H, 8).view(S, B, H), keep(H, 9).view(S, B, H)
    kl, ke = keep(2 * H, 11).view(S, B, 2, H), keep(He, 10).view(S, B, He)
    out = []
    for t in range(S):
        out += [kg[t], kp[t].unsqueeze(1).expand(-1, 2, -1), kl[t], ke[t]]
    return out


@pytest.mark.parametrize("S,B", [(7, 3), (23, 5), (94, 30), (33, 40), (1, 2), (110, 4)])
def test_eval_mode_matches_torch_restatement(S, B):
    from gan_ffn_amd import ops
    U, qmask = make_inputs(S, B, seed=S * 100 + B + 1)
    m_cpu = build().double().eval()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().eval()
    assert ops.dialogue_rnn_listener_supported(m_gpu.dialogue_cell, U.cuda(), qmask.cuda())
    assert not ops.dialogue_rnn_supported(m_gpu.dialogue_cell, U.cuda(), qmask.cuda())
    compare(m_gpu, m_cpu, U, qmask)          # emotions, alpha, dU, every parameter gradient (l_cell included)
    assert any(".l_cell." in k for k, _ in m_gpu.named_parameters())


@pytest.mark.parametrize("S,B", [(9, 4), (94, 30)])
def test_train_mode_matches_torch_restatement_with_the_same_philox_masks(S, B):
    from gan_ffn_amd import ops
    U, qmask = make_inputs(S, B, seed=S + B + 1)
    p, seed = 0.1, 20261015
    m_cpu = build(dropout=p).double().train()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().train()
    m_cpu.dialogue_cell.dropout = _MaskSeq(listener_masks(S, B, 500, 100, p, seed, 0))
    ops.manual_seed(seed)                       # the call below takes rng offset 0
    compare(m_gpu, m_cpu, U, qmask)


def _formula_bimodel():
    import test_drnn_listener_cpu as L
    return L.listener_model().cuda()


def test_bimodel_matches_reference_fixture_small():
    import test_drnn_listener_cpu as L
    L.check_small(_formula_bimodel(), "cuda", lp_tol=5e-5, du_tol=2e-4, g_tol=5e-4)


def test_bimodel_matches_reference_fixture_at_configuration_5_size():
    import test_drnn_listener_cpu as L
    L.check_big(_formula_bimodel(), "cuda", rtol=1e-4, grtol=1e-3)


def test_hip_path_is_taken(monkeypatch):
    """with the per-step torch cell disabled, a listener BiModel still runs forward and backward on CUDA"""
    from gan_ffn_amd import dialogue_rnn as DR

    def refuse(*a, **k):
        raise AssertionError("DialogueRNNCell.forward called: the listener ran on torch ops")
    torch.manual_seed(4)
    m = DR.BiModel(D_m=100, D_g=500, D_p=500, D_e=100, D_h=100, n_classes=6, context_attention="general", listener_state=True,
                   dropout_rec=0.1, dropout=0.6).cuda().train()
    monkeypatch.setattr(DR.DialogueRNNCell, "forward", refuse)
    U, qmask = make_inputs(13, 4, seed=9)
    umask = (qmask.sum(2) > 0).float().t().contiguous()
    Ug = U.cuda().requires_grad_(True)
    lp = m(Ug, qmask.cuda(), umask.cuda())[0]
    lp.sum().backward()
    assert torch.isfinite(Ug.grad).all()
    lw = m.dialog_rnn_r.dialogue_cell.l_cell.weight_hh.grad
    assert lw is not None and float(lw.abs().max()) > 0


@pytest.mark.parametrize("S,B", [(13, 4), (94, 30)])
def test_engine_step_with_listener_matches_module_path_autograd(S, B):
    """DrnnEngine accepts a listener GAN_FFN_DialogueRNN; dropout off: its step's loss, log-probabilities and every head
    gradient (l_cell included) equal the module path's autograd results, and Adam moves the l_cell tensors state_dict() sees"""
    from gan_ffn_amd import data as D, engine as E, model as M
    from test_hip_drnn_engine import DIMS as EDIMS, W, rel
    torch.manual_seed(3)
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                listener_state=True, context_attention="general", dropout_rec=0.1, dropout=0.6, **EDIMS)
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for g in (net.acoustic_generator, net.visual_generator, net.text_generator):
        g.transformer_encoder.enc_dropout = 0.0
    net = net.cuda().train()
    ref = copy.deepcopy(net)
    b = D.synthetic_batch(B=B, S_max=S, seed=5, device="cuda")
    lp = ref(b["acoustic"], b["visual"], b["text"], b["qmask"], b["umask"])[0]
    loss_ref = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))(lp.transpose(0, 1).contiguous().view(-1, 6), b["label"].view(-1),
                                                               b["umask"])
    loss_ref.backward()
    keys = [k for k in net.state_dict() if ".l_cell." in k]
    assert len(keys) == 8
    before = {k: v.detach().clone() for k, v in net.state_dict().items() if k in keys}
    eng = E.DrnnEngine(net)
    loss, log_prob = eng.step(b, train=True)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 2e-5 * max(1.0, abs(float(loss_ref)))
    assert rel(log_prob, lp) < 1e-4
    refp = dict(ref.named_parameters())
    names = {id(p): n for n, p in net.named_parameters()}
    seen = []
    for i, p in enumerate(eng._hparams):
        g_ref = refp[names[id(p)]].grad
        assert g_ref is not None, names[id(p)]
        assert rel(eng._hp(i, True).view_as(p), g_ref) < 2e-3, names[id(p)]
        seen.append(names[id(p)])
    assert len(seen) == 40 and sum(".l_cell." in k for k in seen) == 8
    after = net.state_dict()
    for k in keys:
        assert float((after[k] - before[k]).abs().max()) > 0, k
