"""The multi-party DialogueRNN (qmask [S x B x P], model.py:861-926; MELD's 9 speakers) on the HIP recurrence
(csrc/dialogue_rnn.hip through ganffn_drnn_party_fwd / _bwd): against the fp64 torch restatement on the CPU in eval mode and
in train mode with the same Philox masks (the listener's site 11 + 4z mask is P·H wide), every context attention type,
BiModel against the reference's own fixture, the proof that the HIP path (not the per-step torch cell) runs, the party entry
points at P = 2 bit for bit against the two-party ones, and DrnnEngine at P = 9 (against autograd, against the fp64 oracle
with dropout, and its refusal beyond the limit)."""
import copy
import ctypes as C

import pytest
import torch

from gan_ffn_amd.ops import DRNN_MAX_PARTIES        # (a tree without the party axis fails here, before any launch)
from oracle import philox
from test_hip_drnn_kernel import _MaskSeq, compare

pytestmark = pytest.mark.gpu

DIMS = dict(D_m=100, D_g=500, D_p=500, D_e=100)
ATT_DIMS = {"general": {}, "simple": {}, "dot": dict(D_g=100, D_p=100), "general2": {}, "concat": dict(D_a=100)}


def make_inputs(S, B, P, seed, Dm=100):
    """ragged batch, one-hot speakers over P parties (party P - 1 never speaks for P >= 3; dialogue 1 has one speaker),
    zero rows on padding"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(1, S // 3), S + 1, (B,), generator=g)
    lens[0] = S
    valid = (torch.arange(S).unsqueeze(1) < lens.unsqueeze(0)).float()            # (S, B)
    U = (torch.rand(S, B, Dm, generator=g) - 0.3) * valid.unsqueeze(2)
    spk = torch.randint(0, P - 1 if P >= 3 else P, (S, B), generator=g)
    if B > 1:
        spk[:, 1] = spk[0, 1]
    qmask = torch.nn.functional.one_hot(spk, P).float() * valid.unsqueeze(2)
    return U, qmask


def build(listener=False, att="general", seed=7, dropout=0.1):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    d = dict(DIMS)
    d.update(ATT_DIMS[att])
    m = DR.DialogueRNN(context_attention=att, listener_state=listener, dropout=dropout, **d)
    with torch.no_grad():                       # livelier recurrent weights than the default init
        for n, p in m.named_parameters():
            p.mul_(1.5)
            if n == "dialogue_cell.attention.transform.weight" and att == "general2":
                p.mul_(4.0)
    return m


def party_masks(S, B, H, He, p, seed, offset, P, listener, direction=0):
    """the cell's dropout calls per step in order as the HIP recurrence draws them: g (B,H) site 8; qs (B,P,H) site 9, one
    row of width H shared by the party rows; with listener state ql (B,P,H) site 11, one row of width P·H; e (B,He) site 10
    (+ 4 per direction)"""
    def keep(cols, site):
        return torch.from_numpy(philox.keep_mask(S * B, cols, p, site + 4 * direction, seed, offset)).double() / (1 - p)
    kg, kp, ke = keep(H, 8).view(S, B, H), keep(H, 9).view(S, B, H), keep(He, 10).view(S, B, He)
    kl = keep(P * H, 11).view(S, B, P, H) if listener else None
    out = []
    for t in range(S):
        out += [kg[t], kp[t].unsqueeze(1).expand(-1, P, -1)] + ([kl[t]] if listener else []) + [ke[t]]
    return out


@pytest.mark.parametrize("S,B", [(7, 3), (33, 32), (94, 30), (33, 40)])
@pytest.mark.parametrize("listener", [False, True])
@pytest.mark.parametrize("P", [1, 3, 9, DRNN_MAX_PARTIES])
def test_eval_mode_matches_torch_restatement(P, listener, S, B):
    from gan_ffn_amd import ops
    U, qmask = make_inputs(S, B, P, seed=S * 100 + B + P)
    m_cpu = build(listener).double().eval()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().eval()
    pred = ops.dialogue_rnn_listener_supported if listener else ops.dialogue_rnn_supported
    assert pred(m_gpu.dialogue_cell, U.cuda(), qmask.cuda())
    compare(m_gpu, m_cpu, U, qmask)          # emotions, alpha, dU, every parameter gradient


@pytest.mark.parametrize("S,B", [(9, 4), (94, 30)])
@pytest.mark.parametrize("listener", [False, True])
def test_train_mode_matches_torch_restatement_with_the_same_philox_masks(listener, S, B):
    from gan_ffn_amd import ops
    P = 9
    U, qmask = make_inputs(S, B, P, seed=S + B + 9)
    p, seed = 0.1, 20261016
    m_cpu = build(listener, dropout=p).double().train()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().train()
    m_cpu.dialogue_cell.dropout = _MaskSeq(party_masks(S, B, 500, 100, p, seed, 0, P, listener))
    ops.manual_seed(seed)                       # the call below takes rng offset 0
    compare(m_gpu, m_cpu, U, qmask)


@pytest.mark.parametrize("listener", [False, True])
@pytest.mark.parametrize("att", list(ATT_DIMS))
def test_every_attention_type_at_nine_parties(att, listener):
    U, qmask = make_inputs(13, 5, 9, seed=31)
    m_cpu = build(listener, att).double().eval()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().eval()
    compare(m_gpu, m_cpu, U, qmask)


def _fixture_model(case):
    import test_drnn_parties_cpu as X
    return X.party_model(case).cuda()


@pytest.mark.parametrize("case,P", [("general", 1), ("general", 9), ("general_listener", 3), ("concat_listener", 9), ("simple", 3)])
def test_bimodel_matches_reference_fixture_small(case, P):
    import test_drnn_parties_cpu as X
    X.check_small(_fixture_model(case), case, P, "cuda", lp_tol=5e-5, du_tol=2e-4, g_tol=5e-4)


def test_bimodel_matches_reference_fixture_at_meld_size():
    import test_drnn_parties_cpu as X
    X.check_big(_fixture_model("general"), "cuda", rtol=1e-4, grtol=1e-3)


@pytest.mark.parametrize("listener", [False, True])
def test_hip_path_is_taken(listener, monkeypatch):
    """with the per-step torch cell disabled, a nine-party BiModel still runs forward and backward on CUDA"""
    from gan_ffn_amd import dialogue_rnn as DR

    def refuse(*a, **k):
        raise AssertionError("DialogueRNNCell.forward called: the recurrence ran on torch ops")
    torch.manual_seed(4)
    m = DR.BiModel(D_m=100, D_g=500, D_p=500, D_e=100, D_h=100, n_classes=7, context_attention="general", listener_state=listener,
                   dropout_rec=0.1, dropout=0.6).cuda().train()
    monkeypatch.setattr(DR.DialogueRNNCell, "forward", refuse)
    U, qmask = make_inputs(13, 4, 9, seed=9)
    umask = (qmask.sum(2) > 0).float().t().contiguous()
    Ug = U.cuda().requires_grad_(True)
    lp = m(Ug, qmask.cuda(), umask.cuda())[0]
    lp.sum().backward()
    assert torch.isfinite(Ug.grad).all() and float(Ug.grad.abs().max()) > 0
    w = m.dialog_rnn_r.dialogue_cell.p_cell.weight_hh.grad
    assert w is not None and float(w.abs().max()) > 0


def _run_direct(cell, U, qmask, gy, party, train):
    """one direction through the C entry points, forward and backward: the party ones with parties = 2, or the two-party
    ones ops uses at P = 2 (ganffn_drnn_* / _listener_* for general, ganffn_drnn_att_* otherwise) -> list of outputs"""
    from gan_ffn_amd import _lib, ops
    att, listener = ops.drnn_att_type(cell), bool(cell.listener_state)
    Ux, params = ops._drnn_cell_args(cell, U)
    Ux, params = Ux.contiguous(), [p.detach().contiguous() for p in params]
    S, B, Dm = Ux.shape
    n_att = len(ops.DRNN_ATT_KEYS[att])
    prm = params[:12] + ([params[12]] if att == "general" else [None])
    aprm = params[12:12 + n_att]
    lprm = params[12 + n_att:] if listener else None
    spk64 = torch.argmax(qmask, 2)
    mval = qmask.gather(2, spk64.unsqueeze(2)).squeeze(2).contiguous()
    spk = spk64.to(torch.int32).contiguous()
    p = float(cell.dropout.p) if train else 0.0
    cfg = _lib.DrnnCfg(S, B, Dm, cell.D_g, cell.D_e, p, 1 if train else 0)
    acfg = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], int(cell.attention.transform.weight.shape[0]) if att == "concat" else 0)
    lib = _lib.load()
    if party:
        ns = lib.ganffn_drnn_party_saved_floats(C.byref(cfg), C.byref(acfg), int(listener), 2)
        nw = lib.ganffn_drnn_party_workspace_floats(C.byref(cfg), C.byref(acfg), int(listener), 2)
    else:
        ns = lib.ganffn_drnn_att_saved_floats(C.byref(cfg), C.byref(acfg), int(listener))
        nw = lib.ganffn_drnn_att_workspace_floats(C.byref(cfg), C.byref(acfg), int(listener))
    dev = U.device
    sv, ws = torch.empty(ns, device=dev), torch.empty(nw, device=dev)
    e, al = torch.empty(S, B, cell.D_e, device=dev), torch.empty(B, S, S, device=dev)
    A = ops._ptr_array
    P1 = (_lib.DrnnPtrs * 1)(ops._drnn_ptrs(prm))
    LP = (_lib.DrnnListenerPtrs * 1)(ops._drnn_ptrs(lprm, _lib.DrnnListenerPtrs)) if listener else None
    AP = (_lib.DrnnAttPtrs * 1)(ops._att_ptrs(att, aprm))
    rng = ops.DeviceRng.get(dev).state
    ops.manual_seed(20261016)
    tail = (A([e]), A([al]), A([sv]), A([ws]), ops._ptr(rng), C.c_uint64(0), ops._stream())
    head = (A([Ux]), A([spk]), A([mval]), P1)
    if party:
        _lib.call("ganffn_drnn_party_fwd", C.byref(cfg), C.byref(acfg), 2, 1, *head, LP, AP, *tail)
    elif att == "general" and not listener:
        _lib.call("ganffn_drnn_fwd", C.byref(cfg), 1, *head, *tail)
    elif att == "general":
        _lib.call("ganffn_drnn_listener_fwd", C.byref(cfg), 1, *head, LP, *tail)
    else:
        _lib.call("ganffn_drnn_att_fwd", C.byref(cfg), C.byref(acfg), 1, *head, LP, AP, *tail)
    dU = torch.empty_like(Ux)
    grads = [torch.zeros_like(t) if t is not None else None for t in prm]
    agr = [grads[12]] if att == "general" else [torch.zeros_like(t) for t in aprm]
    lgr = [torch.zeros_like(t) for t in lprm] if listener else []
    G1 = (_lib.DrnnPtrs * 1)(ops._drnn_ptrs(grads))
    AG = (_lib.DrnnAttPtrs * 1)(ops._att_ptrs(att, agr))
    LG = (_lib.DrnnListenerPtrs * 1)(ops._drnn_ptrs(lgr, _lib.DrnnListenerPtrs)) if listener else None
    btail = (A([dU]), A([al]), A([sv]), A([ws]), ops._ptr(rng), C.c_uint64(0), ops._stream())
    bhead = (A([gy.contiguous()]), A([Ux]), A([spk]), A([mval]), P1)
    if party:
        _lib.call("ganffn_drnn_party_bwd", C.byref(cfg), C.byref(acfg), 2, 1, *bhead, LP, AP, G1, LG, AG, *btail)
    elif att == "general" and not listener:
        _lib.call("ganffn_drnn_bwd", C.byref(cfg), 1, *bhead, G1, *btail)
    elif att == "general":
        _lib.call("ganffn_drnn_listener_bwd", C.byref(cfg), 1, *bhead, LP, G1, LG, *btail)
    else:
        _lib.call("ganffn_drnn_att_bwd", C.byref(cfg), C.byref(acfg), 1, *bhead, LP, AP, G1, LG, AG, *btail)
    torch.cuda.synchronize()
    return [e, al, dU] + [g for g in grads if g is not None] + ([] if att == "general" else agr) + lgr


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("att,listener", [("general", False), ("general", True), ("concat", True), ("general2", False)])
def test_party_entry_points_at_two_parties_equal_the_two_party_ones(att, listener, train):
    m = build(listener, att).cuda()
    U, qmask = make_inputs(23, 6, 2, seed=5)
    U, qmask = U.cuda(), qmask.cuda()
    gy = (torch.rand(23, 6, 100, generator=torch.Generator().manual_seed(2)) - 0.5).cuda()
    with torch.no_grad():
        old = _run_direct(m.dialogue_cell, U, qmask, gy, False, train)
        new = _run_direct(m.dialogue_cell, U, qmask, gy, True, train)
    assert len(old) == len(new) >= 15
    for i, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), i
    assert float(old[2].abs().max()) > 0


# ---- DrnnEngine --------------------------------------------------------------------------------------------------------
def _party_batch(S, B, P, seed):
    from gan_ffn_amd import data as D
    b = {k: v for k, v in D.synthetic_batch(B=B, S_max=S, seed=seed, device="cuda").items() if torch.is_tensor(v)}
    spk = torch.randint(0, P - 1 if P >= 3 else P, (S, B), generator=torch.Generator().manual_seed(seed))
    b["qmask"] = torch.nn.functional.one_hot(spk, P).float().cuda() * b["umask"].t().unsqueeze(2)    # the batch's padding
    return b


def _engine_net(listener, dropout_off):
    from gan_ffn_amd import model as M
    from test_hip_drnn_engine import DIMS as EDIMS
    torch.manual_seed(3)
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                listener_state=listener, context_attention="general", dropout_rec=0.1, dropout=0.6, **EDIMS)
    if dropout_off:
        for mod in net.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        for g in (net.acoustic_generator, net.visual_generator, net.text_generator):
            g.transformer_encoder.enc_dropout = 0.0
    return net.cuda().train()


@pytest.mark.parametrize("listener", [False, True])
@pytest.mark.parametrize("S,B", [(13, 4), (94, 30)])
def test_engine_step_at_nine_parties_matches_module_path_autograd(S, B, listener):
    """dropout off: the engine step's loss, log-probabilities and every head gradient equal the module path's autograd
    results on a nine-party batch; a two-party batch after it re-uses the same slab"""
    from gan_ffn_amd import engine as E, model as M
    from test_hip_drnn_engine import W, rel
    net = _engine_net(listener, True)
    ref = copy.deepcopy(net)
    b = _party_batch(S, B, 9, seed=5)
    lp = ref(b["acoustic"], b["visual"], b["text"], b["qmask"], b["umask"])[0]
    loss_ref = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))(lp.transpose(0, 1).contiguous().view(-1, 6), b["label"].view(-1),
                                                               b["umask"])
    loss_ref.backward()
    eng = E.DrnnEngine(net)
    loss, log_prob = eng.step(b, train=True)
    torch.cuda.synchronize()
    assert eng._shape == (S, B, 9)
    assert abs(float(loss) - float(loss_ref)) < 2e-5 * max(1.0, abs(float(loss_ref)))
    assert rel(log_prob, lp) < 1e-4
    refp = dict(ref.named_parameters())
    names = {id(p): n for n, p in net.named_parameters()}
    for i, p in enumerate(eng._hparams):
        g_ref = refp[names[id(p)]].grad
        assert g_ref is not None, names[id(p)]
        assert rel(eng._hp(i, True).view_as(p), g_ref) < 2e-3, names[id(p)]
    assert len(eng._hparams) == (40 if listener else 32)
    # a two-party batch next: the same engine, the two-party entry points, a finite loss
    loss2, _ = eng.step(_party_batch(S, B, 2, seed=6), train=True)
    torch.cuda.synchronize()
    assert eng._shape == (S, B, 2) and bool(torch.isfinite(loss2).all())


@pytest.mark.parametrize("listener", [False, True])
def test_engine_train_step_with_dropout_at_nine_parties_matches_fp64_oracle(listener, monkeypatch):
    """dropout on: the engine step against tests/engine_oracle.drnn_step with the engine's Philox masks restated for P
    parties (engine_oracle.rec_masks is two-party), on the engine's ReLU patterns"""
    import engine_oracle as EO
    from gan_ffn_amd import engine as E, ops
    from test_hip_classifier_engines_train_oracle import DRNN_L2, DRNN_LR, SEED, W, _close, _host_batch
    from util import relu_masks
    S, B, P = 13, 4, 9
    monkeypatch.setattr(EO, "rec_masks", lambda S_, B_, H, He, p, seed, off, z, lis: party_masks(S_, B_, H, He, p, seed, off, P, lis, z))
    net = _engine_net(listener, False)
    eng = E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W)
    bm = copy.deepcopy(net.bi_model).cpu().double()
    pre = {k: eng.G[k].slab.cpu().clone() for k in EO.GEN_KEYS}
    batch = _party_batch(S, B, P, seed=100 * S + B)
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
    tag = "P = 9%s" % (" listener" if listener else "")
    assert abs(float(loss) - ch["loss"]) < 2e-5 * abs(ch["loss"]), (float(loss), ch["loss"])
    _close("log_prob", f["log_prob"][:T * 6].view(S, B, 6).cpu().double(), ch["log_prob"], 1e-4, 0.0, tag + " log_prob")
    hg = eng.h_grad.cpu()
    names = {id(p): n for n, p in net.named_parameters()}
    for o, p in zip(eng._hoffs, eng._hparams):
        n = names[id(p)][len("bi_model."):]
        _close("head gradient", hg[o:o + p.numel()].view(p.shape).double(), ch["grads"][n], 1e-3, 1e-12, "%s grad %s" % (tag, n))


def test_engine_refuses_more_parties_than_the_kernels_take():
    from gan_ffn_amd import engine as E
    net = _engine_net(False, True)
    eng = E.DrnnEngine(net)
    b = _party_batch(13, 4, 2, seed=1)
    b["qmask"] = torch.zeros(13, 4, DRNN_MAX_PARTIES + 1, device="cuda")
    b["qmask"][:, :, DRNN_MAX_PARTIES] = b["umask"].t()
    with pytest.raises(ValueError, match="ops.DRNN_MAX_PARTIES"):
        eng.step(b, train=True)
    assert eng._shape is None                          # refused before any buffer or launch
