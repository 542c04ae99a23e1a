"""mask_padding on the GPU: the encoder stack with key lengths (ganffn_encoder_fwd_len / _bwd_len), Phase2Engine and DrnnEngine
with mask_padding=True, and the module path, against the fp64 oracle with masked self-attention (tests/key_len_oracle.py) on
the engines' own dropout masks and ReLU patterns.  Bounds: those of tests/test_hip_classifier_engines_train_oracle.py for the
unmasked step — generator outputs and log_prob 1e-4 of scale, gradients 1e-3 of scale.  Each engine test first shows, on the
oracle alone, that its inputs tell the masked function from the unmasked one by more than 10x the bound."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import engine_oracle as EO
from oracle import ganffn_oracle as O
from key_len_oracle import masked_attention, valid_rows
from util import _assert_close, relu_masks
from test_hip_classifier_engines_train_oracle import W, DRNN_LR, DRNN_L2, P2_LR, P2_L2, DIMS, _batch, _host_batch, _gen_slabs
from test_hip_dispatch_range import _encoder_inputs, _encoder_params

pytestmark = pytest.mark.gpu

SEED = 20261019
OUT_TOL, GRAD_TOL = 1e-4, 1e-3
ENGINE_SHAPES = [(7, 2, [7, 1]), (33, 5, [33, 1, 20, 7, 12])]


def _close(got, want, rtol, label, atol=0.0):
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu() if torch.is_tensor(want) else want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    r = _assert_close(got, want, rtol, atol, label, 0.0, 1.0)
    print("%-60s err / scale %.3g (bound %g)" % (label, r, rtol))


# ================================================================================================================
# encoder stacks
# ================================================================================================================
def _encoder_len_run(S, B, E, H, F, L, lengths, use_len=True):
    """the stack forward (saved, train mode) and whole backward on the GPU, with key lengths (ops.encoder_*_raw key_len=) or
    through the plain entry points -> out, dx, gradient slab, saved (device tensors), and the inputs"""
    from gan_ffn_amd import ops
    slab, x, pe, dout = _encoder_inputs(S, B, E, H, F, L)
    cfg = ops.enc_cfg(S, B, E, H, L, F=F, train=True)
    n_saved, n_ws = ops.enc_sizes(cfg)
    f32 = dict(device="cuda", dtype=torch.float32)
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    slab_d, x_d, pe_d = slab.cuda(), x.cuda(), pe.cuda()
    kl = torch.tensor(lengths, dtype=torch.int32, device="cuda") if use_len else None
    out = torch.full((S * B * E,), float("nan"), **f32)
    saved, ws = torch.zeros(n_saved, **f32), torch.zeros(n_ws, **f32)
    ops.encoder_fwd_raw(cfg, x_d, pe_d, slab_d, out, saved, ws, rng, 5, key_len=kl)
    dx = dout.cuda().clone()
    gslab = torch.zeros_like(slab_d)
    ops.encoder_bwd_raw(cfg, 0, L, dx, slab_d, gslab, saved, ws, rng, 5, key_len=kl)
    torch.cuda.synchronize()
    return dict(cfg=cfg, slab=slab, x=x, pe=pe, dout=dout, out=out.view(S, B, E), dx=dx, gslab=gslab, saved=saved)


@pytest.mark.parametrize("E,H,F", [(100, 10, 2048), (512, 8, 2048), (64, 4, 128)])
def test_encoder_stack_with_key_lengths_matches_masked_oracle(E, H, F):
    from gan_ffn_amd import ops
    S, B, L, lengths = 17, 4, 2, [17, 16, 1, 5]
    r = _encoder_len_run(S, B, E, H, F, L, lengths)
    masks = []
    for l in range(L):
        off = int(ops._lib.load().ganffn_encoder_saved_hidden_offset(C.byref(r["cfg"]), l))
        masks.append((r["saved"][off:off + S * B * F] != 0).view(S, B, F).double().cpu())
    P = _encoder_params(r["slab"], r["pe"], E, F, L)
    xo = r["x"].double().requires_grad_(True)
    with masked_attention(lengths):
        yo = O.encoder_stack(xo, P, H, O.Rng(SEED, 5, True), n_layers=L, relu_masks=masks)
    (yo * r["dout"].double()).sum().backward()
    tag = "encoder (%d, %d, %d) " % (E, H, F)
    _close(r["out"], yo.detach(), OUT_TOL, tag + "out")
    _close(r["dx"], xo.grad, GRAD_TOL, tag + "dx", 1e-12)
    per, offs = ops.layer_layout(E, F)
    gs = r["gslab"].cpu()
    for l in range(L):
        for key, o, shape in zip(ops.LAYER_KEYS, offs, ops.layer_shapes(E, F)):
            k = "transformer_encoder.layers.%d.%s" % (l, key)
            _close(gs[l * per + o:l * per + o + int(np.prod(shape))].view(shape), P[k].grad, GRAD_TOL, tag + "grad " + k, 1e-12)
    # the inputs tell the two functions apart
    with torch.no_grad():
        y_plain = O.encoder_stack(r["x"].double(), P, H, O.Rng(SEED, 5, True), n_layers=L, relu_masks=masks)
    valid = valid_rows(S, lengths)
    assert float((y_plain - yo.detach())[valid].abs().max()) > 10 * OUT_TOL * float(yo.detach().abs().max())


@pytest.mark.parametrize("E,H,F", [(100, 10, 2048), (512, 8, 2048), (64, 4, 128)])
def test_encoder_stack_full_lengths_give_the_plain_calls_bits(E, H, F):
    S, B, L = 17, 4, 2
    a = _encoder_len_run(S, B, E, H, F, L, [S] * B)
    b = _encoder_len_run(S, B, E, H, F, L, None, use_len=False)
    for k in ("out", "dx", "gslab", "saved"):
        # (compared as bit patterns: the saved block also holds keep words and ReLU pattern bits, NaNs when read as floats)
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ================================================================================================================
# engines
# ================================================================================================================
def _phase2_engine(mask_padding, seed=11, lr=P2_LR, dropout_off=False):
    from gan_ffn_amd import engine as E, model
    gens, _ = E.build_networks(device="cuda", seed=seed)
    net = model.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, mask_padding=mask_padding).cuda()
    if dropout_off:
        _dropout_off(net)
    return net, E.Phase2Engine(net, lr=lr, weight_decay=P2_L2, class_weights=W, mask_padding=mask_padding)


# the network seed: the eval step's DialogueRNN head (no dropout, so no 1 / (1 - p) factors) moves its log_prob little for the ONE
# padded dialogue of the (7, 2, [7, 1]) batch — 3.5x to 18x the bound over some 50 network seeds on the CPU, about 9x typically, and
# the Adam step between the test's train and eval step moves it again (seed 33: 22x before that step, 10.6x after).  Seed 44, from a
# CPU search that applies the train step's fp64 Adam update before it evaluates the eval step: (7, 2) train 56x, eval 18x; (33, 5)
# train 106x, eval 19x — the 10x condition holds in every step of the test with room
def _drnn_engine(mask_padding, seed=44):
    from gan_ffn_amd import engine as E, model as M
    torch.manual_seed(seed)
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                listener_state=False, context_attention="general", dropout_rec=0.1, dropout=0.6,
                                mask_padding=mask_padding, **DIMS).cuda().train()
    return net, E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W, mask_padding=mask_padding)


def _dropout_off(net):
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for g in (net.acoustic_generator, net.visual_generator, net.text_generator):
        g.transformer_encoder.enc_dropout = 0.0


def _p2_batch(batch):
    return {k: batch[k] for k in ("acoustic", "visual", "text", "umask", "label")}


def _scale(t):
    return float(t.abs().max())


def _assert_discriminates(masked, plain, valid, what="log_prob"):
    """a condition on the inputs: at valid positions the unmasked oracle's value is further from the masked one's than 10x
    the bound the engine is held to — an engine that ignored the lengths could not pass"""
    gap = float((masked - plain)[valid].abs().max())
    bound = OUT_TOL * _scale(masked)
    print("masked vs unmasked oracle %s at valid positions: %.3g = %.3g x bound" % (what, gap, gap / bound))
    assert gap > 10 * bound, (what, gap, bound)


def _check_generators(eng, pre, hb, lens, b, train, S, B, tag):
    """generator outputs (and, in train mode, every generator gradient from the engine's dL/dfusion) against the masked oracle"""
    gens = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"], requires_grad=train) for i, k in enumerate(EO.GEN_KEYS)}
    masks_g = {k: relu_masks(eng.pass_G[k], eng.pass_G[k].cfg_train, S, B) for k in EO.GEN_KEYS} if train else None
    with masked_attention(lens):
        if train:
            outs = EO.generators(gens, hb, SEED, EO.gen_adds(b), masks_g)
        else:
            with torch.no_grad():
                outs = EO.generators(gens, hb, SEED, None)
    for k in EO.GEN_KEYS:
        _close(eng.pass_G[k].out, outs[k].detach(), OUT_TOL, "%s %s output" % (tag, k))
    return gens, outs


def _check_generator_grads(eng, gens, outs, d_fusion, tag):
    gg = EO.generator_grads(gens, outs, d_fusion)
    for k in EO.GEN_KEYS:
        g = eng.G[k].grad.cpu()
        for n, (o, shape) in eng.G[k].named.items():
            _close(g[o:o + int(np.prod(shape))].view(*shape), gg[k][n], GRAD_TOL, "%s %s grad %s" % (tag, k, n), 1e-12)


def _oracle_gen_sum(slabs, eng, hb, adds, lens):
    """fusion of the oracle's own chain from the raw modalities, masked (lens) or not (None)"""
    gens = {k: EO.Net.from_state(eng.G[k], slabs[i]["slab"], requires_grad=False) for i, k in enumerate(EO.GEN_KEYS)}
    with torch.no_grad():
        if lens is None:
            outs = EO.generators(gens, hb, SEED, adds)
        else:
            with masked_attention(lens):
                outs = EO.generators(gens, hb, SEED, adds)
    return outs["acoustic"] + outs["visual"] + outs["text"]


@pytest.mark.parametrize("S,B,lens", ENGINE_SHAPES, ids=["7x2", "33x5"])
def test_phase2_engine_mask_padding_train_and_eval_match_masked_oracle(S, B, lens):
    from gan_ffn_amd import ops
    net, eng = _phase2_engine(True)
    slabs = _gen_slabs(eng, P2_LR, P2_L2)
    batch = _p2_batch(_batch(S, B, 31 * S + B, lens=lens))
    hb = _host_batch(batch)
    valid = valid_rows(S, lens)
    ops.manual_seed(SEED)
    for train in (True, False):
        tag = "phase2 (%d, %d) %s" % (S, B, "train" if train else "eval")
        torch.cuda.synchronize()
        pre = [sl.host() for sl in slabs]
        fc = eng.fc_slab.cpu().clone()
        nw, C_ = eng.fc_w.numel(), eng.n_classes
        fc_w, fc_b = fc[:nw].view(C_, 100), fc[eng.fc_off_b:eng.fc_off_b + C_]
        eng.step(batch, train=train)
        torch.cuda.synchronize()
        b = eng._base_add
        # the inputs: masked and unmasked oracle differ
        adds = EO.gen_adds(b) if train else None
        fus_m, fus_u = _oracle_gen_sum(pre, eng, hb, adds, lens), _oracle_gen_sum(pre, eng, hb, adds, None)
        _assert_discriminates(fus_m, fus_u, valid, "fusion")
        lp_m = torch.log_softmax(fus_m @ fc_w.double().T + fc_b.double(), 2)
        lp_u = torch.log_softmax(fus_u @ fc_w.double().T + fc_b.double(), 2)
        _assert_discriminates(lp_m, lp_u, valid)
        gens, outs = _check_generators(eng, pre, hb, lens, b, train, S, B, tag)
        res = EO.phase2_head(eng.fusion.cpu().double(), fc_w, fc_b, hb["label"], hb["umask"], W)
        _close(eng.log_prob, res["log_prob"], OUT_TOL, tag + " log_prob")
        if train:
            d_fusion = eng.d_fusion.cpu().double()
            _close(d_fusion, res["d_fusion"], GRAD_TOL, tag + " d_fusion", 1e-12)
            _check_generator_grads(eng, gens, outs, d_fusion, tag)


@pytest.mark.parametrize("S,B,lens", ENGINE_SHAPES, ids=["7x2", "33x5"])
def test_drnn_engine_mask_padding_train_and_eval_match_masked_oracle(S, B, lens):
    from gan_ffn_amd import ops
    net, eng = _drnn_engine(True)
    batch = _batch(S, B, 100 * S + B, lens=lens)
    hb = _host_batch(batch)
    valid = valid_rows(S, lens)
    bm = copy.deepcopy(net.bi_model).cpu().double()
    names = {id(p): n for n, p in net.named_parameters()}
    hnames = [names[id(p)][len("bi_model."):] for p in eng._hparams]
    slabs = _gen_slabs(eng, DRNN_LR, DRNN_L2)
    ops.manual_seed(SEED)
    for train in (True, False):
        tag = "drnn (%d, %d) %s" % (S, B, "train" if train else "eval")
        torch.cuda.synchronize()
        pre = [sl.host() for sl in slabs]
        hs = eng.h_slab.cpu().clone()
        params = dict(bm.named_parameters())
        with torch.no_grad():
            for n, o, p in zip(hnames, eng._hoffs, eng._hparams):
                params[n].copy_(hs[o:o + p.numel()].view(p.shape).double())
        eng.step(batch, train=train)
        torch.cuda.synchronize()
        b = eng._base_add
        T, f = S * B, eng._f
        Dm, Dh2, Cn = eng.Dm, eng.Dh2, eng.n_classes
        e_fusion = f["fusion"][:T * Dm].view(S, B, Dm).cpu().double()
        e_hidden = f["hidden"][:T * Dh2].view(S, B, Dh2).cpu().double()
        e_lp = f["log_prob"][:T * Cn].view(S, B, Cn).cpu().double()
        masks = EO.drnn_masks(bm, S, B, SEED, b + EO.A_REC, b + EO.A_HEAD) if train else None
        # the inputs: the oracle's own chain, masked and unmasked
        adds = EO.gen_adds(b) if train else None
        heads, fus = {}, {}
        for key, ln in (("masked", lens), ("plain", None)):
            fus[key] = _oracle_gen_sum(pre, eng, hb, adds, ln)
            heads[key] = EO.drnn_head(bm, fus[key], hb["qmask"], hb["umask"], hb["label"], W, masks)["log_prob"]
        _assert_discriminates(fus["masked"], fus["plain"], valid, "fusion")
        _assert_discriminates(heads["masked"], heads["plain"], valid)
        gens, outs = _check_generators(eng, pre, hb, lens, b, train, S, B, tag)
        res = EO.drnn_head(bm, e_fusion, hb["qmask"], hb["umask"], hb["label"], W, masks, e_hidden > 0)
        _close(e_lp, res["log_prob"], OUT_TOL, tag + " log_prob")
        if train:
            d_fusion = f["dU_f"][:T * Dm].view(S, B, Dm).cpu().double()
            _close(d_fusion, res["d_fusion"], GRAD_TOL, tag + " d_fusion", 1e-12)
            _check_generator_grads(eng, gens, outs, d_fusion, tag)


def _engine_state(eng, kind):
    slabs = {}
    for k, st in eng.G.items():
        slabs.update({k + ".slab": st.slab, k + ".m": st.exp_avg, k + ".v": st.exp_avg_sq, k + ".step": st.step})
    if kind == "phase2":
        slabs.update({"fc.slab": eng.fc_slab, "fc.m": eng.fc_m, "fc.v": eng.fc_v, "fc.step": eng.fc_step})
    else:
        slabs.update({"head.slab": eng.h_slab, "head.m": eng.h_m, "head.v": eng.h_v, "head.step": eng.h_step})
    return {k: v.detach().clone() for k, v in slabs.items()}


def _train_step(kind, mask_padding, batch):
    from gan_ffn_amd import ops
    net, eng = (_phase2_engine if kind == "phase2" else _drnn_engine)(mask_padding)
    ops.manual_seed(SEED)
    loss, lp = eng.step(_p2_batch(batch) if kind == "phase2" else batch, train=True)
    torch.cuda.synchronize()
    return loss.detach().clone(), lp.detach().clone(), _engine_state(eng, kind)


@pytest.mark.parametrize("kind", ["phase2", "drnn"])
def test_engine_with_full_lengths_gives_the_unmasked_engines_bits(kind):
    S, B = 7, 2
    batch = _batch(S, B, 5, lens=[S, S])
    assert bool((batch["umask"] == 1).all())
    la, lpa, sa = _train_step(kind, True, batch)
    lb, lpb, sb = _train_step(kind, False, batch)
    assert torch.equal(la, lb) and torch.equal(lpa, lpb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("kind", ["phase2", "drnn"])
def test_engine_padded_values_change_no_bit(kind):
    S, B, lens = 17, 3, [17, 5, 1]
    batch = _batch(S, B, 77, lens=lens)
    other = dict(batch)
    pad = (~valid_rows(S, lens)).cuda().unsqueeze(2)
    g = torch.Generator().manual_seed(1)
    for k in ("acoustic", "visual", "text"):
        other[k] = torch.where(pad, (torch.rand(batch[k].shape, generator=g) * 3.0 - 1.0).cuda(), batch[k])
        assert not torch.equal(other[k], batch[k])
    la, lpa, sa = _train_step(kind, True, batch)
    lb, lpb, sb = _train_step(kind, True, other)
    valid = valid_rows(S, lens).cuda()
    assert torch.equal(la, lb)
    assert torch.equal(lpa[valid], lpb[valid])
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("kind", ["phase2", "drnn"])
def test_a_dialogue_in_a_padded_batch_is_predicted_as_if_alone(kind):
    """eval mode.  Each side is within 1e-4 of scale of the same fp64 value, so the two are within 2e-4 of each other"""
    S, lens = 17, [17, 5, 1]
    B = len(lens)
    batch = _batch(S, B, 123, lens=lens, single=0)
    build = _phase2_engine if kind == "phase2" else _drnn_engine
    lp = {}
    for mp in (True, False):
        net, eng = build(mp)
        net.eval()
        feed = (lambda d: _p2_batch(d)) if kind == "phase2" else (lambda d: d)
        full = eng.step(feed(batch), train=False)[1].detach().clone()
        alone = []
        for b_, n in enumerate(lens):
            one = {k: (v[:n, b_:b_ + 1] if k in ("acoustic", "visual", "text", "qmask") else v[b_:b_ + 1, :n]).contiguous()
                   for k, v in batch.items()}
            alone.append(eng.step(feed(one), train=False)[1].detach().clone())
        torch.cuda.synchronize()
        lp[mp] = (full, alone)
    scale = _scale(lp[True][0][valid_rows(S, lens).cuda()])
    for b_, n in enumerate(lens):
        d_m = float((lp[True][0][:n, b_] - lp[True][1][b_][:, 0]).abs().max())
        d_u = float((lp[False][0][:n, b_] - lp[False][1][b_][:, 0]).abs().max())
        print("%s dialogue %d (length %d): in the batch vs alone, masked %.3g, unmasked %.3g (scale %.3g)" % (kind, b_, n, d_m, d_u, scale))
        assert d_m < 2 * OUT_TOL * scale, (b_, n, d_m, scale)


def test_module_path_with_mask_padding_matches_the_engine():
    """GAN_FFN(mask_padding=True) under autograd against Phase2Engine(mask_padding=True), dropout off (both then compute the same
    function); bounds of tests/test_hip_drnn_engine.py::test_engine_step_matches_module_path_autograd"""
    from gan_ffn_amd import model as M
    S, B, lens = 17, 4, [17, 16, 1, 5]
    batch = _p2_batch(_batch(S, B, 9, lens=lens))
    net, eng = _phase2_engine(True, dropout_off=True)
    net.train()
    ref = copy.deepcopy(net)
    lp = ref(batch["acoustic"], batch["visual"], batch["text"], batch["umask"])[0]
    loss_ref = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))(lp.transpose(0, 1).contiguous().view(-1, 6), batch["label"].view(-1),
                                                              batch["umask"])
    loss_ref.backward()
    loss, log_prob = eng.step(batch, train=True)
    torch.cuda.synchronize()

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    assert abs(float(loss) - float(loss_ref)) < 2e-5 * max(1.0, abs(float(loss_ref)))
    assert rel(log_prob, lp) < 1e-4
    refp = dict(ref.named_parameters())
    for k, pre in (("acoustic", "acoustic_generator."), ("visual", "visual_generator."), ("text", "text_generator.")):
        st = eng.G[k]
        for name in st.named:
            assert rel(st.w(name, True).view_as(refp[pre + name]), refp[pre + name].grad) < 2e-3, (k, name)
    # and the unmasked module is a different function on this batch
    plain = copy.deepcopy(ref)
    plain.mask_padding = False
    with torch.no_grad():
        lp_u = plain(batch["acoustic"], batch["visual"], batch["text"])[0]
    valid = valid_rows(S, lens).cuda()
    assert float((lp_u - lp)[valid].abs().max()) > 10 * 1e-4 * float(lp.abs().max())
