"""causal on the GPU: the encoder stack with GANFFN_ATTN_CAUSAL (ganffn_encoder_fwd_mask / _bwd_mask), Phase2Engine with
causal=True (alone and with mask_padding=True) and the module path, against the fp64 oracle with causal self-attention
(tests/causal_oracle.py) on the engine's own dropout masks and ReLU patterns.  Harness and bounds: those of
tests/test_hip_key_len_engines.py — generator outputs and log_prob 1e-4 of scale, gradients 1e-3 of scale.  Each engine step first
shows, on the oracle alone, that its inputs tell the causal function from the bidirectional one by more than 10x the bound."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import engine_oracle as EO
from oracle import ganffn_oracle as O
from causal_oracle import causal_attention
from key_len_oracle import masked_attention, valid_rows
from util import relu_masks
from test_hip_classifier_engines_train_oracle import W, P2_LR, P2_L2, _batch, _host_batch, _gen_slabs
from test_hip_dispatch_range import _encoder_inputs, _encoder_params
from test_hip_key_len_engines import OUT_TOL, GRAD_TOL, _close, _check_generator_grads, _dropout_off, _p2_batch, _scale

pytestmark = pytest.mark.gpu

SEED = 20261019
# (50, 2): head_dim 64 of the visual generator on the 32-row kernels (S > 48)
ENGINE_SHAPES = [(7, 2, [7, 1]), (33, 5, [33, 1, 20, 7, 12]), (50, 2, [50, 3])]


# ================================================================================================================
# encoder stacks
# ================================================================================================================
def _encoder_run(S, B, E, H, F, L, lengths, causal=True, entry="ops"):
    """the stack forward (saved, train mode) and whole backward on the GPU -> out, dx, gradient slab, saved, and the inputs.
    entry="ops": ops.encoder_*_raw(key_len=, causal=); "mask0": the _mask entry points with flags = 0; "len": the _len ones."""
    from gan_ffn_amd import ops
    slab, x, pe, dout = _encoder_inputs(S, B, E, H, F, L)
    cfg = ops.enc_cfg(S, B, E, H, L, F=F, train=True)
    n_saved, n_ws = ops.enc_sizes(cfg)
    f32 = dict(device="cuda", dtype=torch.float32)
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    slab_d, x_d, pe_d = slab.cuda(), x.cuda(), pe.cuda()
    kl = torch.tensor(lengths, dtype=torch.int32, device="cuda") if lengths is not None else None
    out = torch.full((S * B * E,), float("nan"), **f32)
    saved, ws = torch.zeros(n_saved, **f32), torch.zeros(n_ws, **f32)
    dx = dout.cuda().clone()
    gslab = torch.zeros_like(slab_d)
    p, st = ops._ptr, ops._stream
    if entry == "ops":
        ops.encoder_fwd_raw(cfg, x_d, pe_d, slab_d, out, saved, ws, rng, 5, key_len=kl, causal=causal)
        ops.encoder_bwd_raw(cfg, 0, L, dx, slab_d, gslab, saved, ws, rng, 5, key_len=kl, causal=causal)
    else:
        fl = (C.c_uint32(0),) if entry == "mask0" else ()
        name = "mask" if entry == "mask0" else "len"
        ops._lib.call("ganffn_encoder_fwd_" + name, C.byref(cfg), p(kl), *fl, p(x_d), p(pe_d), p(slab_d), p(out), p(saved), p(ws),
                      p(rng), C.c_uint64(5), st())
        ops._lib.call("ganffn_encoder_bwd_" + name, C.byref(cfg), p(kl), *fl, 0, L, p(dx), p(slab_d), p(gslab), p(saved), p(ws),
                      p(rng), C.c_uint64(5), 1, st())
    torch.cuda.synchronize()
    return dict(cfg=cfg, slab=slab, x=x, pe=pe, dout=dout, out=out.view(S, B, E), dx=dx, gslab=gslab, saved=saved)


@pytest.mark.parametrize("lengths", [None, [17, 16, 1, 5]], ids=["no_lengths", "lengths"])
@pytest.mark.parametrize("E,H,F", [(100, 10, 2048), (512, 8, 2048), (64, 4, 128)])
def test_encoder_stack_causal_matches_causal_oracle(E, H, F, lengths):
    from gan_ffn_amd import ops
    S, B, L = 17, 4, 2
    r = _encoder_run(S, B, E, H, F, L, lengths)
    masks = []
    for l in range(L):
        off = int(ops._lib.load().ganffn_encoder_saved_hidden_offset(C.byref(r["cfg"]), l))
        masks.append((r["saved"][off:off + S * B * F] != 0).view(S, B, F).double().cpu())
    P = _encoder_params(r["slab"], r["pe"], E, F, L)
    xo = r["x"].double().requires_grad_(True)
    with causal_attention(lengths):
        yo = O.encoder_stack(xo, P, H, O.Rng(SEED, 5, True), n_layers=L, relu_masks=masks)
    (yo * r["dout"].double()).sum().backward()
    tag = "causal encoder (%d, %d, %d) %s " % (E, H, F, "lengths" if lengths else "no lengths")
    _close(r["out"], yo.detach(), OUT_TOL, tag + "out")
    _close(r["dx"], xo.grad, GRAD_TOL, tag + "dx", 1e-12)
    per, offs = ops.layer_layout(E, F)
    gs = r["gslab"].cpu()
    for l in range(L):
        for key, o, shape in zip(ops.LAYER_KEYS, offs, ops.layer_shapes(E, F)):
            k = "transformer_encoder.layers.%d.%s" % (l, key)
            _close(gs[l * per + o:l * per + o + int(np.prod(shape))].view(shape), P[k].grad, GRAD_TOL, tag + "grad " + k, 1e-12)
    # the inputs tell the causal function from the bidirectional one (with the same lengths)
    with torch.no_grad():
        if lengths is None:
            y_bi = O.encoder_stack(r["x"].double(), P, H, O.Rng(SEED, 5, True), n_layers=L, relu_masks=masks)
        else:
            with masked_attention(lengths):
                y_bi = O.encoder_stack(r["x"].double(), P, H, O.Rng(SEED, 5, True), n_layers=L, relu_masks=masks)
    valid = valid_rows(S, lengths or [S] * B)
    assert float((y_bi - yo.detach())[valid].abs().max()) > 10 * OUT_TOL * float(yo.detach().abs().max())


@pytest.mark.parametrize("lengths", [None, [17, 16, 1, 5]], ids=["no_lengths", "lengths"])
@pytest.mark.parametrize("E,H,F", [(100, 10, 2048), (512, 8, 2048), (64, 4, 128)])
def test_encoder_stack_flags_zero_gives_the_len_calls_bits(E, H, F, lengths):
    S, B, L = 17, 4, 2
    a = _encoder_run(S, B, E, H, F, L, lengths, entry="mask0")
    b = _encoder_run(S, B, E, H, F, L, lengths, entry="len")
    c = _encoder_run(S, B, E, H, F, L, lengths, causal=False)
    for k in ("out", "dx", "gslab", "saved"):
        # (compared as bit patterns: the saved block also holds keep words and ReLU pattern bits, NaNs when read as floats)
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        assert torch.equal(c[k].view(torch.int32), b[k].view(torch.int32)), k


def test_encoder_stack_refuses_an_unknown_flag_bit_and_writes_nothing():
    from gan_ffn_amd import ops
    S, B, E, H, F, L = 17, 4, 100, 10, 2048, 2
    slab, x, pe, dout = _encoder_inputs(S, B, E, H, F, L)
    cfg = ops.enc_cfg(S, B, E, H, L, F=F, train=True)
    n_saved, n_ws = ops.enc_sizes(cfg)
    f32 = dict(device="cuda", dtype=torch.float32)
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    slab_d, x_d, pe_d = slab.cuda(), x.cuda(), pe.cuda()
    out, saved = torch.full((S * B * E,), float("nan"), **f32), torch.full((n_saved,), float("nan"), **f32)
    ws, gslab = torch.zeros(n_ws, **f32), torch.full_like(slab_d, float("nan"))
    dx = dout.cuda().clone()
    p, lib = ops._ptr, ops._lib.load()
    rc = lib.ganffn_encoder_fwd_mask(C.byref(cfg), None, C.c_uint32(2), p(x_d), p(pe_d), p(slab_d), p(out), p(saved), p(ws), p(rng),
                                     C.c_uint64(5), ops._stream())
    assert rc != 0 and b"flag" in lib.ganffn_last_error()
    rc = lib.ganffn_encoder_bwd_mask(C.byref(cfg), None, C.c_uint32(3), 0, L, p(dx), p(slab_d), p(gslab), p(saved), p(ws), p(rng),
                                     C.c_uint64(5), 1, ops._stream())
    assert rc != 0 and b"flag" in lib.ganffn_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(saved).all()) and bool(torch.isnan(gslab).all())
    assert torch.equal(dx.cpu(), dout)


# ================================================================================================================
# Phase2Engine
# ================================================================================================================
def _phase2_engine(causal, mask_padding=False, seed=11, dropout_off=False):
    from gan_ffn_amd import engine as E, model
    gens, _ = E.build_networks(device="cuda", seed=seed)
    net = model.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, mask_padding=mask_padding, causal=causal).cuda()
    if dropout_off:
        _dropout_off(net)
    return net, E.Phase2Engine(net, lr=P2_LR, weight_decay=P2_L2, class_weights=W, mask_padding=mask_padding, causal=causal)


def attention_as(causal, lens):
    """the context manager under which the oracle computes that variant of self-attention"""
    if causal:
        return causal_attention(lens)
    return masked_attention(lens) if lens is not None else contextlib.nullcontext()


def _oracle_gen_sum(slabs, eng, hb, adds, ctx):
    gens = {k: EO.Net.from_state(eng.G[k], slabs[i]["slab"], requires_grad=False) for i, k in enumerate(EO.GEN_KEYS)}
    with torch.no_grad(), ctx:
        outs = EO.generators(gens, hb, SEED, adds)
    return outs["acoustic"] + outs["visual"] + outs["text"]


def _assert_discriminates(causal, bidir, valid, what):
    """a condition on the inputs: the bidirectional oracle's value is further from the causal one's than 10x the bound the engine
    is held to — an engine that ignored the flag could not pass"""
    gap = float((causal - bidir)[valid].abs().max())
    bound = OUT_TOL * _scale(causal)
    print("causal vs bidirectional oracle %s: %.3g = %.3g x bound" % (what, gap, gap / bound))
    assert gap > 10 * bound, (what, gap, bound)


@pytest.mark.parametrize("mask_padding", [False, True], ids=["causal", "causal+mask_padding"])
@pytest.mark.parametrize("S,B,lens", ENGINE_SHAPES, ids=["7x2", "33x5", "50x2"])
def test_phase2_engine_causal_train_and_eval_match_causal_oracle(S, B, lens, mask_padding):
    from gan_ffn_amd import ops
    net, eng = _phase2_engine(True, mask_padding)
    slabs = _gen_slabs(eng, P2_LR, P2_L2)
    batch = _p2_batch(_batch(S, B, 31 * S + B, lens=lens))
    hb = _host_batch(batch)
    key_lens = lens if mask_padding else None          # what the attention is given; the loss is over real utterances either way
    valid = valid_rows(S, lens)
    ops.manual_seed(SEED)
    for train in (True, False):
        tag = "phase2 causal%s (%d, %d) %s" % (" + mask_padding" if mask_padding else "", S, B, "train" if train else "eval")
        torch.cuda.synchronize()
        pre = [sl.host() for sl in slabs]
        fc = eng.fc_slab.cpu().clone()
        nw, C_ = eng.fc_w.numel(), eng.n_classes
        fc_w, fc_b = fc[:nw].view(C_, 100), fc[eng.fc_off_b:eng.fc_off_b + C_]
        eng.step(batch, train=train)
        torch.cuda.synchronize()
        b = eng._base_add
        # the inputs: causal and bidirectional oracle (same lengths) differ
        adds = EO.gen_adds(b) if train else None
        fus_c = _oracle_gen_sum(pre, eng, hb, adds, attention_as(True, key_lens))
        fus_b = _oracle_gen_sum(pre, eng, hb, adds, attention_as(False, key_lens))
        _assert_discriminates(fus_c, fus_b, valid, "fusion")
        lp_c = torch.log_softmax(fus_c @ fc_w.double().T + fc_b.double(), 2)
        lp_b = torch.log_softmax(fus_b @ fc_w.double().T + fc_b.double(), 2)
        _assert_discriminates(lp_c, lp_b, valid, "log_prob")
        # the engine's generators against the causal oracle, on the engine's own ReLU patterns
        gens = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"], requires_grad=train) for i, k in enumerate(EO.GEN_KEYS)}
        with attention_as(True, key_lens):
            if train:
                masks_g = {k: relu_masks(eng.pass_G[k], eng.pass_G[k].cfg_train, S, B) for k in EO.GEN_KEYS}
                outs = EO.generators(gens, hb, SEED, EO.gen_adds(b), masks_g)
            else:
                with torch.no_grad():
                    outs = EO.generators(gens, hb, SEED, None)
        for k in EO.GEN_KEYS:
            _close(eng.pass_G[k].out, outs[k].detach(), OUT_TOL, "%s %s output" % (tag, k))
        res = EO.phase2_head(eng.fusion.cpu().double(), fc_w, fc_b, hb["label"], hb["umask"], W)
        _close(eng.log_prob, res["log_prob"], OUT_TOL, tag + " log_prob")
        if train:
            d_fusion = eng.d_fusion.cpu().double()
            _close(d_fusion, res["d_fusion"], GRAD_TOL, tag + " d_fusion", 1e-12)
            _check_generator_grads(eng, gens, outs, d_fusion, tag)


def test_phase2_engine_causal_off_gives_the_bits_of_the_default_engine():
    from gan_ffn_amd import ops
    S, B = 17, 3
    batch = _p2_batch(_batch(S, B, 5, lens=[17, 5, 1]))
    got = []
    for kwargs in ({}, {"causal": False}):
        from gan_ffn_amd import engine as E, model
        gens, _ = E.build_networks(device="cuda", seed=11)
        net = model.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, **kwargs).cuda()
        eng = E.Phase2Engine(net, lr=P2_LR, weight_decay=P2_L2, class_weights=W, **kwargs)
        ops.manual_seed(SEED)
        loss, lp = eng.step(batch, train=True)
        torch.cuda.synchronize()
        got.append((loss.detach().clone(), lp.detach().clone(), {k: st.slab.detach().clone() for k, st in eng.G.items()}))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    for k in got[0][2]:
        assert torch.equal(got[0][2][k], got[1][2][k]), k


# ================================================================================================================
# module path
# ================================================================================================================
def _replace_future(batch, t, seed=1):
    other = dict(batch)
    g = torch.Generator().manual_seed(seed)
    for k in ("acoustic", "visual", "text"):
        v = batch[k].clone()
        v[t + 1:] = (torch.rand(v[t + 1:].shape, generator=g) * 3.0 - 1.0).cuda()
        other[k] = v
    return other


@pytest.mark.parametrize("S,B,lens", [(33, 3, [33, 20, 1]), (50, 2, [50, 3])], ids=["33x3", "50x2"])
def test_module_causal_prediction_does_not_depend_on_the_future(S, B, lens):
    """GAN_FFN(causal=True).eval(): log_prob[:t + 1] keeps every bit when the three modalities' rows > t are replaced; with
    causal=False the same replacement changes rows <= t"""
    batch = _p2_batch(_batch(S, B, 9, lens=lens))
    net, _ = _phase2_engine(True)
    net.eval()
    plain = copy.deepcopy(net)
    plain.causal = False
    with torch.no_grad():
        lp = net(batch["acoustic"], batch["visual"], batch["text"])[0]
        lp_plain = plain(batch["acoustic"], batch["visual"], batch["text"])[0]
        assert not bool(torch.isnan(lp).any())
        for t in sorted({0, 15, 16, 31, 32, 47, 48, S - 2} & set(range(S - 1))):
            other = _replace_future(batch, t)
            lp2 = net(other["acoustic"], other["visual"], other["text"])[0]
            assert torch.equal(lp2[:t + 1], lp[:t + 1]), t
            assert not torch.equal(lp2[t + 1:], lp[t + 1:]), t
            lp3 = plain(other["acoustic"], other["visual"], other["text"])[0]
            assert float((lp3[:t + 1] - lp_plain[:t + 1]).abs().max()) > 10 * OUT_TOL * float(lp_plain.abs().max()), t


def test_module_path_causal_matches_the_engine():
    """GAN_FFN(causal=True) under autograd against Phase2Engine(causal=True), dropout off (both then compute the same
    function), alone and with mask_padding; bounds of tests/test_hip_key_len_engines.py::test_module_path_with_mask_padding_matches_the_engine"""
    from gan_ffn_amd import model as M
    S, B, lens = 17, 4, [17, 16, 1, 5]
    batch = _p2_batch(_batch(S, B, 9, lens=lens))

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    for mask_padding in (False, True):
        net, eng = _phase2_engine(True, mask_padding, dropout_off=True)
        net.train()
        ref = copy.deepcopy(net)
        args = (batch["acoustic"], batch["visual"], batch["text"]) + ((batch["umask"],) if mask_padding else ())
        lp = ref(*args)[0]
        loss_ref = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))(lp.transpose(0, 1).contiguous().view(-1, 6),
                                                                  batch["label"].view(-1), batch["umask"])
        loss_ref.backward()
        loss, log_prob = eng.step(batch, train=True)
        torch.cuda.synchronize()
        assert abs(float(loss) - float(loss_ref)) < 2e-5 * max(1.0, abs(float(loss_ref)))
        assert rel(log_prob, lp) < 1e-4
        refp = dict(ref.named_parameters())
        for k, pre in (("acoustic", "acoustic_generator."), ("visual", "visual_generator."), ("text", "text_generator.")):
            st = eng.G[k]
            for name in st.named:
                assert rel(st.w(name, True).view_as(refp[pre + name]), refp[pre + name].grad) < 2e-3, (mask_padding, k, name)
        # and the bidirectional module is a different function on this batch
        bidir = copy.deepcopy(ref)
        bidir.causal = False
        with torch.no_grad():
            lp_u = bidir(*args)[0]
        valid = valid_rows(S, lens).cuda()
        assert float((lp_u - lp)[valid].abs().max()) > 10 * 1e-4 * float(lp.abs().max())
