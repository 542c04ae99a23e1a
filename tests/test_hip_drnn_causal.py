"""The causal DialogueRNN classifier on the GPU: the causal general2 kernels (all six instantiations) against the causal formula
in fp64, flags = 0 against the existing entry points bit for bit, guard bands round every buffer the raw causal calls write,
GAN_FFN_DialogueRNN(causal=True) through the module path against the per-step fp64 oracle (tests/drnn_causal_oracle.py) and
bit for bit against its own future, DrnnEngine on a causal net in TRAIN mode against that oracle with the engine's own Philox
masks (method and tolerances of tests/test_hip_classifier_engines_train_oracle.py), the default engine untouched by a causal one
in the same process, and engine against module."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import drnn_causal_oracle as DCO
import engine_oracle as EO
from causal_oracle import causal_attention
from util import relu_masks
from test_hip_classifier_engines_train_oracle import (DIMS, DRNN_L2, DRNN_LR, SEED, W, WORST, _Slab, _Taps, _batch, _check_adam,
                                                      _check_blocks, _close, _gen_slabs, _host_batch, _kink_audit, _within)

pytestmark = pytest.mark.gpu

CAUSAL = 1        # GANFFN_ATTN_CAUSAL


@pytest.fixture(scope="module", autouse=True)
def _report():
    WORST.clear()
    yield
    print("\ncausal DialogueRNN classifier, largest error / tolerance per check: " +
          ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


# ================================================================================================================
# 1-3: the kernels
# ================================================================================================================
G2_SHAPES = [(1, 1, 4), (16, 2, 100), (17, 3, 100), (33, 3, 50), (128, 2, 100), (5, 2, 1024), (112, 2, 600), (128, 2, 600)]


def _g2_inputs(S, B, D):
    """the inputs of test_general2_attention_kernel_vs_fp64_torch, ragged lengths with S and 1 among them"""
    g = torch.Generator().manual_seed(S * 1000 + D)
    M = (torch.rand(S, B, D, generator=g) - 0.5)
    X = (torch.rand(S, B, D, generator=g) - 0.5) * 0.7
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    if B > 1:
        lens[1] = 1
    mask = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).float()
    gy = torch.rand(S, B, D, generator=g) - 0.5
    return M, X, mask, gy


def _causal_formula(X64, M64, m):
    """a_tj = e^{s_tj} m_j [j <= t] / sum_k e^{s_tk} m_k [k <= t], s_tj = tanh(m_j <x_t, m_j M_j>), att_t = sum_j a_tj M_j"""
    S = M64.shape[0]
    Mb = M64.transpose(0, 1)                                                             # (B, S, D)
    s = torch.tanh(torch.einsum("tbd,bjd->btj", X64, Mb * m.unsqueeze(2)) * m.unsqueeze(1))
    e = torch.exp(s) * m.unsqueeze(1) * torch.tril(torch.ones(S, S, dtype=torch.float64))
    a = e / e.sum(2, keepdim=True)
    return torch.einsum("btj,bjd->tbd", a, Mb), a


def _raw_fwd(x, mem, mask, flags, att, alpha, ts, S, B, D, entry="mask"):
    from gan_ffn_amd import _lib, ops
    P = ops._ptr
    if entry == "mask":
        _lib.call("ganffn_general2_attention_fwd_mask", P(x), P(mem), P(mask), C.c_uint32(flags), P(att), P(alpha), P(ts), S, B, D,
                  ops._stream())
    else:
        _lib.call("ganffn_general2_attention_fwd", P(x), P(mem), P(mask), P(att), P(alpha), P(ts), S, B, D, ops._stream())


def _raw_bwd(g, x, mem, mask, flags, alpha, ts, du, dx, dm, S, B, D, entry="mask"):
    from gan_ffn_amd import _lib, ops
    P = ops._ptr
    if entry == "mask":
        _lib.call("ganffn_general2_attention_bwd_mask", P(g), P(x), P(mem), P(mask), C.c_uint32(flags), P(alpha), P(ts), P(du),
                  P(dx), P(dm), S, B, D, ops._stream())
    else:
        _lib.call("ganffn_general2_attention_bwd", P(g), P(x), P(mem), P(mask), P(alpha), P(ts), P(du), P(dx), P(dm), S, B, D,
                  ops._stream())


def _raw_pass(S, B, D, flags, entry="mask", fill=float("nan")):
    M, X, mask, gy = (t.cuda().contiguous() for t in _g2_inputs(S, B, D))
    new = lambda *shape: torch.full(shape, fill, device="cuda", dtype=torch.float32)
    out = dict(att=new(S, B, D), alpha=new(B, S, S), ts=new(B, S, S), du=new(B, S, S), dx=new(S, B, D), dm=new(S, B, D))
    _raw_fwd(X, M, mask, flags, out["att"], out["alpha"], out["ts"], S, B, D, entry)
    _raw_bwd(gy, X, M, mask, flags, out["alpha"], out["ts"], out["du"], out["dx"], out["dm"], S, B, D, entry)
    torch.cuda.synchronize()
    return out, mask


@pytest.mark.parametrize("S,B,D", G2_SHAPES)
def test_causal_general2_kernels_vs_fp64(S, B, D):
    from gan_ffn_amd import ops
    M, X, mask, gy = _g2_inputs(S, B, D)
    M64, X64 = M.double().requires_grad_(True), X.double().requires_grad_(True)
    att64, a64 = _causal_formula(X64, M64, mask.double())
    (att64 * gy.double()).sum().backward()
    Md, Xd = M.cuda().requires_grad_(True), X.cuda().requires_grad_(True)
    att, alpha = ops.General2AttnFn.apply(Xd, Md, mask.cuda(), True)
    (att * gy.cuda()).sum().backward()

    def rel(a, b):
        return float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30))
    errs = dict(alpha=rel(alpha, a64), att=rel(att, att64), dx=rel(Xd.grad, X64.grad), dmem=rel(Md.grad, M64.grad))
    print("causal general2 (%d, %d, %d): %s" % (S, B, D, ", ".join("%s %.3g" % kv for kv in errs.items())))
    assert errs["alpha"] < 5e-6 and errs["att"] < 5e-6
    assert errs["dx"] < 2e-5 and errs["dmem"] < 2e-5
    # the saved tensors through the raw calls, buffers pre-filled with NaN: written completely, exact zeros above the diagonal and
    # on masked keys
    out, _ = _raw_pass(S, B, D, CAUSAL)
    above = torch.triu(torch.ones(S, S), 1).bool()
    dead = above.unsqueeze(0) | (mask == 0).unsqueeze(1)                                  # (B, S query, S key)
    for k in ("alpha", "ts", "du"):
        v = out[k].cpu()
        assert not bool(torch.isnan(v).any()), k
        assert float(v[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0, k
    for k in ("att", "dx", "dm"):
        assert not bool(torch.isnan(out[k]).any()), k
    assert torch.equal(out["alpha"], alpha.detach()) and torch.equal(out["att"], att.detach())
    assert torch.equal(out["dx"], Xd.grad) and torch.equal(out["dm"], Md.grad)
    # and the flag is not ignored (a condition on the inputs): the bidirectional weights are far from these
    if S > 1:
        plain, _ = _raw_pass(S, B, D, 0)
        assert float((plain["alpha"] - out["alpha"]).abs().max()) > 1e-3


@pytest.mark.parametrize("S,B,D", [(17, 3, 100), (112, 2, 600)])
def test_flags_zero_gives_the_bits_of_the_existing_entry_points(S, B, D):
    new, _ = _raw_pass(S, B, D, 0, "mask")
    old, _ = _raw_pass(S, B, D, 0, "plain")
    for k in new:
        assert not bool(torch.isnan(new[k]).any()), k
        assert torch.equal(new[k], old[k]), k


@pytest.mark.parametrize("S,B,D", [(17, 3, 100), (5, 1, 4)])
def test_causal_general2_writes_inside_its_buffers(S, B, D):
    """every output and workspace buffer of the raw causal calls sits inside a canary-filled allocation; no canary changes"""
    M, X, mask, gy = (t.cuda().contiguous() for t in _g2_inputs(S, B, D))
    GUARD, CANARY = 4096, -7.25
    sizes = dict(att=S * B * D, alpha=B * S * S, ts=B * S * S, du=B * S * S, dx=S * B * D, dm=S * B * D)
    whole = {k: torch.full((n + 2 * GUARD,), CANARY, device="cuda", dtype=torch.float32) for k, n in sizes.items()}
    v = {k: whole[k][GUARD:GUARD + n] for k, n in sizes.items()}
    _raw_fwd(X, M, mask, CAUSAL, v["att"], v["alpha"], v["ts"], S, B, D)
    _raw_bwd(gy, X, M, mask, CAUSAL, v["alpha"], v["ts"], v["du"], v["dx"], v["dm"], S, B, D)
    torch.cuda.synchronize()
    for k, n in sizes.items():
        w = whole[k].cpu()
        assert bool((w[:GUARD] == CANARY).all()) and bool((w[GUARD + n:] == CANARY).all()), k
        assert not bool((w[GUARD:GUARD + n] == CANARY).any()), k        # and the buffer itself was written completely


# ================================================================================================================
# nets, oracles
# ================================================================================================================
def _net(listener=False, att="general", seed=3, causal=True, mask_padding=False):
    from gan_ffn_amd import model as M
    torch.manual_seed(seed)
    kw = dict(causal=True) if causal else {}
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                listener_state=listener, context_attention=att, dropout_rec=0.1, dropout=0.6,
                                mask_padding=mask_padding, **kw, **DIMS)
    return net.cuda().train()


def _lens(batch):
    return [int(v) for v in batch["umask"].sum(1).tolist()]


def _ctx(batch, mask_padding):
    """the context under which the oracle's generators compute what the causal net's compute"""
    return causal_attention(_lens(batch) if mask_padding else None)


def _flip_future(batch, t, seed=1):
    """other features and the other speaker after step t, same shapes"""
    other = dict(batch)
    g = torch.Generator().manual_seed(seed)
    for k in ("acoustic", "visual", "text"):
        v = batch[k].clone()
        v[t + 1:] = (torch.rand(v[t + 1:].shape, generator=g) * 3.0 - 1.0).cuda()
        other[k] = v
    q = batch["qmask"].clone()
    q[t + 1:] = q[t + 1:].flip(2)
    other["qmask"] = q
    return other


def _module_lp(net, batch):
    return net(batch["acoustic"], batch["visual"], batch["text"], batch["qmask"], batch["umask"])[0]


# ================================================================================================================
# 4: module path
# ================================================================================================================
@pytest.mark.parametrize("S,B,att,listener", [(13, 4, "general", False), (33, 7, "general", False), (13, 4, "concat", True)],
                         ids=["13x4", "33x7", "13x4_concat_listener"])
def test_module_path_causal_matches_the_oracle(S, B, att, listener):
    from gan_ffn_amd import dialogue_rnn as DR, engine as E
    net = _net(listener, att).eval()
    assert type(net.bi_model) is DR.UniModel and net.causal
    batch = _batch(S, B, 100 * S + B)
    hb = _host_batch(batch)
    with torch.no_grad():
        outs = {k: getattr(net, k + "_generator")(batch[k], None, causal=True) for k in EO.GEN_KEYS}
        fusion = outs["acoustic"] + outs["visual"] + outs["text"]
        lp, alpha, alpha_f, alpha_b = net(batch["acoustic"], batch["visual"], batch["text"], batch["qmask"], batch["umask"])
    assert lp.shape == (S, B, 6) and len(alpha) == S and alpha_b == [] and not bool(torch.isnan(lp).any())
    # the generators through the causal oracle (the NetStates of an engine give the oracle its parameters)
    eng = E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W)
    gens = {k: EO.Net.from_state(eng.G[k], eng.G[k].slab.cpu(), requires_grad=False) for k in EO.GEN_KEYS}
    with torch.no_grad(), causal_attention(None):
        want = EO.generators(gens, hb, SEED, None)
    with torch.no_grad():
        bidir = EO.generators(gens, hb, SEED, None)
    for k in EO.GEN_KEYS:
        _close("generator output", outs[k], want[k], 1e-4, 0.0, "module %s output" % k)
    assert float((want["text"] - bidir["text"]).abs().max()) > 10 * 1e-4 * float(want["text"].abs().max())
    # the head, fed the module's own fusion
    um = copy.deepcopy(net.bi_model).cpu().double().eval()
    res = DCO.uni_head(um, fusion.cpu().double(), hb["qmask"], hb["umask"])
    _close("log_prob", lp, res["log_prob"], 1e-4, 0.0, "module log_prob")
    a = torch.stack(alpha, 1)
    assert float(a[:, torch.triu(torch.ones(S, S), 1).bool()].abs().max()) == 0.0
    _close("alpha", a, res["alpha"], 1e-4, 0.0, "module alpha")


def test_module_causal_prediction_does_not_depend_on_the_future():
    """GAN_FFN_DialogueRNN(causal=True).eval(): log_prob[:t + 1] keeps every bit when features and speakers after t change;
    the rows after t do change"""
    S, B = 33, 3
    net = _net().eval()
    batch = _batch(S, B, 9, lens=[33, 20, 1])
    with torch.no_grad():
        lp = _module_lp(net, batch)
        for t in (0, S // 2, S - 2):
            lp2 = _module_lp(net, _flip_future(batch, t))
            assert torch.equal(lp2[:t + 1], lp[:t + 1]), t
            assert not torch.equal(lp2[t + 1:], lp[t + 1:]), t


def test_module_causal_backward_moves_the_head_and_the_generators():
    from gan_ffn_amd import model as M
    S, B = 13, 4
    net = _net(listener=True)
    batch = _batch(S, B, 5)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    lp = _module_lp(net, batch)
    loss = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))(lp.transpose(0, 1).contiguous().view(-1, 6), batch["label"].view(-1),
                                                           batch["umask"])
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach()))
    moved = {k: float((v.detach() - before[k]).abs().max()) for k, v in net.named_parameters()}
    head = [k for k in moved if k.startswith("bi_model.")]
    assert any(k.startswith("bi_model.dialog_rnn_f.dialogue_cell.l_cell.") for k in head)
    assert not any(k.startswith("bi_model.dialog_rnn_r.") for k in head)
    for k in head + ["text_generator.transformer_encoder.layers.0.linear1.weight", "visual_generator.fc2.weight",
                     "acoustic_generator.fc1.weight"]:
        assert moved[k] > 0, k


# ================================================================================================================
# 5: DrnnEngine on a causal net, train mode
# ================================================================================================================
class _CausalHarness:
    """wraps one causal DrnnEngine's _step: state before and after, every library call in between, the engine's intermediates"""

    def __init__(self, eng, net, monkeypatch):
        from gan_ffn_amd import _lib
        self.eng = eng
        self.taps = _Taps(monkeypatch)
        self.calls = None
        tapped = _lib.call

        def every(name, *a):
            if self.calls is not None:
                self.calls.append((name, [getattr(x, "value", x) for x in a]))
            return tapped(name, *a)
        monkeypatch.setattr(_lib, "call", every)
        self.bases, self.compared = [], 0
        names = {id(p): n for n, p in net.named_parameters()}
        self.hnames = [names[id(p)][len("bi_model."):] for p in eng._hparams]
        self.um = copy.deepcopy(net.bi_model).cpu().double()
        assert set(self.hnames) == {n for n, _ in self.um.named_parameters()}
        assert not any(n.startswith("dialog_rnn_r.") for n in self.hnames)
        assert len(self.hnames) == eng.ncell + 6 + (4 if eng.listener else 0)
        # the slab's order: one cell, the six head tensors, then the cell's listener tensors
        assert self.hnames[eng.ncell:eng.ncell + 6] == ["matchatt.transform.weight", "matchatt.transform.bias", "linear.weight",
                                                        "linear.bias", "smax_fc.weight", "smax_fc.bias"]
        assert all(n.startswith("dialog_rnn_f.dialogue_cell.l_cell.") for n in self.hnames[eng.ncell + 6:])
        self.slabs = _gen_slabs(eng, DRNN_LR, DRNN_L2) + [
            _Slab("head", eng.h_slab, eng.h_grad, eng.h_m, eng.h_v, eng.h_step, DRNN_LR, DRNN_L2,
                  [(o, p.numel()) for o, p in zip(eng._hoffs, eng._hparams)])]
        step = eng._step
        eng._step = lambda batch, train=True: self._run(step, batch, train)

    def _load_head(self, slab):
        params = dict(self.um.named_parameters())
        with torch.no_grad():
            for n, o, p in zip(self.hnames, self.eng._hoffs, self.eng._hparams):
                params[n].copy_(slab[o:o + p.numel()].view(p.shape).double())
        return self.um

    def _check_launches(self, b, S, B, P, train):
        from gan_ffn_amd import ops
        eng, log, calls = self.eng, self.taps_log, self.calls_log
        ga = EO.gen_adds(b)
        t = 1 if train else 0
        fl = lambda x: float(np.float32(x))
        fam = ops.drnn_family(B, P, eng.att, eng.listener)
        rec = "ganffn_drnn_%s" % (fam + "_" if fam else "")
        # what the taps of the train-oracle test see: the generators at their slots, the hidden layer at b + 7 (the recurrence
        # is among them for the families those taps name)
        want = []
        for k in EO.GEN_KEYS:
            want += [("encoder_fwd_raw", ga[k][0], ()), ("head_fwd_raw", ga[k][1], ())]
        if fam in ("", "listener"):
            want += [(rec + "fwd", b + EO.A_REC, ())]
        want += [("ganffn_ffn_linear1_fwd", b + EO.A_HEAD, (fl(eng.p_hid), EO.SITE_HIDDEN, t))]
        if train:
            if fam in ("", "listener"):
                want += [(rec + "bwd", b + EO.A_REC, ())]
            for k in EO.GEN_KEYS:
                want += [("head_bwd_raw", ga[k][1], ()), ("encoder_bwd_raw", ga[k][0], ())]
        assert log == want, (b, log)
        names = [n for n, _ in calls]
        # one recurrence direction, nothing reversed, no join of two directions
        assert "ganffn_seq_reverse" not in names and not any(n.startswith("ganffn_drnn_join") for n in names), names
        ndir_pos = {"": 1, "listener": 1, "att": 2, "party": 3, "batch": 3}[fam]
        recs = [(n, a) for n, a in calls if n.startswith("ganffn_drnn_") and n.endswith(("_fwd", "_bwd"))]
        assert [n for n, _ in recs] == [rec + "fwd"] + ([rec + "bwd"] if train else []), recs
        for n, a in recs:
            assert a[ndir_pos] == 1 and a[-2] == b + EO.A_REC, (n, a[ndir_pos], a[-2])
        # the join: dropout_rec on e_f alone, forward and on the gradient, at the join's site and the head's offset; none in eval
        drops = [a for n, a in calls if n == "ganffn_dropout"]
        assert len(drops) == (2 if train else 0), drops
        for a in drops:
            assert a[2:6] == [S * B, eng.He, fl(eng.p_join), EO.SITE_JOIN_F] and a[7] == b + EO.A_HEAD, a
        # the causal general2 entry points, under the flag
        g2 = [(n, a) for n, a in calls if "general2" in n]
        assert [n for n, _ in g2] == ["ganffn_general2_attention_fwd_mask"] + (["ganffn_general2_attention_bwd_mask"] if train else [])
        assert g2[0][1][3] == CAUSAL and (not train or g2[1][1][4] == CAUSAL)
        # the RNG block: distinct forward offsets b .. b + 7 (the join and the hidden layer share b + 7, at different sites)
        fwd = [a for n, a, _ in log if "fwd" in n] + ([] if fam in ("", "listener") else [recs[0][1][-2]])
        assert sorted(fwd) == list(range(b, b + 8)), (b, fwd)

    def _run(self, step, batch, train):
        eng = self.eng
        torch.cuda.synchronize()
        pre = [sl.host() for sl in self.slabs]
        self.taps.log, self.calls = [], []
        out = step(batch, train)
        torch.cuda.synchronize()
        self.taps_log, self.taps.log = self.taps.log, None
        self.calls_log, self.calls = self.calls, None
        b = eng._base_add
        self.bases.append(b)
        post = [sl.host(grad=True) for sl in self.slabs]
        S, B = batch["text"].shape[:2]
        self._check_launches(b, S, B, batch["qmask"].size(2), train)
        T, f = S * B, eng._f
        hb = _host_batch(batch)
        tag = "causal step %d (%d, %d)%s" % (len(self.bases) - 1, S, B, "" if train else " eval")
        ctx = lambda: _ctx(batch, eng.mask_padding)
        Dm, Dh, Cn = eng.Dm, eng.Dh2, eng.n_classes
        assert Dh == DIMS["D_h"] and eng.D2 == DIMS["D_e"]
        e = dict(outs={k: eng.pass_G[k].out.cpu().double() for k in EO.GEN_KEYS},
                 fusion=f["fusion"][:T * Dm].view(S, B, Dm).cpu().double(), hidden=f["hidden"][:T * Dh].view(S, B, Dh).cpu().double(),
                 log_prob=f["log_prob"][:T * Cn].view(S, B, Cn).cpu().double(),
                 d_fusion=f["dU_f"][:T * Dm].view(S, B, Dm).cpu().double(), loss=float(eng.loss))
        um = self._load_head(pre[3]["slab"])
        pattern = e["hidden"] > 0
        if train:
            gens = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"]) for i, k in enumerate(EO.GEN_KEYS)}
            masks_g = {k: relu_masks(eng.pass_G[k], eng.pass_G[k].cfg_train, S, B) for k in EO.GEN_KEYS}
            with ctx():
                outs = EO.generators(gens, hb, SEED, EO.gen_adds(b), masks_g)
            for k in EO.GEN_KEYS:
                _close("generator output", e["outs"][k], outs[k], 1e-4, 0.0, "%s %s output" % (tag, k))
            masks = DCO.uni_masks(um, S, B, SEED, b + EO.A_REC, b + EO.A_HEAD)
            # the train-mode join mask is the one the contract names
            assert torch.equal(masks["join_f"], EO._keep(S * B, eng.He, eng.p_join, EO.SITE_JOIN_F, SEED, b + EO.A_HEAD).view(S, B, -1))
            res = DCO.uni_head(um, e["fusion"], hb["qmask"], hb["umask"], hb["label"], W, masks, pattern)
            _kink_audit(res["pre"], pattern, masks["hidden"] > 0, tag)
            _close("hidden", e["hidden"], res["hidden"], 1e-4, 0.0, tag + " hidden")
            _close("log_prob", e["log_prob"], res["log_prob"], 1e-4, 0.0, tag + " log_prob")
            _within("loss", np.array([abs(e["loss"] - res["loss"])]), np.array([2e-5 * abs(res["loss"])]), tag + " loss")
            hg = post[3]["grad"]
            for n, o, p in zip(self.hnames, eng._hoffs, eng._hparams):
                _close("head gradient", hg[o:o + p.numel()].view(p.shape), res["grads"][n], 1e-3, 1e-12, "%s grad %s" % (tag, n))
            _close("d_fusion", e["d_fusion"], res["d_fusion"], 1e-3, 1e-12, tag + " d_fusion")
            with ctx():
                gg = EO.generator_grads(gens, outs, e["d_fusion"])
            for i, k in enumerate(EO.GEN_KEYS):
                st = eng.G[k]
                assert set(gg[k]) == set(st.named)
                for n, (o, shape) in st.named.items():
                    _close("generator gradient", post[i]["grad"][o:o + int(np.prod(shape))].view(*shape), gg[k][n], 1e-3, 1e-12,
                           "%s %s grad %s" % (tag, k, n))
            for sl, a, z in zip(self.slabs, pre, post):
                _check_adam(sl, a, z, tag)
            gens0 = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"]) for i, k in enumerate(EO.GEN_KEYS)}
            with ctx():
                ch = DCO.uni_step(gens0, um, hb, SEED, b, True, class_w=W)
            _within("chained loss", np.array([abs(e["loss"] - ch["loss"])]), np.array([2e-4 * abs(ch["loss"])]), tag + " chained loss")
        else:
            gens = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"], requires_grad=False) for i, k in enumerate(EO.GEN_KEYS)}
            with torch.no_grad(), ctx():
                outs = EO.generators(gens, hb, SEED, None)
            for k in EO.GEN_KEYS:
                _close("generator output", e["outs"][k], outs[k], 1e-4, 0.0, "%s %s output" % (tag, k))
            res = DCO.uni_head(um, e["fusion"], hb["qmask"], hb["umask"], hb["label"], W, None, pattern)
            _kink_audit(res["pre"], pattern, torch.ones_like(pattern), tag)
            _close("log_prob", e["log_prob"], res["log_prob"], 1e-4, 0.0, tag + " log_prob")
            _within("loss", np.array([abs(e["loss"] - res["loss"])]), np.array([2e-5 * abs(res["loss"])]), tag + " loss")
            for sl, a, z in zip(self.slabs, pre, post):
                for k in ("slab", "m", "v"):
                    assert torch.equal(a[k], z[k]), (tag, sl.name, k)
                assert a["t"] == z["t"], (tag, sl.name)
        self.compared += 1
        return out


ENGINE_CASES = {
    "13x4_two_steps_then_eval": (dict(), [(13, 4, {}), (13, 4, {})], True),
    "33x7": (dict(), [(33, 7, dict(lens=[33, 1, 20, 33, 7, 12, 2]))], False),
    "17x5_listener": (dict(listener=True), [(17, 5, {})], False),
    "13x4_mask_padding": (dict(mask_padding=True), [(13, 4, {})], False),
    "20x33_max_dialogues_64": (dict(max_dialogues=64), [(20, 33, {})], False),
}


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_causal_drnn_engine_train_step_matches_fp64_oracle(case, monkeypatch):
    from gan_ffn_amd import engine as E, ops
    kw, shapes, eval_after = ENGINE_CASES[case]
    listener, mask_padding = kw.get("listener", False), kw.get("mask_padding", False)
    net = _net(listener, mask_padding=mask_padding)
    eng = E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W, mask_padding=mask_padding,
                       max_dialogues=kw.get("max_dialogues", 32))
    assert eng.causal and eng.ndir == 1 and (eng.p_rec, eng.p_join, eng.p_hid) == (0.1, 0.75, 0.6) and eng.listener == listener
    for st in eng.G.values():
        assert (st.p_pe, st.p_enc, st.p_head) == (0.2, 0.1, 0.2)
    # buffers for one direction
    h = _CausalHarness(eng, net, monkeypatch)
    eng.reserve(max(S for S, _, _ in shapes), max(B for _, B, _ in shapes))
    ops.manual_seed(SEED)
    for i, (S, B, bkw) in enumerate(shapes):
        eng.step(_batch(S, B, 100 * S + B + i, **bkw), train=True)
    if eval_after:
        S, B, bkw = shapes[-1]
        eng.step(_batch(S, B, 7 + S, **bkw), train=False)
    torch.cuda.synchronize()
    _check_blocks(h.bases, EO.DRNN_ADDS)
    assert h.compared == len(shapes) + (1 if eval_after else 0)
    for k in ("rev_U", "e_b", "alpha_b", "d_e_b", "dU_b", "saved_b", "ws_b"):
        assert eng._f[k] is None, k
    T = eng._alloc_S * eng._alloc_B
    assert eng._f["emotions"].numel() == T * DIMS["D_e"] and eng._f["hidden"].numel() == T * DIMS["D_h"]


# ================================================================================================================
# 6: the default engine is untouched
# ================================================================================================================
def _default_two_steps():
    from gan_ffn_amd import engine as E, ops
    net = _net(causal=False, seed=5)
    eng = E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W)
    assert not eng.causal and eng.ndir == 2
    ops.manual_seed(SEED)
    losses = []
    for i in range(2):
        loss, lp = eng.step(_batch(13, 4, 50 + i), train=True)
        losses.append((loss.detach().clone(), lp.detach().clone()))
    torch.cuda.synchronize()
    slabs = [eng.h_slab.clone(), eng.h_m.clone(), eng.h_v.clone()] + [t.clone() for st in eng.G.values()
                                                                      for t in (st.slab, st.exp_avg, st.exp_avg_sq)]
    return losses, slabs


def test_default_engine_is_untouched_by_a_causal_engine_in_the_same_process():
    from gan_ffn_amd import engine as E, ops
    first = _default_two_steps()
    cnet = _net(seed=5)
    ceng = E.DrnnEngine(cnet, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W)
    ops.manual_seed(SEED)
    closs, _ = ceng.step(_batch(13, 4, 50), train=True)
    torch.cuda.synchronize()
    second = _default_two_steps()
    for (l1, p1), (l2, p2) in zip(first[0], second[0]):
        assert torch.equal(l1, l2) and torch.equal(p1, p2)
    assert len(first[1]) == len(second[1]) == 12
    for a, b in zip(first[1], second[1]):
        assert torch.equal(a, b)
    assert float(closs) != float(first[0][0][0])          # and the causal step is another function


# ================================================================================================================
# 7: engine and module agree
# ================================================================================================================
def test_causal_engine_and_module_agree_and_the_engine_ignores_the_future():
    from gan_ffn_amd import engine as E
    S, B = 13, 4
    net = _net().eval()
    eng = E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W)
    batch = _batch(S, B, 21)
    with torch.no_grad():
        lp_mod = _module_lp(net, batch).clone()
    _, lp = eng.step(batch, train=False)
    lp = lp.detach().clone()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(lp).any())
    assert float((lp - lp_mod).abs().max()) <= 1e-5 * float(lp_mod.abs().max())
    for t in (0, S // 2, S - 2):
        _, lp2 = eng.step(_flip_future(batch, t), train=False)
        torch.cuda.synchronize()
        assert torch.equal(lp2[:t + 1], lp[:t + 1]), t
        assert not torch.equal(lp2[t + 1:], lp[t + 1:]), t
