"""The causal DialogueRNN classifier on the CPU: dialogue_rnn.UniModel (torch path, fp64) against the per-step fp64 oracle
(tests/drnn_causal_oracle.py: one truncated MatchingAttention call per step), general2_all_queries(causal=True) against the
truncated calls, the state_dict of GAN_FFN_DialogueRNN(causal=True), the property the feature exists for (nothing after step t
reaches log_prob[:t+1]; with BiModel it does), and what the new general2 entry points refuse before any launch."""
import ctypes as C

import pytest
import torch

import drnn_causal_oracle as DCO

S, B, LENS = 9, 3, [9, 1, 4]
DIMS = dict(D_m=12, D_g=16, D_p=16, D_e=8, D_h=10, D_a=12)
ATT = ["general", "simple", "dot", "general2", "concat"]


def _dims(att):
    d = dict(DIMS)
    if att == "dot":
        d["D_m"] = d["D_g"]
    return d


def _inputs(D_m, seed=3, lens=LENS, S_=S):
    g = torch.Generator().manual_seed(seed)
    Bn = len(lens)
    valid = (torch.arange(S_).unsqueeze(1) < torch.tensor(lens).unsqueeze(0)).double()         # (S, B)
    U = (torch.rand(S_, Bn, D_m, generator=g, dtype=torch.float64) - 0.5) * valid.unsqueeze(2)
    spk = torch.randint(0, 2, (S_, Bn), generator=g)
    qmask = torch.nn.functional.one_hot(spk, 2).double() * valid.unsqueeze(2)
    label = torch.randint(0, 6, (Bn, S_), generator=g) * valid.t().long()
    return U, qmask, valid.t().contiguous(), label


def _uni(att, listener, seed=1):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    return DR.UniModel(n_classes=6, listener_state=listener, context_attention=att, dropout_rec=0.1, dropout=0.6,
                       **_dims(att)).double().eval()


@pytest.mark.parametrize("listener", [False, True], ids=["", "listener"])
@pytest.mark.parametrize("att", ATT)
def test_unimodel_cpu_equals_the_per_step_oracle(att, listener):
    um = _uni(att, listener)
    U, qmask, umask, label = _inputs(_dims(att)["D_m"])
    with torch.no_grad():
        lp, alpha, alpha_f, alpha_b = um(U, qmask, umask)
    res = DCO.uni_head(um, U, qmask, umask)
    assert lp.shape == (S, B, 6) and not bool(torch.isnan(lp).any())
    assert float((lp - res["log_prob"]).abs().max()) <= 1e-12
    assert len(alpha) == S and alpha_b == [] and len(alpha_f) == S - 1
    assert float((torch.stack(alpha, 1) - res["alpha"]).abs().max()) <= 1e-12
    with torch.no_grad():                                   # att2 = False: no second attention at all
        lp0, alpha0, _, _ = um(U, qmask, umask, att2=False)
    assert alpha0 == [] and lp0.shape == lp.shape


def test_general2_all_queries_causal_equals_the_truncated_calls():
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(2)
    m = DR.MatchingAttention(8, 8, att_type="general2").double()
    with torch.no_grad():
        m.transform.weight.mul_(60.0)                       # scores away from tanh's linear range
    g = torch.Generator().manual_seed(4)
    for lens in (LENS, [1], [5, 9, 9, 2]):
        Bn = len(lens)
        Sn = max(lens)
        M = torch.rand(Sn, Bn, 8, generator=g, dtype=torch.float64) - 0.5
        mask = (torch.arange(Sn).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).double()
        with torch.no_grad():
            att, alpha = m.general2_all_queries(M, mask, causal=True)
            want_att, want_alpha = DCO.causal_general2(m, M, mask)
            att_b, alpha_b = m.general2_all_queries(M, mask)
            att_d, alpha_d = m.general2_all_queries(M, mask, causal=False)
        assert float((att - want_att).abs().max()) <= 1e-14 and float((alpha - want_alpha).abs().max()) <= 1e-14
        assert not bool(torch.isnan(att).any())              # rows past a dialogue's end attend over its real steps
        above = torch.triu(torch.ones(Sn, Sn), 1).bool()
        assert float(alpha[:, above].abs().max() if Sn > 1 else 0.0) == 0.0
        assert float((alpha * (1 - mask).unsqueeze(1)).abs().max()) == 0.0
        assert torch.allclose(alpha.sum(2), torch.ones(Bn, Sn, dtype=torch.float64), atol=1e-14)
        assert torch.equal(att_b, att_d) and torch.equal(alpha_b, alpha_d)          # the keyword's default is the old call
        if Sn > 1:
            assert float((alpha - alpha_b).abs().max()) > 1e-3


def _net(causal=None, **kw):
    from gan_ffn_amd import model as M
    torch.manual_seed(0)
    extra = {} if causal is None else {"causal": causal}
    extra.update({k: v for k, v in kw.items() if k != "listener"})
    return M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100, num_layers=1), M.VisualGenerator(100, num_layers=1),
                                 M.TextGenerator(100, num_layers=1), D_m=100, D_g=40, D_p=40, D_e=20, D_h=24, D_a=100, n_classes=6,
                                 listener_state=kw.get("listener", False), context_attention="general", dropout_rec=0.1, dropout=0.6,
                                 **extra)


def test_state_dict_of_the_causal_classifier():
    from gan_ffn_amd import dialogue_rnn as DR
    shapes = lambda net: {k: tuple(v.shape) for k, v in net.state_dict().items()}
    default, off, on = _net(), _net(False), _net(True)
    assert default.causal is False and off.causal is False and on.causal is True
    assert type(default.bi_model) is DR.BiModel and type(off.bi_model) is DR.BiModel and type(on.bi_model) is DR.UniModel
    assert shapes(off) == shapes(default) and list(off.state_dict()) == list(default.state_dict())
    want = {k: v for k, v in shapes(default).items() if not k.startswith("bi_model.dialog_rnn_r.")}
    assert any(k.startswith("bi_model.dialog_rnn_r.") for k in shapes(default))
    want.update({"bi_model.linear.weight": (24, 20), "bi_model.linear.bias": (24,),
                 "bi_model.matchatt.transform.weight": (20, 20), "bi_model.matchatt.transform.bias": (20,),
                 "bi_model.smax_fc.weight": (6, 24), "bi_model.smax_fc.bias": (6,)})
    assert shapes(on) == want
    assert shapes(default)["bi_model.linear.weight"] == (48, 40) and shapes(default)["bi_model.smax_fc.weight"] == (6, 48)
    assert "causal" not in on.state_dict()
    with pytest.raises(TypeError, match="unexpected keyword argument 'causl'"):        # the option is the only extra keyword
        _net(causl=True)
    assert "bi_model" in (DR.GAN_FFN_DialogueRNN.__doc__ or "") and "UniModel" in DR.GAN_FFN_DialogueRNN.__doc__


@pytest.mark.parametrize("listener", [False, True], ids=["", "listener"])
def test_nothing_after_step_t_reaches_the_causal_prediction(listener):
    """the property the feature exists for: change utterances and speakers after step t (same shapes) and the oracle's
    log_prob[:t+1] of that dialogue keeps every bit; BiModel's moves"""
    from gan_ffn_amd import dialogue_rnn as DR
    um = _uni("general", listener)
    torch.manual_seed(1)
    bi = DR.BiModel(n_classes=6, listener_state=listener, context_attention="general", dropout_rec=0.1, dropout=0.6,
                    **DIMS).double().eval()
    U, qmask, umask, _ = _inputs(DIMS["D_m"], lens=[9, 9, 9])
    lp = DCO.uni_head(um, U, qmask, umask)["log_prob"]
    with torch.no_grad():
        lp_bi = bi(U, qmask, umask)[0]
        lp_mod = um(U, qmask, umask)[0]
    g = torch.Generator().manual_seed(8)
    for t in (0, S // 2, S - 2):
        U2, q2 = U.clone(), qmask.clone()
        U2[t + 1:] = torch.rand(U2[t + 1:].shape, generator=g, dtype=torch.float64) * 2 - 1
        q2[t + 1:] = 1 - q2[t + 1:]                          # the other party speaks
        lp2 = DCO.uni_head(um, U2, q2, umask)["log_prob"]
        assert torch.equal(lp2[:t + 1], lp[:t + 1]), t
        assert float((lp2[t + 1:] - lp[t + 1:]).abs().max()) > 1e-6, t
        with torch.no_grad():
            assert torch.equal(um(U2, q2, umask)[0][:t + 1], lp_mod[:t + 1]), t
            assert float((bi(U2, q2, umask)[0][:t + 1] - lp_bi[:t + 1]).abs().max()) > 1e-6, t


def test_oracle_train_masks_and_gradients_are_consistent():
    """the oracle with explicit masks: gradients by name for every UniModel parameter, d_fusion zero after nothing (a step's loss
    reaches every earlier utterance), and masks of all ones give the eval result"""
    um = _uni("general", True)
    U, qmask, umask, label = _inputs(DIMS["D_m"])
    res = DCO.uni_head(um, U, qmask, umask, label, [1.0, 0.6, 0.4, 0.9, 0.7, 0.3])
    assert set(res["grads"]) == {n for n, _ in um.named_parameters()} and res["d_fusion"].shape == U.shape
    assert all(float(g.abs().max()) > 0 for n, g in res["grads"].items())
    H, He, Dh = DIMS["D_g"], DIMS["D_e"], DIMS["D_h"]
    o = torch.ones
    ones = dict(rec=sum(([o(B, H), o(B, 2, H), o(B, 2, H), o(B, He)] for _ in range(S)), []),
                join_f=o(S, B, He), hidden=o(S, B, Dh))
    res1 = DCO.uni_head(um, U, qmask, umask, label, [1.0, 0.6, 0.4, 0.9, 0.7, 0.3], ones)
    assert res1["loss"] == res["loss"] and torch.equal(res1["log_prob"], res["log_prob"])
    m = DCO.uni_masks(um, S, B, 7, 6, 7)
    assert len(m["rec"]) == 4 * S and m["join_f"].shape == (S, B, He) and m["hidden"].shape == (S, B, Dh)


# ---- what the new entry points refuse, before any launch (no GPU needed) ------------------------------------------------------
def _bufs(n=8):
    return [(C.c_float * n)() for _ in range(9)]


def _fwd(S_, B_, D_, flags, null=None):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    x, mem, mask, att, alpha, ts = _bufs()[:6]
    a = dict(x=x, mem=mem, mask=mask, att=att, alpha=alpha, ts=ts)
    if null:
        a[null] = None
    rc = lib.ganffn_general2_attention_fwd_mask(a["x"], a["mem"], a["mask"], C.c_uint32(flags), a["att"], a["alpha"], a["ts"],
                                                S_, B_, D_, None)
    return int(rc), (lib.ganffn_last_error() or b"").decode()


def _bwd(S_, B_, D_, flags, null=None):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    names = "d_att x mem mask alpha ts du dx dmem".split()
    a = dict(zip(names, _bufs()))
    if null:
        a[null] = None
    rc = lib.ganffn_general2_attention_bwd_mask(a["d_att"], a["x"], a["mem"], a["mask"], C.c_uint32(flags), a["alpha"], a["ts"],
                                                a["du"], a["dx"], a["dmem"], S_, B_, D_, None)
    return int(rc), (lib.ganffn_last_error() or b"").decode()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_general2_mask_entry_points_refuse_bad_arguments(call):
    rc, msg = call(1, 1, 4, 2)
    assert rc != 0 and "unknown flag bits 0x2" in msg, (rc, msg)
    rc, msg = call(1, 1, 4, 0x80000001)
    assert rc != 0 and "unknown flag bits" in msg, (rc, msg)
    for flags in (0, 1):
        rc, msg = call(129, 1, 4, flags)
        assert rc != 0 and "S=129" in msg, (rc, msg)
        rc, msg = call(1, 1, 1025, flags)
        assert rc != 0 and "D=1025" in msg, (rc, msg)
        for name in (["x", "mem", "mask", "att", "alpha", "ts"] if call is _fwd else
                     ["d_att", "x", "mem", "mask", "alpha", "ts", "du", "dx", "dmem"]):
            rc, msg = call(1, 1, 4, flags, null=name)
            assert rc != 0 and "null pointer" in msg, (name, rc, msg)


def test_bindings_of_the_mask_entry_points_are_the_old_lists_plus_flags():
    from gan_ffn_amd import _lib
    for what in ("fwd", "bwd"):
        old = _lib.SIGNATURES["ganffn_general2_attention_%s" % what]
        new = _lib.SIGNATURES["ganffn_general2_attention_%s_mask" % what]
        assert new[0] is old[0]
        rest = list(new[1])
        rest.remove(C.c_uint32)
        assert rest == list(old[1]) and len(new[1]) == len(old[1]) + 1
