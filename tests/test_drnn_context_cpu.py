"""The other context attention types of the DialogueRNN (dot, general2, concat; model.py:134-194) without a GPU: the C ABI
of their HIP path (ganffn_drnn_att_*: declared, exported, bound, argument errors reported) and the torch restatement of
gan_ffn_amd/dialogue_rnn.py against the reference fixtures tests/golden/dialogue_rnn_context*.npz (make_golden_context.py:
the reference's BiModel, eval mode, formula weights) — the oracle the GPU tests compare against."""
import ctypes as C

import pytest
import torch

import formula as F_
from test_dialogue_rnn_cpu import DIMS, big_inputs, close, inputs
from util import check_summary, golden

ATT_SYMBOLS = ["ganffn_drnn_att_saved_floats", "ganffn_drnn_att_workspace_floats", "ganffn_drnn_att_fwd", "ganffn_drnn_att_bwd"]
CASES = {
    "general2": dict(context_attention="general2"),
    "concat": dict(context_attention="concat"),
    "dot": dict(context_attention="dot", D_g=100, D_p=100),
    "general2_listener": dict(context_attention="general2", listener_state=True),
    "concat_listener": dict(context_attention="concat", listener_state=True),
}
ATT_PARAMS = {"general2": ("attention.transform.weight", "attention.transform.bias"),
              "concat": ("attention.transform.weight", "attention.vector_prod.weight"), "dot": ()}


def context_model(case):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(1)
    d = dict(DIMS)
    d.update(CASES[case])
    m = DR.BiModel(**d).eval()
    sd = F_.formula_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})       # reference keys
    return m


def _n_att(case):
    return len(ATT_PARAMS[case.split("_")[0]])


def check_small(m, case, dev, lp_tol=2e-5, du_tol=1e-4, g_tol=2e-4):
    """BiModel `m` at the ragged (7, 3) batch against <case>/* of dialogue_rnn_context.npz"""
    g = golden("dialogue_rnn_context")
    U, qmask, umask = inputs()
    Ut = torch.from_numpy(U).to(dev).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask).to(dev), torch.from_numpy(umask).to(dev))
    close(lp.detach().cpu().numpy(), g["%s/log_prob" % case], lp_tol, "log_prob")
    close(torch.stack(alpha, 0).detach().cpu().numpy(), g["%s/alpha" % case], lp_tol, "alpha")
    for name, al in (("alpha_f", alpha_f), ("alpha_b", alpha_b)):
        assert len(al) == int(g["%s/%s/n" % (case, name)])
        for t, a in enumerate(al):
            close(a.detach().cpu().numpy(), g["%s/%s/%d" % (case, name, t)], lp_tol, "%s[%d]" % (name, t))
    gy = torch.from_numpy(F_.formula_input("drnn.grad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy.to(dev)).sum().backward()
    close(Ut.grad.cpu().numpy(), g["%s/dU" % case], du_tol, "dU")
    n = n_att = 0
    for k, p in m.named_parameters():
        key = "%s/grad/%s" % (case, k)
        if p.grad is None:
            assert key not in g.files, k
            continue
        gr = p.grad.cpu()
        got = gr.numpy() if gr.numel() <= 4096 else gr.reshape(-1)[F_.sample_indices(gr.numel())].numpy()
        close(got, g[key], g_tol, "grad " + k)
        n += 1
        n_att += ".attention." in k and "matchatt" not in k
    assert n >= 22 and n_att == 2 * _n_att(case)
    if case == "dot":           # no attention parameter, so no gradient for one
        assert not any(f.startswith("dot/grad/") and ".dialogue_cell.attention." in f for f in g.files)


def check_big(m, case, dev, rtol=5e-5, grtol=5e-4):
    """BiModel `m` at (94, 30) against the big_<case>/* summaries"""
    g = golden("dialogue_rnn_context_big")
    tag = "big_" + case
    U, qmask, umask = big_inputs()
    Ut = torch.from_numpy(U).to(dev).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask).to(dev), torch.from_numpy(umask).to(dev))
    check_summary(g, tag + "/log_prob", lp, rtol=rtol, atol=1e-6, what="log_prob", strict=True)
    check_summary(g, tag + "/alpha", torch.stack(alpha, 0), rtol=rtol, atol=1e-7, what="alpha", strict=True)
    check_summary(g, tag + "/alpha_f_last", alpha_f[-1], rtol=rtol, atol=1e-7, what="alpha_f", strict=True)
    check_summary(g, tag + "/alpha_b_last", alpha_b[-1], rtol=rtol, atol=1e-7, what="alpha_b", strict=True)
    gy = torch.from_numpy(F_.formula_input("drnn.biggrad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy.to(dev)).sum().backward()
    check_summary(g, tag + "/dU", Ut.grad, rtol=grtol, atol=1e-7, what="dU", strict=True)
    n = 0
    for k, p in m.named_parameters():
        if p.grad is None:
            assert not any(f.startswith("%s/grad/%s/" % (tag, k)) for f in g.files), k
            continue
        check_summary(g, tag + "/grad/" + k, p.grad, rtol=grtol, atol=1e-7, what="grad " + k, strict=True, l2_rtol=2e-3)
        n += 1
    assert n >= 22


@pytest.mark.parametrize("case", sorted(CASES))
def test_torch_restatement_matches_reference_fixture_small(case):
    check_small(context_model(case), case, "cpu")


@pytest.mark.parametrize("case", ["general2", "concat"])
def test_torch_restatement_matches_reference_fixture_at_configuration_5_size(case):
    check_big(context_model(case), case, "cpu")


def test_library_exports_the_attention_entry_points_with_bindings():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    for s in ATT_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    # cfg and att descriptor first, then ndir, the listener-path arguments plus the attention parameters (and gradients)
    assert len(_lib.SIGNATURES["ganffn_drnn_att_fwd"][1]) == len(_lib.SIGNATURES["ganffn_drnn_listener_fwd"][1]) + 2
    assert len(_lib.SIGNATURES["ganffn_drnn_att_bwd"][1]) == len(_lib.SIGNATURES["ganffn_drnn_listener_bwd"][1]) + 3
    assert C.sizeof(_lib.DrnnAtt) == 8 and C.sizeof(_lib.DrnnAttPtrs) == 3 * C.sizeof(C.c_void_p)
    assert _lib.DRNN_ATT_TYPES == {"general": 0, "simple": 1, "dot": 2, "general2": 3, "concat": 4}


def test_attention_sizes_add_the_type_regions_behind_the_base_layout():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    S, B, Dm, H, He, Da = 94, 30, 100, 500, 100, 100
    cfg = _lib.DrnnCfg(S, B, Dm, H, He, 0.1, 1)
    T = S * B
    base = [(lib.ganffn_drnn_saved_floats(C.byref(cfg)), lib.ganffn_drnn_workspace_floats(C.byref(cfg))),
            (lib.ganffn_drnn_listener_saved_floats(C.byref(cfg)), lib.ganffn_drnn_listener_workspace_floats(C.byref(cfg)))]
    for listener in (0, 1):
        bs, bw = base[listener]

        def sizes(t, da=0):
            a = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[t], da)
            return lib.ganffn_drnn_att_saved_floats(C.byref(cfg), C.byref(a), listener), \
                lib.ganffn_drnn_att_workspace_floats(C.byref(cfg), C.byref(a), listener)
        assert sizes("general") == (bs, bw) and sizes("simple") == (bs, bw)
        assert sizes("general2") == (bs + B * S * S, bw)                        # saved tanh scores
        assert sizes("concat", Da) == (bs + 2 * T * Da, bw + 3 * T * Da)        # X, P; dX, dP, v partials
    cfg_dot = _lib.DrnnCfg(S, B, 100, 100, He, 0.1, 1)
    a = _lib.DrnnAtt(2, 0)
    assert lib.ganffn_drnn_att_saved_floats(C.byref(cfg_dot), C.byref(a), 0) == lib.ganffn_drnn_saved_floats(C.byref(cfg_dot))


@pytest.mark.parametrize("att,da,dims,msg", [(7, 0, (7, 3, 100, 500, 100), b"unknown attention type 7"),
                                             (-1, 0, (7, 3, 100, 500, 100), b"unknown attention type"),
                                             (4, 102, (7, 3, 100, 500, 100), b"D_a=102"),
                                             (4, 516, (7, 3, 100, 500, 100), b"D_a=516"),
                                             (4, 0, (7, 3, 100, 500, 100), b"D_a=0"),
                                             (2, 0, (7, 3, 100, 500, 100), b"D_m == D_g"),
                                             (3, 0, (7, 3, 100, 516, 100), b"512")])
def test_attention_argument_errors_are_reported_not_crashed(att, da, dims, msg):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    cfg = _lib.DrnnCfg(*dims, 0.1, 0)
    a = _lib.DrnnAtt(att, da)
    assert lib.ganffn_drnn_att_saved_floats(C.byref(cfg), C.byref(a), 0) < 0
    assert msg in lib.ganffn_last_error()
    assert lib.ganffn_drnn_att_workspace_floats(C.byref(cfg), C.byref(a), 1) < 0
    with pytest.raises(_lib.GanffnError, match=msg.decode()):
        _lib.call("ganffn_drnn_att_fwd", C.byref(cfg), C.byref(a), 1, *([None] * 11), C.c_uint64(0), None)
    with pytest.raises(_lib.GanffnError, match=msg.decode()):
        _lib.call("ganffn_drnn_att_bwd", C.byref(cfg), C.byref(a), 1, *([None] * 15), C.c_uint64(0), None)


def test_null_attention_descriptor_and_parameters_are_reported():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    cfg = _lib.DrnnCfg(7, 3, 100, 500, 100, 0.1, 0)
    assert lib.ganffn_drnn_att_saved_floats(C.byref(cfg), None, 0) < 0
    assert b"null attention descriptor" in lib.ganffn_last_error()
    with pytest.raises(_lib.GanffnError, match="null attention descriptor"):
        _lib.call("ganffn_drnn_att_fwd", C.byref(cfg), None, 1, *([None] * 11), C.c_uint64(0), None)
    for t in (0, 1, 3, 4):               # every type but dot has parameters
        a = _lib.DrnnAtt(t, 100)
        with pytest.raises(_lib.GanffnError, match="null attention parameters"):
            _lib.call("ganffn_drnn_att_fwd", C.byref(cfg), C.byref(a), 1, *([None] * 11), C.c_uint64(0), None)


@pytest.mark.parametrize("case", sorted(CASES))
def test_predicates_are_false_on_cpu_tensors(case):
    from gan_ffn_amd import dialogue_rnn as DR, ops
    d = dict(D_m=100, D_g=500, D_p=500, D_e=100)
    d.update({k: v for k, v in CASES[case].items() if k in ("D_g", "D_p")})
    m = DR.DialogueRNN(context_attention=CASES[case]["context_attention"], listener_state=CASES[case].get("listener_state", False),
                       **d)
    U, qmask = torch.zeros(5, 2, 100), torch.zeros(5, 2, 2)
    assert not ops.dialogue_rnn_supported(m.dialogue_cell, U, qmask)
    assert not ops.dialogue_rnn_listener_supported(m.dialogue_cell, U, qmask)
    assert ops.drnn_att_limits_hold(m.dialogue_cell)


def test_attention_limits():
    from gan_ffn_amd import dialogue_rnn as DR, ops
    assert not ops.drnn_att_limits_hold(DR.DialogueRNN(100, 100, 100, 100, context_attention="concat", D_a=102).dialogue_cell)
    assert not ops.drnn_att_limits_hold(DR.DialogueRNN(100, 100, 100, 100, context_attention="concat", D_a=516).dialogue_cell)
    assert ops.drnn_att_limits_hold(DR.DialogueRNN(100, 100, 100, 100, context_attention="concat", D_a=512).dialogue_cell)
    assert ops.drnn_att_limits_hold(DR.DialogueRNN(100, 100, 100, 100, context_attention="dot").dialogue_cell)
    assert ops.drnn_att_limits_hold(DR.DialogueRNN(100, 500, 500, 100, context_attention="simple").dialogue_cell)
