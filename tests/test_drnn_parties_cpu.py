"""The multi-party DialogueRNN (qmask [S x B x P], model.py:861-926; MELD's speaker one-hots are 9 wide) without a GPU: the
C ABI of its HIP path (ganffn_drnn_party_*: exported, bound, sized — the two-party sizes at P = 2, growing with P by the
party regions —, party counts outside [1, GANFFN_DRNN_MAX_PARTIES] reported as errors, not crashed on) and the torch
restatement against the reference fixture tests/golden/dialogue_rnn_parties.npz (make_golden_parties.py: the reference's
BiModel with 1, 3 and 9 parties, eval mode, formula weights)."""
import ctypes as C
import os
import re

import pytest
import torch

import formula as F_
from test_dialogue_rnn_cpu import DIMS, close
from util import check_summary, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTY_SYMBOLS = ["ganffn_drnn_party_saved_floats", "ganffn_drnn_party_workspace_floats", "ganffn_drnn_party_fwd",
                 "ganffn_drnn_party_bwd"]
CASES = {"general": dict(context_attention="general", listener_state=False),
         "general_listener": dict(context_attention="general", listener_state=True),
         "concat_listener": dict(context_attention="concat", listener_state=True),
         "simple": dict(context_attention="simple", listener_state=False)}
RUNS = [("general", 1), ("general", 9), ("general_listener", 3), ("concat_listener", 9), ("simple", 3)]
ATTS = [("general", 0), ("simple", 0), ("dot", 0), ("general2", 0), ("concat", 100)]


def header_max_parties():
    src = open(os.path.join(ROOT, "include", "ganffn.h")).read()
    return int(re.search(r"#define\s+GANFFN_DRNN_MAX_PARTIES\s+(\d+)", src).group(1))


PMAX = header_max_parties()


def _cfg(att):
    from gan_ffn_amd import _lib
    H = 100 if att == "dot" else 500                      # dot: D_m == D_g
    return _lib.DrnnCfg(94, 30, 100, H, 100, 0.1, 1)


def _sizes(cfg, a, listener, P):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    return (lib.ganffn_drnn_party_saved_floats(C.byref(cfg), C.byref(a), listener, P),
            lib.ganffn_drnn_party_workspace_floats(C.byref(cfg), C.byref(a), listener, P))


def test_library_exports_the_party_entry_points_with_bindings():
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    for s in PARTY_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    for s in ("fwd", "bwd", "saved_floats", "workspace_floats"):          # the _att_ arguments plus the party count
        assert len(_lib.SIGNATURES["ganffn_drnn_party_" + s][1]) == len(_lib.SIGNATURES["ganffn_drnn_att_" + s][1]) + 1
    assert ops.DRNN_MAX_PARTIES == PMAX >= 9
    assert lib.ganffn_version() == 100


@pytest.mark.parametrize("listener", [0, 1])
@pytest.mark.parametrize("att,da", ATTS)
def test_two_party_sizes_are_the_existing_sizes(att, da, listener):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    cfg = _cfg(att)
    a = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], da)
    want = (lib.ganffn_drnn_att_saved_floats(C.byref(cfg), C.byref(a), listener),
            lib.ganffn_drnn_att_workspace_floats(C.byref(cfg), C.byref(a), listener))
    assert want[0] > 0 and want[1] > 0
    assert _sizes(cfg, a, listener, 2) == want
    if att == "general":
        old = (lib.ganffn_drnn_listener_saved_floats(C.byref(cfg)), lib.ganffn_drnn_listener_workspace_floats(C.byref(cfg))) \
            if listener else (lib.ganffn_drnn_saved_floats(C.byref(cfg)), lib.ganffn_drnn_workspace_floats(C.byref(cfg)))
        assert want == old


@pytest.mark.parametrize("listener", [0, 1])
@pytest.mark.parametrize("att,da", ATTS)
def test_sizes_grow_by_the_party_regions(att, da, listener):
    from gan_ffn_amd import _lib
    cfg = _cfg(att)
    a = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], da)
    S, B, H = cfg.S, cfg.B, cfg.H
    T, T1 = S * B, (S + 1) * B
    s2, w2 = _sizes(cfg, a, listener, 2)
    for P in (1, 3, 9, PMAX):
        s, w = _sizes(cfg, a, listener, P)
        # Q [(S+1) B x P x H]; with listener state its four gate blocks [S B x P x H]
        assert s == s2 + (P - 2) * (T1 * H + (4 * T * H if listener else 0)), P
        # the dQ ping-pong 2 x [B x P x H]; with listener state GH_l [B x P x 3H], dGH_l [S B x P x 3H], dQ_l and dh'z [B x P x H]
        assert w == w2 + (P - 2) * (2 * B * H + ((3 * B * H + 3 * T * H + 2 * B * H) if listener else 0)), P


@pytest.mark.parametrize("P", [0, -1, PMAX + 1, 64])
def test_party_counts_outside_the_limit_are_reported_not_crashed(P):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    cfg = _lib.DrnnCfg(7, 3, 100, 500, 100, 0.1, 0)
    a = _lib.DrnnAtt(0, 0)
    for listener in (0, 1):
        assert lib.ganffn_drnn_party_saved_floats(C.byref(cfg), C.byref(a), listener, P) < 0
        assert b"parties=%d" % P in lib.ganffn_last_error()
        assert lib.ganffn_drnn_party_workspace_floats(C.byref(cfg), C.byref(a), listener, P) < 0
    with pytest.raises(_lib.GanffnError, match="parties"):
        _lib.call("ganffn_drnn_party_fwd", C.byref(cfg), C.byref(a), P, 2, *([None] * 11), C.c_uint64(0), None)
    with pytest.raises(_lib.GanffnError, match="parties"):
        _lib.call("ganffn_drnn_party_bwd", C.byref(cfg), C.byref(a), P, 2, *([None] * 15), C.c_uint64(0), None)


def test_predicates_on_cpu_tensors_stay_false():
    from gan_ffn_amd import dialogue_rnn as DR, ops
    m = DR.DialogueRNN(100, 500, 500, 100, context_attention="general")
    assert not ops.dialogue_rnn_supported(m.dialogue_cell, torch.zeros(5, 2, 100), torch.zeros(5, 2, 9))


def party_model(case):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(1)
    m = DR.BiModel(**DIMS, **CASES[case]).eval()
    sd = F_.formula_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def small_inputs(g, tag):
    qmask, umask = g[tag + "/qmask"], g[tag + "/umask"]
    S, B = qmask.shape[:2]
    U = F_.formula_input("drnn.U", S, B, 100) * umask.T[:, :, None]        # make_golden.drnn_inputs()
    return U, qmask, umask


def check_small(m, case, P, dev, lp_tol=2e-5, du_tol=1e-4, g_tol=2e-4):
    """BiModel `m` at the ragged (7, 3) batch with P parties against <case>/P<P>/* of dialogue_rnn_parties.npz"""
    g = golden("dialogue_rnn_parties")
    tag = "%s/P%d" % (case, P)
    U, qmask, umask = small_inputs(g, tag)
    assert qmask.shape[2] == P
    Ut = torch.from_numpy(U).to(dev).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask).to(dev), torch.from_numpy(umask).to(dev))
    close(lp.detach().cpu().numpy(), g["%s/log_prob" % tag], lp_tol, "log_prob")
    close(torch.stack(alpha, 0).detach().cpu().numpy(), g["%s/alpha" % tag], lp_tol, "alpha")
    for name, al in (("alpha_f", alpha_f), ("alpha_b", alpha_b)):
        assert len(al) == int(g["%s/%s/n" % (tag, name)])
        for t, a in enumerate(al):
            close(a.detach().cpu().numpy(), g["%s/%s/%d" % (tag, name, t)], lp_tol, "%s[%d]" % (name, t))
    gy = torch.from_numpy(F_.formula_input("drnn.grad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy.to(dev)).sum().backward()
    close(Ut.grad.cpu().numpy(), g["%s/dU" % tag], du_tol, "dU")
    n = 0
    for k, p in m.named_parameters():
        key = "%s/grad/%s" % (tag, k)
        if p.grad is None:
            assert key not in g.files, k
            continue
        gr = p.grad.cpu()
        got = gr.numpy() if gr.numel() <= 4096 else gr.reshape(-1)[F_.sample_indices(gr.numel())].numpy()
        close(got, g[key], g_tol, "grad " + k)
        n += 1
    assert n >= 22


def check_big(m, dev, rtol=5e-5, grtol=5e-4):
    """BiModel `m` (general, no listener) at (33, 32) with 9 parties against the big_parties/* summaries"""
    g = golden("dialogue_rnn_parties")
    qmask, umask = g["big_parties/qmask"], g["big_parties/umask"]
    S, B, P = qmask.shape
    assert (S, B, P) == (33, 32, 9)
    U = F_.formula_input("drnn.partiesU", S, B, 100) * umask.T[:, :, None]
    Ut = torch.from_numpy(U).to(dev).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask).to(dev), torch.from_numpy(umask).to(dev))
    check_summary(g, "big_parties/log_prob", lp, rtol=rtol, atol=1e-6, what="log_prob", strict=True)
    check_summary(g, "big_parties/alpha", torch.stack(alpha, 0), rtol=rtol, atol=1e-7, what="alpha", strict=True)
    check_summary(g, "big_parties/alpha_f_last", alpha_f[-1], rtol=rtol, atol=1e-7, what="alpha_f", strict=True)
    check_summary(g, "big_parties/alpha_b_last", alpha_b[-1], rtol=rtol, atol=1e-7, what="alpha_b", strict=True)
    gy = torch.from_numpy(F_.formula_input("drnn.partiesgrad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy.to(dev)).sum().backward()
    check_summary(g, "big_parties/dU", Ut.grad, rtol=grtol, atol=1e-7, what="dU", strict=True)
    n = 0
    for k, p in m.named_parameters():
        if p.grad is None:
            continue
        check_summary(g, "big_parties/grad/" + k, p.grad, rtol=grtol, atol=1e-7, what="grad " + k, strict=True, l2_rtol=2e-3)
        n += 1
    assert n >= 24


@pytest.mark.parametrize("case,P", RUNS)
def test_torch_restatement_matches_reference_fixture_small(case, P):
    check_small(party_model(case), case, P, "cpu")


def test_torch_restatement_matches_reference_fixture_at_meld_size():
    check_big(party_model("general"), "cpu")
