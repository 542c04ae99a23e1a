"""The listener-state DialogueRNN (listener_state = True, model.py:899-921) without a GPU: the C ABI of its HIP path
(ganffn_drnn_listener_*: exported, bound, sized, argument errors reported) and the torch restatement against the reference
fixture tests/golden/dialogue_rnn_listener.npz (make_golden_listener.py: the reference's BiModel with general attention and
listener state, eval mode, formula weights)."""
import ctypes as C

import pytest
import torch

import formula as F_
from test_dialogue_rnn_cpu import DIMS, big_inputs, close, inputs
from util import check_summary, golden

LISTENER_SYMBOLS = ["ganffn_drnn_listener_saved_floats", "ganffn_drnn_listener_workspace_floats", "ganffn_drnn_listener_fwd",
                    "ganffn_drnn_listener_bwd"]
CASE = dict(context_attention="general", listener_state=True)


def test_library_exports_the_listener_entry_points_with_bindings():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    for s in LISTENER_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["ganffn_drnn_listener_fwd"][1]) == len(_lib.SIGNATURES["ganffn_drnn_fwd"][1]) + 1
    assert len(_lib.SIGNATURES["ganffn_drnn_listener_bwd"][1]) == len(_lib.SIGNATURES["ganffn_drnn_bwd"][1]) + 2
    assert C.sizeof(_lib.DrnnListenerPtrs) == 4 * C.sizeof(C.c_void_p)
    assert lib.ganffn_version() == 100


def test_listener_sizes_exceed_the_listener_free_ones_by_the_listener_regions():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    S, B, Dm, H, He = 94, 30, 100, 500, 100
    cfg = _lib.DrnnCfg(S, B, Dm, H, He, 0.1, 1)
    base_s, base_w = lib.ganffn_drnn_saved_floats(C.byref(cfg)), lib.ganffn_drnn_workspace_floats(C.byref(cfg))
    ls, lw = lib.ganffn_drnn_listener_saved_floats(C.byref(cfg)), lib.ganffn_drnn_listener_workspace_floats(C.byref(cfg))
    T = S * B
    assert base_s > 0 and base_w > 0
    # XL [T x 3H], QSP [T x H], four listener gate blocks [T x 2H]
    assert ls == base_s + T * 3 * H + T * H + 4 * T * 2 * H
    # GI_l, GH_l per step; dGI_l, dGH_l of all steps; four [B x H]-sized step buffers; two transposed weights
    assert lw == base_w + B * 3 * H + B * 6 * H + T * 3 * H + T * 6 * H + 6 * B * H + 2 * H * 3 * H


@pytest.mark.parametrize("bad,msg", [((7, 3, 100, 516, 100), b"512"), ((7, 33, 100, 500, 100), b"B=33"),
                                     ((7, 3, 102, 500, 100), b"multiples of 4"), ((113, 3, 100, 500, 100), b"S=113")])
def test_listener_argument_errors_are_reported_not_crashed(bad, msg):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    cfg = _lib.DrnnCfg(*bad, 0.1, 0)
    assert lib.ganffn_drnn_listener_saved_floats(C.byref(cfg)) < 0
    assert msg in lib.ganffn_last_error()
    assert lib.ganffn_drnn_listener_workspace_floats(C.byref(cfg)) < 0
    with pytest.raises(_lib.GanffnError):
        _lib.call("ganffn_drnn_listener_fwd", C.byref(cfg), 2, None, None, None, None, None, None, None, None, None, None,
                  C.c_uint64(0), None)
    with pytest.raises(_lib.GanffnError):
        _lib.call("ganffn_drnn_listener_bwd", C.byref(cfg), 2, None, None, None, None, None, None, None, None, None, None, None,
                  None, None, C.c_uint64(0), None)


def test_listener_needs_its_parameters():
    from gan_ffn_amd import _lib
    cfg = _lib.DrnnCfg(7, 3, 100, 500, 100, 0.1, 0)
    with pytest.raises(_lib.GanffnError, match="listener"):
        _lib.call("ganffn_drnn_listener_fwd", C.byref(cfg), 1, None, None, None, None, None, None, None, None, None, None,
                  C.c_uint64(0), None)


def test_predicates_split_on_listener_state():
    """dialogue_rnn_supported keeps meaning the listener-free recurrence; the listener one is its own predicate (CPU
    tensors: neither holds)"""
    from gan_ffn_amd import dialogue_rnn as DR, ops
    m = DR.DialogueRNN(100, 500, 500, 100, **CASE)
    U, qmask = torch.zeros(5, 2, 100), torch.zeros(5, 2, 2)
    assert not ops.dialogue_rnn_supported(m.dialogue_cell, U, qmask)
    assert not ops.dialogue_rnn_listener_supported(m.dialogue_cell, U, qmask)


def listener_model():
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(1)
    m = DR.BiModel(**DIMS, **CASE).eval()
    sd = F_.formula_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})       # reference keys, l_cell included
    assert any(k.endswith("l_cell.weight_hh") for k in sd)
    return m


def check_small(m, dev, lp_tol=2e-5, du_tol=1e-4, g_tol=2e-4):
    """BiModel `m` at the ragged (7, 3) batch against general_listener/* of dialogue_rnn_listener.npz"""
    g = golden("dialogue_rnn_listener")
    tag = "general_listener"
    U, qmask, umask = inputs()
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
    n = n_l = 0
    for k, p in m.named_parameters():
        key = "%s/grad/%s" % (tag, k)
        if p.grad is None:
            assert key not in g.files, k
            continue
        gr = p.grad.cpu()
        got = gr.numpy() if gr.numel() <= 4096 else gr.reshape(-1)[F_.sample_indices(gr.numel())].numpy()
        close(got, g[key], g_tol, "grad " + k)
        n += 1
        n_l += ".l_cell." in k
    assert n >= 24 and n_l == 8


def check_big(m, dev, rtol=5e-5, grtol=5e-4):
    """BiModel `m` at (94, 30) against the big_listener/* summaries"""
    g = golden("dialogue_rnn_listener")
    U, qmask, umask = big_inputs()
    Ut = torch.from_numpy(U).to(dev).requires_grad_(True)
    lp, alpha, alpha_f, alpha_b = m(Ut, torch.from_numpy(qmask).to(dev), torch.from_numpy(umask).to(dev))
    check_summary(g, "big_listener/log_prob", lp, rtol=rtol, atol=1e-6, what="log_prob", strict=True)
    check_summary(g, "big_listener/alpha", torch.stack(alpha, 0), rtol=rtol, atol=1e-7, what="alpha", strict=True)
    check_summary(g, "big_listener/alpha_f_last", alpha_f[-1], rtol=rtol, atol=1e-7, what="alpha_f", strict=True)
    check_summary(g, "big_listener/alpha_b_last", alpha_b[-1], rtol=rtol, atol=1e-7, what="alpha_b", strict=True)
    gy = torch.from_numpy(F_.formula_input("drnn.biggrad", lp.shape[0], lp.shape[1], lp.shape[2])) - 0.5
    (lp * gy.to(dev)).sum().backward()
    check_summary(g, "big_listener/dU", Ut.grad, rtol=grtol, atol=1e-7, what="dU", strict=True)
    n = n_l = 0
    for k, p in m.named_parameters():
        if p.grad is None:
            assert not any(f.startswith("big_listener/grad/%s/" % k) for f in g.files), k
            continue
        check_summary(g, "big_listener/grad/" + k, p.grad, rtol=grtol, atol=1e-7, what="grad " + k, strict=True, l2_rtol=2e-3)
        n += 1
        n_l += ".l_cell." in k
    assert n >= 24 and n_l == 8


def test_torch_restatement_matches_reference_fixture_small():
    check_small(listener_model(), "cpu")


def test_torch_restatement_matches_reference_fixture_at_configuration_5_size():
    check_big(listener_model(), "cpu")
