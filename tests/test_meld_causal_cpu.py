"""The causal MELD classifier without a GPU: the fp64 restatement (tests/meld_causal_oracle.py) pinned to
torch.nn.LSTM(bidirectional=False) — padded and packed — and to dialogue_rnn.MELDLSTMModel(causal=True) on the CPU; the module's
state_dict, its D_h == D_e rule, that the default model is what it was, and that the causal one never looks ahead."""
import pytest
import torch
from torch import nn

import meld_causal_oracle as CO

S0, B0, IN0, H0 = 7, 5, 8, 4
LENGTHS = [7, 1, 4, 2, 6]


def _params(lstm):
    return {k: v.detach().double().requires_grad_(True) for k, v in lstm.named_parameters()}


def _packed(lstm, x, lengths):
    seq = nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lengths), enforce_sorted=False)
    return nn.utils.rnn.pad_packed_sequence(lstm(seq)[0], total_length=x.shape[0])[0]


@pytest.mark.parametrize("lengths", [None, LENGTHS])
@pytest.mark.parametrize("L", [1, 3])
def test_oracle_layer_and_stack_are_torchs_unidirectional_lstm(L, lengths):
    torch.manual_seed(5 + L)
    lstm = nn.LSTM(IN0, H0, num_layers=L, bidirectional=False).double()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(S0, B0, IN0, generator=g, dtype=torch.float64)
    gy = torch.randn(S0, B0, H0, generator=g, dtype=torch.float64)
    xt = x.clone().requires_grad_(True)
    yt = lstm(xt)[0] if lengths is None else _packed(lstm, xt, lengths)
    (yt * gy).sum().backward()
    P = _params(lstm)
    xo = x.clone().requires_grad_(True)
    yo = CO.lstm_forward(xo, P, L, lengths=lengths)
    (yo * gy).sum().backward()
    assert float((yo - yt).abs().max()) < 1e-12
    assert float((xo.grad - xt.grad).abs().max()) < 1e-12
    for k, v in lstm.named_parameters():
        assert float((P[k].grad - v.grad).abs().max()) < 1e-12, k
    if lengths is not None:
        pad = ~torch.arange(S0).unsqueeze(1).lt(torch.tensor(lengths).unsqueeze(0))
        assert float(yo[pad].abs().max()) == 0.0 and float(xo.grad[pad].abs().max()) == 0.0
    if L == 1:
        assert torch.equal(CO.lstm_layer(x, P, 0, lengths), yo.detach())


def _model(D_m=16, D_e=8, D_h=8, seed=3, **kw):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    return DR.MELDLSTMModel(D_m, D_e, D_h, n_classes=7, dropout=0.5, **kw)


def _batch(S, B, D_m, lengths=None, seed=2):
    g = torch.Generator().manual_seed(seed)
    U = torch.randn(S, B, D_m, generator=g, dtype=torch.float64)
    umask = torch.ones(B, S, dtype=torch.float64)
    if lengths is not None:
        umask = torch.arange(S).unsqueeze(0).lt(torch.tensor(lengths).unsqueeze(1)).double()
    return U, umask


@pytest.mark.parametrize("lengths", [None, [9, 4, 1]])
def test_oracle_forward_is_the_causal_module_on_the_cpu(lengths):
    S, B = 9, 3
    m = _model(causal=True).double().eval()
    U, umask = _batch(S, B, 16, lengths)
    with torch.no_grad():
        log_prob, alpha, _, _ = m(U, None, umask)
    P = {k: v.detach() for k, v in m.state_dict().items()}
    _, lp, al = CO.forward(P, U, umask)
    assert float((lp - log_prob).abs().max()) < 1e-12
    assert float((al - torch.stack(alpha, 1)).abs().max()) < 1e-12
    assert float(al.triu(1).abs().max()) == 0.0                    # nothing above the diagonal


def test_oracle_forward_is_the_packed_causal_module_on_the_cpu():
    S, B, lengths = 9, 3, [9, 4, 1]
    m = _model(causal=True, packed=True).double().eval()
    U, umask = _batch(S, B, 16, lengths)
    with torch.no_grad():
        log_prob = m(U, None, umask)[0]
    P = {k: v.detach() for k, v in m.state_dict().items()}
    lp = CO.forward(P, U, umask, lengths=lengths)[1]
    assert float((lp - log_prob).abs().max()) < 1e-12


def test_state_dicts():
    from gan_ffn_amd import dialogue_rnn as DR
    c = _model(causal=True).state_dict()
    assert not [k for k in c if k.endswith("_reverse")]
    assert [k for k in c if k.startswith("lstm.")] == CO.trained_names()[:16]
    assert tuple(c["matchatt.transform.weight"].shape) == (8, 8)
    assert tuple(c["linear.weight"].shape) == (8, 8) and tuple(c["smax_fc.weight"].shape) == (7, 8)
    assert tuple(c["lstm.weight_ih_l1"].shape) == (32, 8)          # layer 1 reads an H-wide input
    # the default model: what a MELDLSTMModel built without the keyword is
    torch.manual_seed(3)
    plain = DR.MELDLSTMModel(16, 8, 16, n_classes=7, dropout=0.5)
    d = _model(D_h=16, causal=False)
    assert not plain.causal and not d.causal and plain.lstm.bidirectional and d.lstm.bidirectional
    sp, sd = plain.state_dict(), d.state_dict()
    assert list(sp) == list(sd)
    for k in sp:
        assert sp[k].shape == sd[k].shape and torch.equal(sp[k], sd[k]), k
    assert len([k for k in sd if k.endswith("_reverse")]) == 16
    assert tuple(sd["matchatt.transform.weight"].shape) == (16, 16)


def test_causal_att2_needs_D_h_equal_D_e():
    m = _model(D_h=16, causal=True).double().eval()
    U, umask = _batch(4, 2, 16)
    with pytest.raises(ValueError, match="D_h == D_e"):
        m(U, None, umask)
    with torch.no_grad():
        assert m(U, None, umask, att2=False)[0].shape == (4, 2, 7)    # the other branch goes through linear: any D_h


@pytest.mark.parametrize("t", [0, 4, 8])
def test_causal_module_never_looks_ahead_on_the_cpu(t):
    S, B = 9, 3
    m = _model(causal=True).double().eval()
    U, umask = _batch(S, B, 16)
    U2 = U.clone()
    U2[t + 1:] = torch.randn(S - t - 1, B, 16, generator=torch.Generator().manual_seed(9), dtype=torch.float64) * 1e3
    with torch.no_grad():
        a, b = m(U, None, umask)[0], m(U2, None, umask)[0]
        assert torch.equal(a[:t + 1], b[:t + 1])
        if t + 1 < S:
            assert not torch.equal(a[t + 1:], b[t + 1:])
            # and the default model does look ahead: the test can tell the two apart
            d = _model(D_h=16).double().eval()
            assert not torch.equal(d(U, None, umask)[0][:t + 1], d(U2, None, umask)[0][:t + 1])
