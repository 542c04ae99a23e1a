"""The packed-sequence LSTM rule on the CPU: tests/lstm_packed_oracle.py (the fp64 restatement the GPU tests compare
csrc/lstm.hip's packed entry points against) pinned to torch's own pack_padded_sequence -> nn.LSTM -> pad_packed_sequence, and
MELDLSTMModel(packed=True)'s CPU route and constructor contract."""
import pytest
import torch
import torch.nn as nn

import lstm_packed_oracle as PO
from oracle import ganffn_oracle as O
from oracle import lstm_oracle as LO

S, B, IN, H, L = 7, 5, 8, 4, 2
LENGTHS = [7, 1, 4, 2, 6]


def torch_packed(lstm, x, lengths):
    seq = nn.utils.rnn.pack_padded_sequence(x, torch.as_tensor(lengths, dtype=torch.int64), enforce_sorted=False)
    return nn.utils.rnn.pad_packed_sequence(lstm(seq)[0], total_length=x.shape[0])[0]


def test_oracle_equals_torch_packed_lstm_forward_and_every_gradient():
    """fp64, (S, B, In, H, L) = (7, 5, 8, 4, 2), lengths [7, 1, 4, 2, 6]; the upstream gradient is random at padded positions too
    — on the oracle's side scaled to 1e3 there, on torch's side as drawn: pad_packed_sequence drops it, the rule's select must."""
    torch.manual_seed(5)
    lstm = nn.LSTM(IN, H, num_layers=L, bidirectional=True).double()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(S, B, IN, generator=g, dtype=torch.float64)
    gy = torch.randn(S, B, 2 * H, generator=g, dtype=torch.float64)
    valid = PO.valid_mask(LENGTHS, S)
    xt = x.clone().requires_grad_(True)
    yt = torch_packed(lstm, xt, LENGTHS)
    (yt * gy).sum().backward()
    P = {k: v.detach().clone().requires_grad_(True) for k, v in lstm.named_parameters()}
    # the oracle's x carries junk at padded positions as well: its values there must not matter
    xo = torch.where(valid, x, 1e3 * torch.randn(S, B, IN, generator=g, dtype=torch.float64)).requires_grad_(True)
    yo = PO.lstm_forward(xo, LENGTHS, P, L)
    (yo * torch.where(valid, gy, 1e3 * gy)).sum().backward()
    d = lambda a, b: float((a - b).abs().max())
    print("forward %.1e dx %.1e" % (d(yo.detach(), yt.detach()), d(xo.grad, xt.grad)))
    assert d(yo.detach(), yt.detach()) < 1e-12
    assert d(xo.grad, xt.grad) < 1e-12
    assert torch.equal(yo.detach()[~valid.expand_as(yo)], torch.zeros(int((~valid).sum()) * 2 * H, dtype=torch.float64))
    assert float(xo.grad[~valid.expand_as(x)].abs().max()) == 0.0
    for k, v in lstm.named_parameters():
        assert d(P[k].grad, v.grad) < 1e-12, k
    # and the padded run really differs at valid positions (the defect the packed form removes)
    with torch.no_grad():
        y_pad = LO.lstm_forward(x, {k: v.detach() for k, v in P.items()}, L)
    assert float((y_pad - yt.detach())[valid.expand_as(y_pad)].abs().max()) > 1e-3


@pytest.mark.parametrize("train", [False, True])
def test_full_lengths_are_the_unpacked_oracle_exactly(train):
    torch.manual_seed(6)
    lstm = nn.LSTM(IN, H, num_layers=3, bidirectional=True).double()
    P = {k: v.detach() for k, v in lstm.named_parameters()}
    x = torch.randn(S, B, IN, dtype=torch.float64)
    a = PO.lstm_forward(x, [S] * B, P, 3, 0.5, rng=O.Rng(77, 3, train))
    b = LO.lstm_forward(x, P, 3, 0.5, rng=O.Rng(77, 3, train))
    assert torch.equal(a, b)
    assert torch.equal(PO.lstm_forward(x, [S + 4] * B, P, 3), LO.lstm_forward(x, P, 3))          # lengths > S count as S
    if train:
        assert not torch.equal(a, LO.lstm_forward(x, P, 3))


def test_model_packed_cpu_route_is_torchs_pack_and_unpack():
    from gan_ffn_amd.dialogue_rnn import MELDLSTMModel
    torch.manual_seed(7)
    m = MELDLSTMModel(16, 8, 16, packed=True).eval()
    plain = MELDLSTMModel(16, 8, 16).eval()
    plain.load_state_dict(m.state_dict())
    Sm, lengths = 6, [6, 2, 1, 4]
    U = torch.randn(Sm, len(lengths), 16)
    umask = (torch.arange(Sm).unsqueeze(0) < torch.tensor(lengths).unsqueeze(1)).float()
    with torch.no_grad():
        lp, alpha, _, _ = m(U, None, umask)
        em = torch_packed(m.lstm, U, lengths)
        att, _ = m.matchatt.general2_all_queries(em, umask)
        want = torch.log_softmax(m.smax_fc(torch.nn.functional.hardswish(em + torch.nn.functional.hardswish(att))), 2)
        lp_plain = plain(U, None, umask)[0]
    assert torch.equal(lp, want) and len(alpha) == Sm
    assert not torch.allclose(lp[:2, 1], lp_plain[:2, 1], atol=1e-6)      # the short dialogue's valid steps change
    assert torch.allclose(lp[:, 0], lp_plain[:, 0], atol=1e-6)            # the full-length one's do not
    # the property: a dialogue inside the batch = the dialogue alone
    with torch.no_grad():
        alone = m(U[:2, 1:2].contiguous(), None, torch.ones(1, 2))[0]
    assert torch.allclose(lp[:2, 1:2], alone, atol=1e-6)


def test_packed_defaults_to_false_and_leaves_the_state_dict_alone():
    from gan_ffn_amd.dialogue_rnn import MELDLSTMModel
    a, b = MELDLSTMModel(16, 8, 16), MELDLSTMModel(16, 8, 16, packed=True)
    assert a.packed is False and b.packed is True
    assert list(a.state_dict()) == list(b.state_dict())
    assert "packed" not in dict(b.named_parameters()) and "packed" not in dict(b.named_buffers())
    import inspect
    from gan_ffn_amd import artifacts, engine, ops
    assert inspect.signature(MELDLSTMModel.__init__).parameters["packed"].default is False
    assert inspect.signature(engine.MeldEngine.__init__).parameters["packed"].default is False
    assert inspect.signature(artifacts.run_meld_training).parameters["packed"].default is False
    assert inspect.signature(ops.lstm_forward).parameters["lengths"].default is None


def test_null_lengths_is_an_argument_error():
    import ctypes as C
    from gan_ffn_amd import _lib
    lib = _lib.load()
    cfg = _lib.LstmCfg(4, 2, 8, 4)
    for name in ("ganffn_lstm_packed_layer_fwd", "ganffn_lstm_packed_layer_bwd"):
        with pytest.raises(_lib.GanffnError, match="null lengths"):
            _lib.call(name, C.byref(cfg), *([None] * (len(_lib.SIGNATURES[name][1]) - 1)))
    scfg = _lib.LstmStackCfg(4, 2, 8, 4, 2, 0.0, 0)
    for name in ("ganffn_lstm_stack_packed_fwd", "ganffn_lstm_stack_packed_bwd"):
        args = [None] * (len(_lib.SIGNATURES[name][1]) - 1)
        args[-2] = C.c_uint64(0)
        with pytest.raises(_lib.GanffnError, match="null lengths"):
            _lib.call(name, C.byref(scfg), *args)
