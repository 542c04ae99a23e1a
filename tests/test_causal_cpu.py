"""Causal self-attention on the CPU: the causal restatement of the oracle (tests/causal_oracle.py) against stock torch's
mask = triu(-inf, 1), with and without src_key_padding_mask; the property the feature exists for (a prefix of a dialogue run alone
gives the rows of the full run: nothing looks ahead); and the `causal` switch of GAN_FFN, Phase2Engine and run_training."""
import inspect

import pytest
import torch

from oracle import ganffn_oracle as O
from oracle import stock_modules as SM
from causal_oracle import causal_attention
from key_len_oracle import masked_attention, valid_rows

CASES = [("AcousticGenerator", 17, [17, 16, 1, 5]), ("VisualGenerator", 9, [9, 2, 1])]


def _stack(name, S, B, seed=5):
    torch.manual_seed(seed)
    net = SM.StockNet(name, 100, 0.2, num_layers=2).double().eval()
    E = net.position_encoding.pe.shape[2]
    P = {k: v.detach() for k, v in net.state_dict().items()}
    x = torch.rand(S, B, E, dtype=torch.float64)
    H = net.encoder_layer.self_attn.num_heads
    return net, P, H, x


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    name, S, lengths = request.param
    net, P, H, x = _stack(name, S, len(lengths))
    with torch.no_grad():
        plain = O.encoder_stack(x, P, H, None, n_layers=2)
        with causal_attention():
            causal = O.encoder_stack(x, P, H, None, n_layers=2)
        with causal_attention(lengths):
            both = O.encoder_stack(x, P, H, None, n_layers=2)
    return dict(net=net, P=P, H=H, x=x, S=S, lengths=lengths, plain=plain, causal=causal, both=both)


def _triu(S):
    return torch.triu(torch.full((S, S), float("-inf"), dtype=torch.float64), 1)


def test_causal_oracle_is_stock_torch_with_the_triu_mask(case):
    S, net = case["S"], case["net"]
    with torch.no_grad():
        want = net.transformer_encoder(net.position_encoding(case["x"]), mask=_triu(S))
    err = float((case["causal"] - want).abs().max())
    print("causal oracle vs stock torch: %.3g" % err)
    assert err < 1e-12
    # and the bidirectional stack is a different function: the tests of the feature can tell the two apart
    assert float((case["plain"] - case["causal"]).abs().max()) > 1e-3


def test_causal_oracle_with_lengths_is_stock_torch_with_both_masks(case):
    S, lengths, net = case["S"], case["lengths"], case["net"]
    valid = valid_rows(S, lengths)                                        # (S, B)
    with torch.no_grad():
        want = net.transformer_encoder(net.position_encoding(case["x"]), mask=_triu(S), src_key_padding_mask=~valid.t())
    err = float((case["both"] - want)[valid].abs().max())
    print("causal + lengths oracle vs stock torch at valid positions: %.3g" % err)
    assert err < 1e-12
    with torch.no_grad(), masked_attention(lengths):
        only_len = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    assert float((only_len - case["both"])[valid].abs().max()) > 1e-3
    # at real utterances the lengths add nothing to a causal mask over a prefix layout: query i < n sees keys j <= i < n anyway
    assert float((case["causal"] - case["both"])[valid].abs().max()) < 1e-12


def test_a_prefix_alone_equals_the_rows_of_the_full_run(case):
    S = case["S"]
    for t in sorted({0, 1, S // 2, S - 2, S - 1}):
        with torch.no_grad(), causal_attention():
            alone = O.encoder_stack(case["x"][:t + 1], case["P"], case["H"], None, n_layers=2)
        err = float((alone - case["causal"][:t + 1]).abs().max())
        assert err < 1e-12, (t, err)
        with torch.no_grad():
            bidir = O.encoder_stack(case["x"][:t + 1], case["P"], case["H"], None, n_layers=2)
        if 0 < t < S - 1:
            assert float((bidir - case["plain"][:t + 1]).abs().max()) > 1e-3, t      # the stock stack does look ahead


def test_full_lengths_add_nothing_to_the_causal_oracle(case):
    B = len(case["lengths"])
    with torch.no_grad(), causal_attention([case["S"]] * B):
        full = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    assert torch.equal(full, case["causal"])
    with torch.no_grad(), causal_attention([0] * B):
        a = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    with torch.no_grad(), causal_attention([1] * B):
        b = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    assert torch.equal(a, b)                                              # the clamp


def test_causal_is_a_plain_attribute_defaulting_to_false():
    from gan_ffn_amd import artifacts, engine
    from gan_ffn_amd import model as M

    def gens():
        return [M.AcousticGenerator(100, num_layers=1), M.VisualGenerator(100, num_layers=1), M.TextGenerator(100, num_layers=1)]
    plain, causal, both = M.GAN_FFN(*gens()), M.GAN_FFN(*gens(), causal=True), M.GAN_FFN(*gens(), mask_padding=True, causal=True)
    assert list(plain.state_dict()) == list(causal.state_dict()) == list(both.state_dict())
    assert plain.causal is False and causal.causal is True and causal.mask_padding is False
    assert both.causal is True and both.mask_padding is True
    for fn in (M.GAN_FFN.__init__, engine.Phase2Engine.__init__, artifacts.run_training, M._Net.forward):
        assert inspect.signature(fn).parameters["causal"].default is False, fn
    assert engine._NetRunner._causal is False
    # the heads of these two are bidirectional recurrences: no such option
    assert "causal" not in inspect.signature(M.GAN_FFN_DialogueRNN.__init__).parameters
    assert "causal" not in inspect.signature(engine.DrnnEngine.__init__).parameters
    assert "causal" not in inspect.signature(engine.MeldEngine.__init__).parameters
    # with lengths the module still refuses to guess them; causal alone needs no umask (it fails later, for want of a GPU)
    a, v, t = torch.zeros(3, 2, 100), torch.zeros(3, 2, 512), torch.zeros(3, 2, 100)
    with pytest.raises(ValueError, match="umask"):
        both(a, v, t)


def test_raw_calls_take_causal_and_the_flag_is_the_header_s():
    import os
    import re
    from gan_ffn_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ganffn.h")).read()
    assert int(re.search(r"#define GANFFN_ATTN_CAUSAL (\d+)u", header).group(1)) == ops.ATTN_CAUSAL == 1
    for fn in (ops.encoder_fwd_raw, ops.encoder_bwd_raw):
        assert inspect.signature(fn).parameters["causal"].default is False
    lib = _lib.load()
    for base in ("attention_fwd", "attention_bwd", "encoder_fwd", "encoder_bwd"):
        mask, ln = _lib.SIGNATURES["ganffn_%s_mask" % base][1], _lib.SIGNATURES["ganffn_%s_len" % base][1]
        assert hasattr(lib, "ganffn_%s_mask" % base)
        assert len(mask) == len(ln) + 1                                   # the _len call with one flags word ...
        at = [i for i in range(len(mask)) if mask[:i] + mask[i + 1:] == ln and mask[i] is _lib._U32]
        assert at, base
        assert "int ganffn_%s_mask(" % base in header
    assert lib.ganffn_version() == 100
