"""Key-length attention on the CPU: the masked restatement of the oracle (tests/key_len_oracle.py) against stock torch's
src_key_padding_mask, the property the feature exists for (a dialogue in a padded batch is computed as if alone), and the
`mask_padding` switch of the two IEMOCAP classifier modules."""
import pytest
import torch

from oracle import ganffn_oracle as O
from oracle import stock_modules as SM
from key_len_oracle import masked_attention, valid_rows

CASES = [("AcousticGenerator", 17, [17, 16, 1, 5]), ("VisualGenerator", 9, [9, 2, 1])]


def _stack(name, S, lengths, seed=5):
    torch.manual_seed(seed)
    net = SM.StockNet(name, 100, 0.2, num_layers=2).double().eval()
    E = net.position_encoding.pe.shape[2]
    P = {k: v.detach() for k, v in net.state_dict().items()}
    x = torch.rand(S, len(lengths), E, dtype=torch.float64)
    H = net.encoder_layer.self_attn.num_heads
    return net, P, H, x


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    name, S, lengths = request.param
    net, P, H, x = _stack(name, S, lengths)
    with torch.no_grad(), masked_attention(lengths):
        masked = O.encoder_stack(x, P, H, None, n_layers=2)
    with torch.no_grad():
        plain = O.encoder_stack(x, P, H, None, n_layers=2)
    return dict(net=net, P=P, H=H, x=x, S=S, lengths=lengths, masked=masked, plain=plain)


def test_masked_oracle_is_stock_torch_with_src_key_padding_mask(case):
    S, lengths, net = case["S"], case["lengths"], case["net"]
    valid = valid_rows(S, lengths)                                        # (S, B)
    with torch.no_grad():
        want = net.transformer_encoder(net.position_encoding(case["x"]), src_key_padding_mask=~valid.t())
    err = float((case["masked"] - want)[valid].abs().max())
    print("masked oracle vs stock torch at valid positions: %.3g" % err)
    assert err < 1e-12
    # and the unmasked stack is a different function: the tests of the feature can tell the two apart
    assert float((case["plain"] - case["masked"])[valid].abs().max()) > 1e-3


def test_a_dialogue_alone_equals_its_rows_in_the_batch(case):
    for b, n in enumerate(case["lengths"]):
        with torch.no_grad(), masked_attention([n]):
            alone = O.encoder_stack(case["x"][:n, b:b + 1], case["P"], case["H"], None, n_layers=2)
        err = float((alone[:, 0] - case["masked"][:n, b]).abs().max())
        assert err < 1e-12, (b, n, err)


def test_full_lengths_equal_the_unmasked_oracle_exactly(case):
    B = len(case["lengths"])
    with torch.no_grad(), masked_attention([case["S"]] * B):
        full = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    assert torch.equal(full, case["plain"])


def test_out_of_range_lengths_are_clamped(case):
    S, B = case["S"], len(case["lengths"])
    with torch.no_grad(), masked_attention([0] * B):
        a = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    with torch.no_grad(), masked_attention([1] * B):
        b = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    assert torch.equal(a, b)
    with torch.no_grad(), masked_attention([S + 5] * B):
        c = O.encoder_stack(case["x"], case["P"], case["H"], None, n_layers=2)
    assert torch.equal(c, case["plain"])


def test_mask_padding_is_a_plain_attribute_and_needs_umask():
    """the switch adds no parameter or buffer (the state_dict is the reference's), and a masked forward refuses to guess lengths"""
    from gan_ffn_amd import model as M

    def gens():
        return [M.AcousticGenerator(100, num_layers=1), M.VisualGenerator(100, num_layers=1), M.TextGenerator(100, num_layers=1)]
    dims = dict(D_m=100, D_g=20, D_p=20, D_e=12, D_h=12, D_a=12, n_classes=6, listener_state=False,
                context_attention="general", dropout_rec=0.1, dropout=0.5)
    plain, masked = M.GAN_FFN(*gens()), M.GAN_FFN(*gens(), mask_padding=True)
    assert list(plain.state_dict()) == list(masked.state_dict())
    assert masked.mask_padding is True and plain.mask_padding is False
    d_plain, d_masked = M.GAN_FFN_DialogueRNN(*gens(), **dims), M.GAN_FFN_DialogueRNN(*gens(), **dims, mask_padding=True)
    assert list(d_plain.state_dict()) == list(d_masked.state_dict())
    assert d_masked.mask_padding is True and d_plain.mask_padding is False
    a, v, t = torch.zeros(3, 2, 100), torch.zeros(3, 2, 512), torch.zeros(3, 2, 100)
    with pytest.raises(ValueError, match="umask"):
        masked(a, v, t)
    with pytest.raises(ValueError, match="umask"):
        masked(a, v, t, umask=None)
    with pytest.raises(ValueError, match="umask"):
        d_masked(a, v, t, torch.zeros(3, 2, 2), None)


def test_lengths_come_from_one_helper_and_the_prefix_check_catches_holes():
    from gan_ffn_amd import ops
    um = torch.tensor([[1., 1., 1., 0.], [1., 0., 0., 0.], [1., 1., 1., 1.]])
    kl = ops.key_lengths_from_umask(um)
    assert kl.dtype == torch.int32 and kl.tolist() == [3, 1, 4]
    ops.check_prefix_mask(um, "test")
    holes = um.clone()
    holes[0, 1] = 0.0
    with pytest.raises(ValueError, match="prefixes"):
        ops.check_prefix_mask(holes, "test")
