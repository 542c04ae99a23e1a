"""GPU parity of the one-direction LSTM (csrc/lstm.hip with a direction count of 1; ganffn_unilstm_*, ops.UniLstmLayerFn) against
the fp64 restatement (tests/meld_causal_oracle.py, pinned to torch.nn.LSTM(bidirectional=False) by tests/test_meld_causal_cpu.py):
one layer forward and backward, padded and with lengths, at the bounds of tests/test_hip_lstm.py; the packed rule's exact zeros
and its indifference to padded positions; the output bit for bit the forward half of the two-direction layer's; the stack call
bit for bit the per-layer chain; determinism.  Every compared distance is printed before it is asserted."""
import ctypes as C

import pytest
import torch

import meld_causal_oracle as CO
from oracle import ganffn_oracle as O

pytestmark = pytest.mark.gpu

# (1, 1, 4, 4): S = 1, no recurrent product; (5, 40, 64, 20): crosses the 32-dialogue tile; (6, 3, 600, 300): MELD's widths
SHAPES = [(1, 1, 4, 4), (7, 5, 8, 4), (5, 40, 64, 20), (6, 3, 600, 300)]
NAMES = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]


def rel(a, b):
    b = b.double()
    return float((a.double().cpu() - b).abs().max() / max(float(b.abs().max()), 1e-30))


def lengths_of(S, B):
    """real steps per dialogue: a full one, a length of 1 and (B > 2) a length of 0 among them"""
    if B == 1:
        return [S]
    return [(S, 1, 0, S // 2 + 1, S - 1)[b % 5] for b in range(B)]


def case(S, B, In, H):
    torch.manual_seed(S * 7 + B)
    bi = torch.nn.LSTM(In, H, num_layers=1, bidirectional=True)
    g = torch.Generator().manual_seed(3)
    return bi, torch.randn(S, B, In, generator=g), torch.randn(S, B, H, generator=g)


def run_uni(params, x, gy, lengths):
    from gan_ffn_amd import ops
    pc = [p.detach().cuda().requires_grad_(True) for p in params]
    xc = x.cuda().requires_grad_(True)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    y = ops.UniLstmLayerFn.apply(xc, ln, *pc)
    (y * gy.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xc.grad, [p.grad for p in pc]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("S,B,In,H", SHAPES)
def test_one_forward_only_layer_forward_and_backward(S, B, In, H, packed):
    from gan_ffn_amd import ops
    bi, x, gy = case(S, B, In, H)
    params = [getattr(bi, n) for n in NAMES]
    lengths = lengths_of(S, B) if packed else None
    # oracle, float64
    P = {n: p.detach().double().requires_grad_(True) for n, p in zip(NAMES, params)}
    xo = x.double().requires_grad_(True)
    yo = CO.lstm_layer(xo, P, 0, lengths)
    (yo * gy.double()).sum().backward()
    y, dx, grads = run_uni(params, x, gy, lengths)
    d = [rel(y, yo.detach()), rel(dx, xo.grad)] + [rel(g_, P[n].grad) for n, g_ in zip(NAMES, grads)]
    print("unilstm (%d, %d, %d, %d) packed=%s: out %.2e dx %.2e w_ih %.2e w_hh %.2e b_ih %.2e b_hh %.2e" % (S, B, In, H, packed, *d))
    assert d[0] < 2e-6
    assert d[1] < 2e-5
    for n, v in zip(NAMES, d[2:]):
        assert v < 3e-5, n
    # deterministic: the same call again gives the same bits (no atomics anywhere)
    y2, dx2, grads2 = run_uni(params, x, gy, lengths)
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)
    # bit for bit the forward half of the two-direction layer with the same forward-direction weights: the same products, one
    # problem per skinny launch instead of two
    allp = [p.detach().cuda() for p in params] + [getattr(bi, n + "_reverse").detach().cuda() for n in NAMES]
    with torch.no_grad():
        if packed:
            yb = ops.LstmPackedLayerFn.apply(x.cuda(), torch.tensor(lengths, dtype=torch.int32, device="cuda"), *allp)
        else:
            yb = ops.LstmLayerFn.apply(x.cuda(), *allp)
    assert yb.shape == (S, B, 2 * H) and torch.equal(yb[:, :, :H], y)
    if packed:
        pad = ~torch.arange(S).unsqueeze(1).lt(torch.tensor(lengths).unsqueeze(0))               # (S, B): t >= lengths[b]
        if bool(pad.any()):
            assert float(y.cpu()[pad].abs().max()) == 0.0 and float(dx.cpu()[pad].abs().max()) == 0.0
            # values of x and d_out at padded positions change no bit
            x2, gy2 = x.clone(), gy.clone()
            x2[pad] = torch.randn(int(pad.sum()), In, generator=torch.Generator().manual_seed(8)) * 50.0
            gy2[pad] = torch.randn(int(pad.sum()), H, generator=torch.Generator().manual_seed(9)) * 1e3
            y3, dx3, grads3 = run_uni(params, x2, gy2, lengths)
            assert torch.equal(y3, y) and torch.equal(dx3, dx)
            for a, b in zip(grads, grads3):
                assert torch.equal(a, b)


def test_more_dialogues_than_one_call_takes_run_in_chunks():
    """B = 260 > MAX_DIALOGUES: two native calls, lengths sliced alongside; every dialogue has the bits it has in a call of its own tile"""
    from gan_ffn_amd import ops
    S, B, In, H = 3, 260, 8, 4
    bi, x, gy = case(S, B, In, H)
    params = [getattr(bi, n) for n in NAMES]
    lengths = lengths_of(S, B)
    y, dx, grads = run_uni(params, x, gy, lengths)
    ya, dxa, ga = run_uni(params, x[:, :256].contiguous(), gy[:, :256].contiguous(), lengths[:256])
    yb, dxb, gb = run_uni(params, x[:, 256:].contiguous(), gy[:, 256:].contiguous(), lengths[256:])
    assert torch.equal(y, torch.cat((ya, yb), 1)) and torch.equal(dx, torch.cat((dxa, dxb), 1))
    P = {n: p.detach().double().requires_grad_(True) for n, p in zip(NAMES, params)}
    yo = CO.lstm_layer(x.double(), P, 0, lengths)
    (yo * gy.double()).sum().backward()
    for n, g_ in zip(NAMES, grads):
        assert rel(g_, P[n].grad) < 3e-5, n


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("train", [False, True])
def test_stack_call_gives_the_bits_of_the_per_layer_chain(train, packed):
    """ganffn_unilstm_stack_fwd / _bwd against the chain ops.lstm_forward issues for a unidirectional nn.LSTM (ganffn_unilstm_layer_*
    + ganffn_dropout per layer), same {seed, offsets}: torch.equal on the output, the input gradient and all 12 parameter
    gradients; the chain itself against the fp64 oracle with the same Philox masks (site 64 + l, width H) at the bounds
    tests/test_hip_lstm.py holds the two-direction stack to; two runs with the same seed give the same bits."""
    from gan_ffn_amd import _lib, ops
    S, B, In, H, L, p = 5, 3, 12, 8, 3, 0.5
    seed = 20261021
    torch.manual_seed(4)
    lstm = torch.nn.LSTM(In, H, num_layers=L, bidirectional=False, dropout=p).cuda().train(train)
    g = torch.Generator().manual_seed(6)
    x0, dy = torch.randn(S, B, In, generator=g), torch.randn(S, B, H, generator=g).cuda()
    lengths = [5, 1, 3] if packed else None
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")

    def chain():
        lstm.zero_grad()
        ops.manual_seed(seed)
        rng = ops.DeviceRng.get("cuda")
        rng.next_add(5)
        base = rng.counter
        x = x0.cuda().requires_grad_(True)
        out = ops.lstm_forward(x, lstm, train, lengths=ln)
        assert rng.counter == base + (L - 1 if train else 0)          # one offset per active dropout call
        out.backward(dy)
        torch.cuda.synchronize()
        return base, out.detach(), x.grad, {k: v.grad.clone() for k, v in lstm.named_parameters()}

    base, out_c, dx_c, g_c = chain()
    base2, out_c2, dx_c2, g_c2 = chain()
    assert base2 == base and torch.equal(out_c2, out_c) and torch.equal(dx_c2, dx_c) and all(torch.equal(g_c[k], g_c2[k]) for k in g_c)
    # the oracle with the same masks
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in lstm.named_parameters()}
    xo = x0.double().requires_grad_(True)
    yo = CO.lstm_forward(xo, P, L, p, rng=O.Rng(seed, base, train), lengths=lengths)
    (yo * dy.cpu().double()).sum().backward()
    d = [rel(out_c, yo.detach()), rel(dx_c, xo.grad), max(rel(g_c[k], P[k].grad) for k in P)]
    print("unilstm stack train=%s packed=%s: out %.2e dx %.2e worst gradient %.2e" % (train, packed, *d))
    assert d[0] < 1e-5 and d[1] < 1e-4 and d[2] < 2e-4
    if train:
        assert not torch.equal(out_c, ops.lstm_forward(x0.cuda(), lstm.eval(), False, lengths=ln).detach())     # dropout happened
        lstm.train()
    # the stack call
    names = [k for k, _ in lstm.named_parameters()]
    assert names == ["%s_l%d" % (k, l) for l in range(L) for k in CO.LSTM_KEYS]
    Pd = {k: v.detach() for k, v in lstm.named_parameters()}
    G = {k: torch.zeros_like(v) for k, v in Pd.items()}
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    col = lambda j, src: [src[names[4 * i + j]] for i in range(L)]                 # [L][1]
    cfg = _lib.LstmStackCfg(S, B, In, H, L, p, 1 if train else 0)
    n_saved, n_ws = ops.unilstm_sizes(cfg)
    saved, ws = torch.empty(n_saved, device="cuda"), torch.empty(n_ws, device="cuda")
    out_s, dx_s = torch.empty(S, B, H, device="cuda"), torch.empty(S, B, In, device="cuda")
    xd = x0.cuda()
    weights = [arr(col(j, Pd)) for j in range(4)]
    rng = ops.DeviceRng.get("cuda")
    ops.unilstm_stack_fwd_raw(cfg, xd, *weights, out_s, saved, ws, rng.state if train else None, base, lengths=ln)
    ops.unilstm_stack_bwd_raw(cfg, dy, xd, out_s, *weights[:2], dx_s, *[arr(col(j, G)) for j in range(4)], saved, ws,
                              rng.state if train else None, base, lengths=ln)
    torch.cuda.synchronize()
    assert torch.equal(out_s, out_c)
    assert torch.equal(dx_s, dx_c)
    for k in names:
        assert torch.equal(G[k], g_c[k]), k
