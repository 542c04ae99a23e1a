"""GPU parity of the packed-sequence LSTM (csrc/lstm.hip: ganffn_lstm_packed_layer_* / ganffn_lstm_stack_packed_*, through
ops.LstmPackedLayerFn, ops.lstm_forward(lengths=...), MELDLSTMModel(packed=True) and engine.MeldEngine(packed=True)) against the
fp64 restatement of the rule (tests/lstm_packed_oracle.py, pinned to torch's pack_padded_sequence -> nn.LSTM ->
pad_packed_sequence by tests/test_lstm_packed_cpu.py).  Tolerances are the ones the unpacked path is held to
(tests/test_hip_lstm.py, tests/test_hip_meld_engine.py); every compared distance is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import engine_oracle as EO
import lstm_packed_oracle as PO
import meld_step_oracle as MO
from oracle import ganffn_oracle as O

pytestmark = pytest.mark.gpu

NAMES = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
KEYS = NAMES + [n + "_reverse" for n in NAMES]
LAYER_CASES = [((7, 5, 8, 4), [7, 1, 4, 2, 6]),                      # the smallest legal widths; a length of 1; a full length
               ((6, 3, 600, 300), [6, 3, 1]),                        # MELD's widths
               ((5, 40, 64, 20), [i % 6 for i in range(40)])]        # crosses the 32-dialogue tile; empty dialogues
LR, L2 = 3e-4, 1e-4                                                  # train_MELD.py:111-112
SEED = 20261019


def rel(a, b):
    b = b.double().cpu()
    return float((a.double().cpu() - b).abs().max() / max(float(b.abs().max()), 1e-30))


def dist(a, ref):
    """max |a - ref| over max |ref|"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def make_lstm(In, H, L, seed, dropout=0.0):
    torch.manual_seed(seed)
    return torch.nn.LSTM(In, H, num_layers=L, bidirectional=True, dropout=dropout)


def layer_params(lstm):
    return [getattr(lstm, k) for k in KEYS]


def dev_lengths(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device="cuda")


def valid_of(lengths, S):
    return PO.valid_mask(lengths, S)                                 # (S, B, 1) bool, on the CPU


def run_layer(x, gy, params, lengths=None):
    """one layer on the GPU, forward and backward -> (y, dx, [parameter gradients]); lengths None: the unpacked entry points"""
    from gan_ffn_amd import ops
    pc = [p.detach().cuda().requires_grad_(True) for p in params]
    xc = x.cuda().requires_grad_(True)
    y = ops.LstmLayerFn.apply(xc, *pc) if lengths is None else ops.LstmPackedLayerFn.apply(xc, dev_lengths(lengths), *pc)
    (y * gy.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xc.grad, [t.grad for t in pc]


# ------------------------------------------------------------------------------------------------------------------
# 1. one packed layer against the oracle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lengths", LAYER_CASES)
def test_packed_layer_forward_and_backward_match_the_oracle(shape, lengths):
    """output 2e-6, dx 2e-5, parameter gradients 3e-5 (tests/test_hip_lstm.py's bounds for the unpacked layer); outputs and dx
    at padded positions exactly 0.  The upstream gradient is random at padded positions too."""
    S, B, In, H = shape
    lstm = make_lstm(In, H, 1, seed=S * 7 + B)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(S, B, In, generator=g)
    gy = torch.randn(S, B, 2 * H, generator=g)
    P = {k: p.detach().double().requires_grad_(True) for k, p in lstm.named_parameters()}
    xo = x.double().requires_grad_(True)
    yo = PO.lstm_forward(xo, lengths, P, 1)
    (yo * gy.double()).sum().backward()
    y, dx, grads = run_layer(x, gy, layer_params(lstm), lengths)
    r = [rel(y, yo.detach()), rel(dx, xo.grad)] + [rel(t, P[k].grad) for k, t in zip(KEYS, grads)]
    print("packed layer %s: out %.1e dx %.1e worst parameter gradient %.1e" % (shape, r[0], r[1], max(r[2:])))
    assert r[0] < 2e-6
    assert r[1] < 2e-5
    for k, v in zip(KEYS, r[2:]):
        assert v < 3e-5, k
    pad = ~valid_of(lengths, S)
    assert int(pad.sum()) > 0
    assert float(y.cpu()[pad.expand_as(y)].abs().max()) == 0.0
    assert float(dx.cpu()[pad.expand_as(dx)].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------
# 2. full lengths: the unpacked entry points' bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 5, 8, 4), (5, 40, 64, 20)])
def test_full_lengths_give_the_bits_of_the_unpacked_entry_points(shape):
    S, B, In, H = shape
    lstm = make_lstm(In, H, 1, seed=S + B)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(S, B, In, generator=g)
    gy = torch.randn(S, B, 2 * H, generator=g)
    y0, dx0, g0 = run_layer(x, gy, layer_params(lstm))
    for lengths in ([S] * B, [S + 3] * B):                           # (a length above S counts as S)
        y1, dx1, g1 = run_layer(x, gy, layer_params(lstm), lengths)
        assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
        for k, a, b in zip(KEYS, g1, g0):
            assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------------------------
# 3. select, not multiply: what x and d_out hold at padded positions does not matter
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lengths", [LAYER_CASES[0], LAYER_CASES[2]])
def test_values_at_padded_positions_change_no_bit(shape, lengths):
    S, B, In, H = shape
    lstm = make_lstm(In, H, 1, seed=S + 2 * B)
    g = torch.Generator().manual_seed(6)
    valid = valid_of(lengths, S)
    x = torch.randn(S, B, In, generator=g) * valid
    gy = torch.randn(S, B, 2 * H, generator=g) * valid
    xj = torch.where(valid, x, 1e3 * torch.randn(S, B, In, generator=g))
    gyj = torch.where(valid, gy, 1e3 * torch.randn(S, B, 2 * H, generator=g))
    assert float(xj[~valid.expand_as(x)].abs().max()) > 1e3
    y0, dx0, g0 = run_layer(x, gy, layer_params(lstm), lengths)
    y1, dx1, g1 = run_layer(xj, gyj, layer_params(lstm), lengths)
    assert torch.equal(y1, y0)
    assert torch.equal(dx1, dx0)
    for k, a, b in zip(KEYS, g1, g0):
        assert torch.equal(a, b), k
    assert float(g0[0].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------
# 4. the four-layer stack in train mode, the Philox stream shared with the oracle
# ------------------------------------------------------------------------------------------------------------------
def test_four_layer_packed_stack_in_train_mode_matches_the_oracle_with_the_same_masks():
    """(9, 6, 16, 8), lengths [9, 1, 5, 2, 9, 3], p = 0.5: output 1e-5, dx 1e-4, parameter gradients 2e-4
    (test_four_layer_stack_matches_oracle_with_the_same_dropout_masks' bounds); the same call twice gives the same bits, and
    ganffn_lstm_stack_packed_fwd / _bwd give the bits of the per-layer chain ops.lstm_forward issues."""
    from gan_ffn_amd import _lib, ops
    S, B, In, H, L, p = 9, 6, 16, 8, 4, 0.5
    lengths = [9, 1, 5, 2, 9, 3]
    lstm = make_lstm(In, H, L, seed=11, dropout=p)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(S, B, In, generator=g) * 0.5
    gy = torch.randn(S, B, 2 * H, generator=g)
    seed = 424242
    P = {k: v.detach().double().requires_grad_(True) for k, v in lstm.named_parameters()}
    xo = x.double().requires_grad_(True)
    yo = PO.lstm_forward(xo, lengths, P, L, p, rng=O.Rng(seed, 0, True))
    (yo * gy.double()).sum().backward()
    m = lstm.cuda().train()
    ln = dev_lengths(lengths)

    def run():
        ops.manual_seed(seed)
        m.zero_grad()
        xc = x.cuda().requires_grad_(True)
        y = ops.lstm_forward(xc, m, True, lengths=ln)
        (y * gy.cuda()).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), xc.grad, {k: v.grad.clone() for k, v in m.named_parameters()}

    y, dx, G = run()
    r = [rel(y, yo.detach()), rel(dx, xo.grad)] + [rel(G[k], P[k].grad) for k in G]
    print("packed stack, train: out %.1e dx %.1e worst parameter gradient %.1e" % (r[0], r[1], max(r[2:])))
    assert r[0] < 1e-5
    assert r[1] < 1e-4
    for k, v in zip(G, r[2:]):
        assert v < 2e-4, k
    pad = ~valid_of(lengths, S)
    assert float(y.cpu()[pad.expand_as(y)].abs().max()) == 0.0 and float(dx.cpu()[pad.expand_as(dx)].abs().max()) == 0.0
    y2, dx2, G2 = run()
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    for k in G:
        assert torch.equal(G2[k], G[k]), k
    # dropout really happened
    with torch.no_grad():
        assert not torch.equal(ops.lstm_forward(x.cuda(), m, False, lengths=ln), y)
    # the stack entry points: the same launches in one call
    names = [k for k, _ in m.named_parameters()]
    Pd = {k: v.detach() for k, v in m.named_parameters()}
    Gs = {k: torch.zeros_like(v) for k, v in Pd.items()}
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    col = lambda j, src: [src[names[4 * i + j]] for i in range(2 * L)]
    cfg = _lib.LstmStackCfg(S, B, In, H, L, p, 1)
    n_saved, n_ws = ops.lstm_sizes(cfg, packed=True)            # (the _batch_ size functions)
    assert n_saved > 0 and n_ws > 0
    saved, ws = torch.empty(n_saved, device="cuda"), torch.empty(n_ws, device="cuda")
    out_s, dx_s = torch.empty(S, B, 2 * H, device="cuda"), torch.empty(S, B, In, device="cuda")
    xd, dy = x.cuda(), gy.cuda()
    ops.manual_seed(seed)
    rng = ops.DeviceRng.get(xd.device)
    # lengths given: ganffn_lstm_stack_packed_fwd / _bwd
    weights = [arr(col(j, Pd)) for j in range(4)]
    ops.lstm_stack_fwd_raw(cfg, xd, *weights, out_s, saved, ws, rng.state, 0, lengths=ln)
    ops.lstm_stack_bwd_raw(cfg, dy, xd, out_s, *weights[:2], dx_s, *[arr(col(j, Gs)) for j in range(4)], saved, ws, rng.state, 0, lengths=ln)
    torch.cuda.synchronize()
    assert torch.equal(out_s, y) and torch.equal(dx_s, dx)
    for k in names:
        assert torch.equal(Gs[k], G[k]), k


# ------------------------------------------------------------------------------------------------------------------
# 5. the module path against its own CPU self (torch's packing)
# ------------------------------------------------------------------------------------------------------------------
def test_packed_module_on_the_gpu_matches_its_cpu_self():
    """MELDLSTMModel(16, 8, 16, packed=True), eval mode: log_prob at valid positions 1e-5, every parameter gradient 2e-4 (the
    stack bounds)"""
    import copy
    from gan_ffn_amd.dialogue_rnn import MELDLSTMModel
    torch.manual_seed(21)
    cpu = MELDLSTMModel(16, 8, 16, packed=True).eval()
    gpu = copy.deepcopy(cpu).cuda().eval()
    assert gpu.packed is True
    S, lengths = 7, [7, 2, 1, 5, 3]
    g = torch.Generator().manual_seed(2)
    valid = valid_of(lengths, S)
    U = torch.randn(S, len(lengths), 16, generator=g) * valid
    umask = valid[:, :, 0].t().float().contiguous()
    gy = torch.randn(S, len(lengths), 7, generator=g) * valid
    lp_c = cpu(U, None, umask)[0]
    (lp_c * gy).sum().backward()
    lp_g = gpu(U.cuda(), None, umask.cuda())[0]
    (lp_g * gy.cuda()).sum().backward()
    torch.cuda.synchronize()
    sel = valid.expand_as(lp_c)
    r = rel(lp_g.detach().cpu()[sel], lp_c.detach()[sel])
    print("packed module: log_prob %.1e" % r)
    assert r < 1e-5
    pg = dict(gpu.named_parameters())
    n = 0
    for k, v in cpu.named_parameters():
        if v.grad is None:
            assert pg[k].grad is None, k
            continue
        d = rel(pg[k].grad, v.grad)
        assert d < 2e-4, (k, d)
        n += 1
    assert n == 36


# ------------------------------------------------------------------------------------------------------------------
# 6. the engine against the fp64 step oracle with the packed LSTM swapped in
# ------------------------------------------------------------------------------------------------------------------
def packed_oracle_step(P, text, umask, label, p_drop=0.0, seed=0, offsets=None, train=False):
    """tests/meld_step_oracle.py's forward and step with PO.lstm_forward(lengths = umask.sum(1)) in LO.lstm_forward's place"""
    from gan_ffn_amd.dialogue_rnn import general2_scores
    names = MO.trained_names()
    Pd = {k: torch.as_tensor(np.asarray(v, np.float64)).clone().requires_grad_(k in set(names)) for k, v in P.items()}
    t = torch.as_tensor(np.asarray(text, np.float64))
    um, lab = torch.as_tensor(np.asarray(umask, np.float64)), torch.as_tensor(np.asarray(label, np.int64))
    rng = O.Rng(seed, offsets[0] if offsets else 0, train)
    em = PO.lstm_forward(t, um.sum(1).long(), Pd, MO.N_LAYERS, p_drop, rng, prefix="lstm.", offsets=offsets)
    xq = em @ Pd["matchatt.transform.weight"].T + Pd["matchatt.transform.bias"]
    alpha = general2_scores(xq.transpose(0, 1), em, um)
    att = torch.bmm(alpha, em.transpose(0, 1)).transpose(0, 1)
    hidden = MO.hardswish(em + MO.hardswish(att))
    log_prob = torch.log_softmax(hidden @ Pd["smax_fc.weight"].T + Pd["smax_fc.bias"], 2)
    lp = log_prob.transpose(0, 1).reshape(-1, log_prob.shape[2])
    y, m = lab.reshape(-1), um.reshape(-1)
    loss = -(m * lp.gather(1, y.unsqueeze(1))[:, 0]).sum() / m.sum()
    grads = torch.autograd.grad(loss, [Pd[k] for k in names])
    return dict(loss=float(loss.detach()), log_prob=log_prob.detach().numpy(), alpha=alpha.detach().numpy(),
                grads={k: g_.numpy() for k, g_ in zip(names, grads)})


def meld_net(seed, dropout=0.6, packed=True):
    from gan_ffn_amd.dialogue_rnn import MELDLSTMModel
    torch.manual_seed(seed)
    return MELDLSTMModel(600, 300, 600, n_classes=7, dropout=dropout, packed=packed).cuda().train()


def meld_batch(S, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    valid = valid_of(lengths, S)
    text = ((torch.rand(S, B, 600, generator=g) - 0.5) * valid).contiguous()
    umask = valid[:, :, 0].t().float().contiguous()
    label = torch.randint(0, 7, (B, S), generator=g) * umask.long()
    return {"text": text.cuda(), "umask": umask.cuda(), "label": label.cuda()}


def engine_named(eng):
    names = {id(p): k for k, p in eng.module.named_parameters()}
    return [names[id(p)] for p in eng._params]


@pytest.mark.parametrize("S,lengths,max_dialogues", [(6, [6, 2, 1, 4], 32), (5, [1 + i % 5 for i in range(40)], 64)])
def test_packed_engine_step_matches_the_fp64_step_oracle(S, lengths, max_dialogues):
    """one train step at dropout 0.6 with the engine's own Philox masks, then an eval step: log_prob, the loss and every gradient
    element at 1e-3 of the tensor's scale, Adam elementwise as tests/test_hip_classifier_engines_train_oracle._check_adam bounds
    it (tests/test_hip_meld_engine.py's train-oracle test); (5, 40): above the 32-dialogue tile, max_dialogues = 64"""
    import test_hip_classifier_engines_train_oracle as TO
    from gan_ffn_amd import engine as E, ops
    net = meld_net(7)
    b = meld_batch(S, lengths, seed=9)
    ops.manual_seed(SEED)
    eng = E.MeldEngine(net, lr=LR, weight_decay=L2, max_dialogues=max_dialogues, packed=True)
    assert eng.packed is True
    names = engine_named(eng)
    assert names == MO.trained_names()
    sl = TO._Slab("meld", eng.slab, eng.grad, eng.exp_avg, eng.exp_avg_sq, eng.step_count, LR, L2,
                  [(o, p.numel()) for o, p in zip(eng._offs, eng._params)])
    text, umask, label = b["text"].cpu().numpy(), b["umask"].cpu().numpy(), b["label"].cpu().numpy()
    pre = sl.host()
    P = {k: eng._p(j).view_as(eng._params[j]).detach().cpu().numpy().copy() for j, k in enumerate(names)}
    loss, lp = eng.step(b, train=True)
    torch.cuda.synchronize()
    post = sl.host(grad=True)
    offsets = [eng._base_add + l for l in range(eng.L - 1)]
    seed = int(ops.DeviceRng.get(eng.dev).state.cpu()[0])
    o = packed_oracle_step(P, text, umask, label, 0.6, seed=seed, offsets=offsets, train=True)
    d_lp, d_loss = dist(lp.cpu().numpy(), o["log_prob"]), abs(float(loss) - o["loss"]) / abs(o["loss"])
    print("packed engine (%d, %d) train: log_prob %.2e loss %.2e alpha %.2e" % (S, len(lengths), d_lp, d_loss, dist(eng.alpha.cpu().numpy(), o["alpha"])))
    assert d_lp <= 1e-3 and d_loss <= 1e-3
    worst = (0.0, "")
    for j, k in enumerate(names):
        d = dist(eng._p(j, True).view_as(eng._params[j]).detach().cpu().numpy(), o["grads"][k])
        worst = max(worst, (d, k))
        assert d <= 1e-3, (k, d)
    print("packed engine (%d, %d) train: worst gradient element %.2e of scale (%s)" % (S, len(lengths), *worst))
    TO._check_adam(sl, pre, post, "packed meld step")
    # eval step: no dropout, nothing moves
    state = [t.clone() for t in (eng.slab, eng.exp_avg, eng.exp_avg_sq, eng.step_count)]
    P1 = {k: eng._p(j).view_as(eng._params[j]).detach().cpu().numpy().copy() for j, k in enumerate(names)}
    loss_e, lp_e = eng.step(b, train=False)
    torch.cuda.synchronize()
    oe = packed_oracle_step(P1, text, umask, label, 0.6, train=False)
    d_lp, d_loss = dist(lp_e.cpu().numpy(), oe["log_prob"]), abs(float(loss_e) - oe["loss"]) / abs(oe["loss"])
    print("packed engine (%d, %d) eval: log_prob %.2e loss %.2e" % (S, len(lengths), d_lp, d_loss))
    assert d_lp <= 1e-3 and d_loss <= 1e-3
    for t0, t1 in zip(state, (eng.slab, eng.exp_avg, eng.exp_avg_sq, eng.step_count)):
        assert torch.equal(t0, t1)
    # the padded step's oracle on the same weights would not pass the bound above: the comparison tells the two apart
    o_pad = MO.step(P1, text, umask, label, 0.0, train=False)
    assert dist(oe["log_prob"], o_pad["log_prob"]) > 1e-3


# ------------------------------------------------------------------------------------------------------------------
# 7. what the feature exists for: a dialogue's prediction does not depend on its batch
# ------------------------------------------------------------------------------------------------------------------
def test_a_dialogue_in_a_padded_batch_is_predicted_as_if_alone():
    """eval mode, S = 5, lengths [5, 2, 1]: log_prob of each dialogue inside the batch equals, at its valid positions, that of the
    dialogue alone at (len, 1), at the engine-versus-oracle bound (1e-3 of the scale)"""
    from gan_ffn_amd import engine as E
    S, lengths = 5, [5, 2, 1]
    b = meld_batch(S, lengths, seed=12)
    eng = E.MeldEngine(meld_net(13), packed=True)
    _, lp = eng.step(b, train=False)
    lp = lp.detach().cpu().numpy().copy()
    eng_pad = E.MeldEngine(meld_net(13, packed=False))
    lp_pad = eng_pad.step(b, train=False)[1].detach().cpu().numpy().copy()
    for i, n in enumerate(lengths):
        one = {"text": b["text"][:n, i:i + 1].contiguous(), "umask": b["umask"][i:i + 1, :n].contiguous(),
               "label": b["label"][i:i + 1, :n].contiguous()}
        alone = eng.step(one, train=False)[1].detach().cpu().numpy().copy()
        d, d_pad = dist(lp[:n, i:i + 1], alone), dist(lp_pad[:n, i:i + 1], alone)
        print("dialogue %d (%d of %d steps): in the batch against alone %.2e (the padded step: %.2e)" % (i, n, S, d, d_pad))
        assert d <= 1e-3, (i, d)
