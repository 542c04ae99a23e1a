"""engine.MeldEngine — the MELD classifier's train / eval step on the C ABI (the counterpart of train_MELD.py:50-104,147-157) —
on the device, against
  1. the REFERENCE-made fixture tests/golden/meld_step.npz (4 Adam steps on one batch; tests/test_meld_step_cpu.py pins it to the
     mirror and to the fp64 oracle),
  2. the module path (MELDLSTMModel under autograd) on the same weights, and the per-layer LSTM chain bit for bit,
  3. the fp64 restatement of the step (tests/meld_step_oracle.py) in TRAIN mode at the script's dropout 0.6, with the engine's
     own Philox masks, and fp64 Adam,
  4.-7. what the step must leave alone, determinism, buffer reuse, limits, the epoch loop.
Bounds are stated where they are used; every compared distance is printed before it is asserted."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import formula as F_
import make_golden_meld_step as MG
from util import golden

pytestmark = pytest.mark.gpu

LR, L2 = 3e-4, 1e-4                      # train_MELD.py:111-112
SEED = 20261016


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def dist(a, ref):
    """max |a - ref| over max |ref|"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def mirror(C_, dropout=0.0, formula=True, seed=2, dims=(600, 300, 600)):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    m = DR.MELDLSTMModel(*dims, n_classes=C_, dropout=dropout)
    if formula:
        sd = F_.formula_state_dict(m.state_dict())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda().train()


def fixture_batch(S, B, C_):
    U, umask, label = MG.case_inputs(S, B, C_)
    return {"text": torch.from_numpy(U).cuda(), "umask": torch.from_numpy(umask).cuda(), "label": torch.from_numpy(label).cuda()}


def random_batch(S, B, C_, seed=5):
    from gan_ffn_amd import data as D
    b = D.synthetic_batch(B=B, S_max=S, seed=seed, device="cuda", n_classes=C_, dims={"text": 600}, lo=2, mean=max(3, S // 2))
    b["text"] = (b["text"] - 0.5 * b["umask"].t().unsqueeze(-1)).contiguous()
    return b


def module_step(m, b, opt=None):
    """train_MELD.py:63-87 on the module path; -> (loss, log_prob, alpha (B, S, S))"""
    from gan_ffn_amd import model as M
    if opt is not None:
        opt.zero_grad()
    lp, alpha, _, _ = m(b["text"], None, b["umask"])
    loss = M.MaskedNLLLoss()(lp.transpose(0, 1).contiguous().view(-1, lp.shape[2]), b["label"].view(-1), b["umask"])
    if m.training:
        loss.backward()
        if opt is not None:
            opt.step()
    return loss.detach(), lp.detach(), torch.stack(alpha, 1).detach()


def engine_named(eng):
    names = {id(p): k for k, p in eng.module.named_parameters()}
    return [names[id(p)] for p in eng._params]


def engine_grads(eng):
    return {k: eng._p(i, True).view_as(eng._params[i]).detach().cpu().numpy().copy() for i, k in enumerate(engine_named(eng))}


# ------------------------------------------------------------------------------------------------------------------
# 1. the reference-made fixture
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(MG.CASES))
def test_engine_reproduces_the_reference_fixture(tag):
    """Step 0: log_prob and alpha 5e-5, sampled gradients 5e-4 of scale (the bounds tests/test_dialogue_rnn_cpu.check_meld holds the
    module path to).  Steps 1-3 and the final parameters: no bound can be derived for a chained Adam trajectory, so the module path
    on this GPU (autograd + torch.optim.Adam) is measured against the fixture too, and the engine's distance must be at most twice
    the module path's or the step-0 bound, whichever is larger.  (The loss is a mean of log_prob entries: its step-0 bound is
    log_prob's.  A parameter has no step-0 bound of its own: an Adam update is at most ~lr whatever the gradient, and a gradient
    known to 5e-4 of its tensor's scale may have either sign where it is smaller than that — 2 lr per step, 2 lr N_STEPS in all.)"""
    from gan_ffn_amd import engine as E
    g = golden("meld_step")
    S, B, C_ = MG.CASES[tag]
    b = fixture_batch(S, B, C_)
    m_e, m_m = mirror(C_), mirror(C_)
    eng = E.MeldEngine(m_e, lr=LR, weight_decay=L2)
    opt = torch.optim.Adam(m_m.parameters(), lr=LR, weight_decay=L2)
    lp_scale = float(np.abs(g[tag + "/log_prob"]).max())
    for i in range(MG.N_STEPS):
        loss_e, lp_e = eng.step(b, train=True)
        loss_e, lp_e, alpha_e = float(loss_e), lp_e.cpu().numpy().copy(), eng.alpha.cpu().numpy().copy()
        g_e = engine_grads(eng)
        loss_m, lp_m, alpha_m = module_step(m_m, b, opt)
        g_m = {k: p.grad.cpu().numpy() for k, p in m_m.named_parameters() if p.grad is not None}
        ref_lp, ref_loss = g[tag + "/log_prob"][i], float(g[tag + "/loss"][i])
        d_e, d_m = dist(lp_e, ref_lp), dist(lp_m.cpu().numpy(), ref_lp)
        dl_e, dl_m = abs(loss_e - ref_loss), abs(float(loss_m) - ref_loss)
        print("%s step %d: log_prob engine %.2e module %.2e | loss engine %.2e module %.2e" % (tag, i, d_e, d_m, dl_e, dl_m))
        assert d_e <= (5e-5 if i == 0 else max(2 * d_m, 5e-5)), (tag, i, d_e, d_m)
        assert dl_e <= (5e-5 * lp_scale if i == 0 else max(2 * dl_m, 5e-5 * lp_scale)), (tag, i, dl_e, dl_m)
        if i == 0:
            da = dist(alpha_e.transpose(1, 0, 2), g[tag + "/alpha"])
            print("%s alpha engine %.2e module %.2e" % (tag, da, dist(alpha_m.cpu().numpy().transpose(1, 0, 2), g[tag + "/alpha"])))
            assert da <= 5e-5, (tag, da)
        worst = (0.0, 0.0, "")
        for k, ge in g_e.items():
            ref = g["%s/grad%d/%s" % (tag, i, k)]
            de, dm = dist(MG.sample(ge), ref), dist(MG.sample(g_m[k]), ref)
            worst = max(worst, (de, dm, k))
            assert de <= (5e-4 if i == 0 else max(2 * dm, 5e-4)), (tag, i, k, de, dm)
        print("%s step %d: worst gradient engine %.2e (module %.2e) %s" % (tag, i, *worst))
    worst = (0.0, 0.0, "")
    pm = dict(m_m.named_parameters())
    for k, p in m_e.named_parameters():
        ref = g["%s/param/%s" % (tag, k)].astype(np.float64)
        de = float(np.abs(MG.sample(p.detach().cpu().numpy()) - ref).max())
        dm = float(np.abs(MG.sample(pm[k].detach().cpu().numpy()) - ref).max())
        worst = max(worst, (de, dm, k))
        assert de <= max(2 * dm, 2 * LR * MG.N_STEPS), (tag, k, de, dm)
    print("%s final parameters: worst engine %.2e (module %.2e) %s" % (tag, *worst))
    assert int(eng.step_count.item()) == MG.N_STEPS


# ------------------------------------------------------------------------------------------------------------------
# 2. the module path on the same weights; the stack entry point against the per-layer chain
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B", [(33, 32), (5, 2)])
def test_engine_step_matches_module_path_autograd(S, B):
    """dropout 0: loss 2e-5 relative, log_prob 1e-4, every gradient tensor 2e-3 of its scale (the numbers
    tests/test_hip_drnn_engine.py uses for the same comparison)"""
    from gan_ffn_amd import engine as E
    net = mirror(7, formula=False, seed=3)
    ref = copy.deepcopy(net)
    b = random_batch(S, B, 7)
    loss_ref, lp_ref, alpha_ref = module_step(ref, b)
    eng = E.MeldEngine(net, lr=LR, weight_decay=L2)
    loss, lp = eng.step(b, train=True)
    torch.cuda.synchronize()
    print("(%d, %d): loss %.3e log_prob %.2e alpha %.2e" % (S, B, abs(float(loss) - float(loss_ref)), rel(lp, lp_ref), rel(eng.alpha, alpha_ref)))
    assert abs(float(loss) - float(loss_ref)) < 2e-5 * max(1.0, abs(float(loss_ref)))
    assert rel(lp, lp_ref) < 1e-4 and rel(eng.alpha, alpha_ref) < 1e-4
    refp = dict(ref.named_parameters())
    worst = (0.0, "")
    for i, k in enumerate(engine_named(eng)):
        assert refp[k].grad is not None, k
        r = rel(eng._p(i, True).view_as(refp[k]), refp[k].grad)
        worst = max(worst, (r, k))
        assert r < 2e-3, (k, r)
    print("(%d, %d): worst gradient %.2e %s" % (S, B, *worst))
    assert refp["linear.weight"].grad is None and len(eng._params) == 36


def test_lstm_stack_entry_points_give_the_bits_of_the_per_layer_chain():
    """ganffn_lstm_stack_fwd / _bwd against the chain ops.lstm_forward issues (ganffn_lstm_layer_* + ganffn_dropout per layer), same
    {seed, offsets}, train mode, p = 0.6: torch.equal on the output, the input gradient and all 32 parameter gradients"""
    from gan_ffn_amd import _lib, ops
    S, B, In, H, L, p = 33, 32, 600, 300, 4, 0.6
    torch.manual_seed(4)
    lstm = torch.nn.LSTM(In, H, num_layers=L, bidirectional=True, dropout=p).cuda().train()
    x = (torch.rand(S, B, In, device="cuda") - 0.5).requires_grad_(True)
    dy = torch.randn(S, B, 2 * H, device="cuda")
    ops.manual_seed(SEED)
    rng = ops.DeviceRng.get(x.device)
    rng.next_add(5)
    base = rng.counter
    out_c = ops.lstm_forward(x, lstm, True)
    assert rng.counter == base + L - 1
    out_c.backward(dy)
    names = [k for k, _ in lstm.named_parameters()]
    P = dict(lstm.named_parameters())
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    col = lambda j, src: [src[names[4 * i + j]] for i in range(2 * L)]
    G = {k: torch.zeros_like(v) for k, v in P.items()}
    Pd = {k: v.detach() for k, v in P.items()}
    cfg = _lib.LstmStackCfg(S, B, In, H, L, p, 1)
    lib = _lib.load()
    assert ops.lstm_family(B, False) == ""                      # ganffn_lstm_stack_fwd / _bwd and their size functions
    n_saved, n_ws = ops.lstm_sizes(cfg)
    assert n_saved > 0 and n_ws > 0
    saved, ws = torch.empty(n_saved, device="cuda"), torch.empty(n_ws, device="cuda")
    out_s, dx_s = torch.empty(S, B, 2 * H, device="cuda"), torch.empty(S, B, In, device="cuda")
    xd = x.detach()
    weights = [arr(col(j, Pd)) for j in range(4)]
    ops.lstm_stack_fwd_raw(cfg, xd, *weights, out_s, saved, ws, rng.state, base)
    ops.lstm_stack_bwd_raw(cfg, dy, xd, out_s, *weights[:2], dx_s, *[arr(col(j, G)) for j in range(4)], saved, ws, rng.state, base)
    torch.cuda.synchronize()
    assert torch.equal(out_s, out_c.detach())
    assert torch.equal(dx_s, x.grad)
    for k in names:
        assert torch.equal(G[k], P[k].grad), k
    assert float((out_s == 0).float().mean()) < 0.01           # (the last layer's output carries no dropout)
    # eval mode: no dropout, no rng needed
    cfg_e = _lib.LstmStackCfg(S, B, In, H, L, p, 0)
    out_e = torch.empty_like(out_s)
    ops.lstm_stack_fwd_raw(cfg_e, xd, *weights, out_e, saved, ws, None, 0)
    assert torch.equal(out_e, ops.lstm_forward(xd, lstm, False).detach())
    bad = _lib.LstmStackCfg(S, 33, In, H, L, p, 1)
    assert lib.ganffn_lstm_stack_saved_floats(C.byref(bad)) < 0


def test_meld_head_kernels_match_torch():
    """ganffn_meld_head_fwd / _bwd alone against torch's hardswish / linear under autograd (C = 7 and 3, a ragged T)"""
    from gan_ffn_amd import _lib, ops
    import torch.nn.functional as F
    for T, D, Cn in ((1056, 600, 7), (21, 600, 3), (50, 64, 16)):
        torch.manual_seed(T)
        e = (3 * torch.randn(T, D, device="cuda")).requires_grad_(True)
        a = (3 * torch.randn(T, D, device="cuda")).requires_grad_(True)
        w = (torch.randn(Cn, D, device="cuda") / D ** 0.5).requires_grad_(True)
        bias = torch.randn(Cn, device="cuda").requires_grad_(True)
        dl = torch.randn(T, Cn, device="cuda")
        hid_ref = F.hardswish(e + F.hardswish(a))
        logits_ref = hid_ref @ w.T + bias
        logits_ref.backward(dl)
        hid, logits = torch.empty(T, D, device="cuda"), torch.empty(T, Cn, device="cuda")
        d_e, d_a = torch.empty(T, D, device="cuda"), torch.empty(T, D, device="cuda")
        gw, gb = torch.zeros(Cn, D, device="cuda"), torch.zeros(Cn, device="cuda")
        P = ops._ptr
        _lib.call("ganffn_meld_head_fwd", P(e.detach()), P(a.detach()), P(w.detach()), P(bias.detach()), P(hid), P(logits), T, D, Cn, ops._stream())
        _lib.call("ganffn_meld_head_bwd", P(dl), P(e.detach()), P(a.detach()), P(hid), P(w.detach()), P(d_e), P(d_a), P(gw), P(gb), T, D, Cn,
                  ops._stream())
        torch.cuda.synchronize()
        r = [rel(hid, hid_ref), rel(logits, logits_ref), rel(d_e, e.grad), rel(d_a, a.grad), rel(gw, w.grad), rel(gb, bias.grad)]
        print("meld head (%d, %d, %d): hidden %.1e logits %.1e d_e %.1e d_att %.1e gw %.1e gb %.1e" % (T, D, Cn, *r))
        assert max(r) < 2e-5, r                                   # fp32 sums of <= 1056 / 600 terms in another order


# ------------------------------------------------------------------------------------------------------------------
# 3. train mode at the script's dropout against the fp64 oracle with the engine's own masks; Adam
# ------------------------------------------------------------------------------------------------------------------
def test_train_mode_step_matches_fp64_oracle_with_the_engines_masks():
    """(33, 32), dropout 0.6, two consecutive steps: the inter-layer masks are Philox sites SITE_LSTM + l at offsets base + l of
    the block the engine drew (distinct within a step; the next step's block starts after them); log_prob, the loss and every
    gradient element at 1e-3 of the tensor's scale, no outliers; Adam elementwise as
    tests/test_hip_classifier_engines_train_oracle._check_adam bounds it (padding floats stay 0)."""
    import meld_step_oracle as MO
    import test_hip_classifier_engines_train_oracle as TO
    from gan_ffn_amd import engine as E, ops
    S, B, C_ = 33, 32, 7
    net = mirror(C_, dropout=0.6, formula=False, seed=7)
    b = random_batch(S, B, C_, seed=9)
    ops.manual_seed(SEED)
    eng = E.MeldEngine(net, lr=LR, weight_decay=L2)
    names = engine_named(eng)
    assert names == MO.trained_names()
    sl = TO._Slab("meld", eng.slab, eng.grad, eng.exp_avg, eng.exp_avg_sq, eng.step_count, LR, L2,
                  [(o, p.numel()) for o, p in zip(eng._offs, eng._params)])
    text, umask, label = b["text"].cpu().numpy(), b["umask"].cpu().numpy(), b["label"].cpu().numpy()
    prev_base = None
    for i in range(2):
        pre = sl.host()
        P = {k: eng._p(j).view_as(eng._params[j]).detach().cpu().numpy().copy() for j, k in enumerate(names)}
        loss, lp = eng.step(b, train=True)
        torch.cuda.synchronize()
        post = sl.host(grad=True)
        base = eng._base_add
        offsets = [base + l for l in range(eng.L - 1)]
        assert eng.n_adds == eng.L - 1 and len(set(offsets)) == len(offsets)
        assert ops.DeviceRng.get(eng.dev).counter == base + eng.n_adds
        if prev_base is not None:
            assert base == prev_base + eng.n_adds            # the next block starts after this step's offsets
        prev_base = base
        seed, dev_off = [int(v) for v in ops.DeviceRng.get(eng.dev).state.cpu()]
        assert dev_off == 0
        o = MO.step(P, text, umask, label, 0.6, seed=seed, offsets=offsets, train=True)
        d_lp, d_loss = dist(lp.cpu().numpy(), o["log_prob"]), abs(float(loss) - o["loss"]) / abs(o["loss"])
        print("train oracle step %d: log_prob %.2e loss %.2e alpha %.2e" % (i, d_lp, d_loss, dist(eng.alpha.cpu().numpy(), o["alpha"])))
        assert d_lp <= 1e-3 and d_loss <= 1e-3
        g_e = engine_grads(eng)
        worst = (0.0, "")
        for k in names:
            d = dist(g_e[k], o["grads"][k])
            worst = max(worst, (d, k))
            assert d <= 1e-3, (i, k, d)
        print("train oracle step %d: worst gradient element %.2e of scale (%s)" % (i, *worst))
        TO._check_adam(sl, pre, post, "meld step %d" % i)
    # a different mask block gives a different step: the masks are really applied
    o2 = MO.step(P, text, umask, label, 0.6, seed=seed, offsets=[off + 100 for off in offsets], train=True)
    assert abs(o2["loss"] - o["loss"]) > 1e-6


# ------------------------------------------------------------------------------------------------------------------
# 4. what the step leaves alone
# ------------------------------------------------------------------------------------------------------------------
def test_linear_stays_untouched_and_eval_changes_nothing():
    from gan_ffn_amd import engine as E
    net = mirror(7, dropout=0.6, formula=False, seed=11)
    lin0 = (net.linear.weight.detach().clone(), net.linear.bias.detach().clone())
    b = random_batch(20, 6, 7)
    eng = E.MeldEngine(net)
    assert (eng.lr, eng.wd, eng.class_w) == (3e-4, 1e-4, None)          # the script's defaults
    for _ in range(3):
        eng.step(b, train=True)
    assert torch.equal(net.linear.weight, lin0[0]) and torch.equal(net.linear.bias, lin0[1])
    assert net.linear.weight.data_ptr() < eng.slab.data_ptr() or net.linear.weight.data_ptr() >= eng.slab.data_ptr() + 4 * eng.total
    state = [t.clone() for t in (eng.slab, eng.exp_avg, eng.exp_avg_sq, eng.step_count)]
    loss, lp = eng.step(b, train=False)
    torch.cuda.synchronize()
    for t0, t1 in zip(state, (eng.slab, eng.exp_avg, eng.exp_avg_sq, eng.step_count)):
        assert torch.equal(t0, t1)
    assert int(eng.step_count.item()) == 3
    net.eval()
    with torch.no_grad():
        loss_m, lp_m, alpha_m = module_step(net, b)
    print("eval: loss %.2e log_prob %.2e alpha %.2e" % (abs(float(loss) - float(loss_m)), rel(lp, lp_m), rel(eng.alpha, alpha_m)))
    assert abs(float(loss) - float(loss_m)) < 2e-5 * abs(float(loss_m)) and rel(lp, lp_m) < 1e-4 and rel(eng.alpha, alpha_m) < 1e-4
    pred = eng.predictions(lp)
    assert pred.shape == (6 * 20,) and torch.equal(pred, lp.transpose(0, 1).reshape(-1, 7).argmax(1))
    # weighted loss: class_weights reach ganffn_logsoftmax_nll
    w = [1.0, 0.5, 2.0, 1.5, 0.7, 0.3, 1.1]
    eng_w = E.MeldEngine(net, class_weights=w)
    loss_w, lp_w = eng_w.step(b, train=False)
    from gan_ffn_amd import model as M
    want = M.MaskedNLLLoss(torch.tensor(w, device="cuda"))(lp_m.transpose(0, 1).contiguous().view(-1, 7), b["label"].view(-1), b["umask"])
    assert abs(float(loss_w) - float(want)) < 2e-5 * abs(float(want))


# ------------------------------------------------------------------------------------------------------------------
# 5. determinism, buffer reuse
# ------------------------------------------------------------------------------------------------------------------
def test_two_engines_same_seed_are_bit_identical_and_reserve_keeps_buffers():
    from gan_ffn_amd import engine as E, ops
    b = random_batch(33, 32, 7)
    slabs = []
    for _ in range(2):
        net = mirror(7, dropout=0.6, formula=False, seed=13)
        ops.manual_seed(SEED)
        eng = E.MeldEngine(net)
        eng.reserve(33, 32)
        for _ in range(3):
            eng.step(b, train=True)
        torch.cuda.synchronize()
        slabs.append([t.clone() for t in (eng.slab, eng.grad, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.loss)])
    for t0, t1 in zip(*slabs):
        assert torch.equal(t0, t1)
    ptrs = {k: v.data_ptr() for k, v in eng._f.items()}
    short = random_batch(20, 7, 7, seed=6)
    loss, lp = eng.step(short, train=True)
    assert lp.shape == (20, 7, 7) and eng.alpha.shape == (7, 20, 20) and bool(torch.isfinite(loss))
    assert {k: v.data_ptr() for k, v in eng._f.items()} == ptrs
    assert eng.alpha.data_ptr() == ptrs["alpha"] and lp.data_ptr() == ptrs["log_prob"]


# ------------------------------------------------------------------------------------------------------------------
# 6. limits
# ------------------------------------------------------------------------------------------------------------------
def test_limits_raise_value_errors_that_name_the_module_path():
    from gan_ffn_amd import engine as E
    net = mirror(7, formula=False)
    eng = E.MeldEngine(net)
    before = eng.slab.clone()
    for S, B in ((5, 33), (129, 2)):
        b = {"text": torch.zeros(S, B, 600, device="cuda"), "umask": torch.ones(B, S, device="cuda"),
             "label": torch.zeros(B, S, dtype=torch.long, device="cuda")}
        with pytest.raises(ValueError, match="module path"):
            eng.step(b, train=True)
    assert int(eng.step_count.item()) == 0 and torch.equal(eng.slab, before)
    with pytest.raises(ValueError, match="module path"):
        E.MeldEngine(mirror(7, formula=False, dims=(600, 302, 604)))
    with pytest.raises(ValueError, match="module path"):
        E.MeldEngine(mirror(7, formula=False, dims=(602, 300, 600)))
    with pytest.raises(ValueError, match="module path"):
        E.MeldEngine(mirror(7, formula=False, dims=(600, 516, 1032)))        # 2 D_e > 1024
    # a parameter re-allocated after construction is refused
    net.lstm.weight_hh_l1.data = net.lstm.weight_hh_l1.data.clone()
    b = random_batch(5, 2, 7)
    with pytest.raises(RuntimeError, match="re-allocated"):
        eng.step(b, train=True)
    # sentiment: 3 classes run
    eng3 = E.MeldEngine(mirror(3, formula=False))
    loss, lp = eng3.step(random_batch(9, 3, 3), train=True)
    assert lp.shape == (9, 3, 3) and bool(torch.isfinite(loss))


# ------------------------------------------------------------------------------------------------------------------
# 7. the epoch loop
# ------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """an engine as train_or_eval_model sees it, keeping every step's unrounded loss and log-probabilities"""

    def __init__(self, eng):
        self.eng, self.losses, self.lps = eng, [], []

    def step(self, batch, train=True):
        loss, lp = self.eng.step(batch, train=train)
        self.losses.append((float(loss), float(batch["umask"].sum())))
        self.lps.append(lp.transpose(0, 1).reshape(-1, lp.shape[2]).detach().cpu().clone())
        self.alpha = self.eng.alpha
        return loss, lp

    def predictions(self, lp):
        return self.eng.predictions(lp)


def test_train_or_eval_model_matches_the_module_path_loop(tmp_path):
    """train_MELD.py:50-104 over a synthetic MELD pickle, one train epoch then one eval epoch, dropout 0: identical predictions
    where the top-two log-probabilities differ by more than 1e-4, epoch loss 2e-5 relative; eval collects one (B, S) attention
    tensor per query step of every batch, like the script's `alphas += alpha`"""
    from gan_ffn_amd import artifacts as A, data as D, engine as E
    path = str(tmp_path / "meld.pkl")
    D.write_synthetic_meld_pickle(path, n_train=40, n_test=12, seed=3)
    train_loader, _, test_loader = D.get_MELD_loaders(path, batch_size=16, valid=0.0)
    net = mirror(7, formula=False, seed=17)
    ref = copy.deepcopy(net)
    rec = _Recorder(E.MeldEngine(net, lr=LR, weight_decay=L2))
    rec.eng.reserve(33, 16)
    opt = torch.optim.Adam(ref.parameters(), lr=LR, weight_decay=L2)
    for train, loader in ((True, train_loader), (False, test_loader)):
        rec.losses, rec.lps = [], []
        torch.manual_seed(23)                            # the train sampler's permutation
        out = A.train_or_eval_model(rec, loader, train, "cuda", D.to_meld_batch)
        ref.train(train)
        torch.manual_seed(23)
        lps, labels, masks, tot, n_steps = [], [], [], [], 0
        for collated in loader:
            b = D.to_meld_batch(collated, "cuda")
            with torch.set_grad_enabled(train):
                loss, lp, alpha = module_step(ref, b, opt if train else None)
            lps.append(lp.transpose(0, 1).reshape(-1, 7).cpu())
            labels.append(b["label"].reshape(-1).cpu().numpy())
            masks.append(b["umask"].reshape(-1).cpu().numpy())
            tot.append((float(loss), float(b["umask"].sum())))
            n_steps += lp.shape[0]
        lp_m, lp_e = torch.cat(lps), torch.cat(rec.lps)
        masks = np.concatenate(masks)
        epoch_m = sum(l * n for l, n in tot) / sum(n for _, n in tot)
        epoch_e = sum(l * n for l, n in rec.losses) / sum(n for _, n in rec.losses)
        print("epoch (train=%s): loss engine %.7f module %.7f" % (train, epoch_e, epoch_m))
        assert abs(epoch_e - epoch_m) <= 2e-5 * abs(epoch_m)
        assert out[0] == round(epoch_e, 4)
        top2 = lp_m.topk(2, 1).values
        sure = ((top2[:, 0] - top2[:, 1]) > 1e-4).numpy() & (masks > 0)
        assert sure.sum() > 0.5 * (masks > 0).sum()
        assert np.array_equal(out[3][sure], lp_m.argmax(1).numpy()[sure])
        assert np.array_equal(out[2], np.concatenate(labels)) and np.array_equal(out[4], masks)
        alphas, vids = out[6][0], out[6][3]
        if train:
            assert alphas == [] and vids == []
        else:
            assert len(alphas) == n_steps and alphas[0].shape[0] == 12 and len(vids) == 12
            a0 = torch.stack(alphas[:alphas[0].shape[1]], 1)
            assert rel(a0, alpha) < 1e-4                 # (one test batch: the module path's last alpha)


def test_run_meld_training_runs_the_scripts_flow(tmp_path):
    """train_MELD.py:143-195 on a synthetic pickle: two epochs, the per-epoch line, the test epoch with the best F-score kept"""
    from gan_ffn_amd import artifacts as A, data as D
    path = str(tmp_path / "meld.pkl")
    D.write_synthetic_meld_pickle(path, n_train=20, n_test=6, seed=4)
    lines = []
    for classify, n_cls in (("emotion", 7), ("sentiment", 3)):
        best_loss, best_f, labels, preds, masks, att = A.run_meld_training(path, n_epochs=2, batch_size=8, classify=classify, seed=1,
                                                                           log=lines.append)
        assert np.isfinite(best_loss) and 0.0 <= best_f <= 100.0 and len(labels) == len(preds) == len(masks)
        assert int(preds.max()) < n_cls and len(att[3]) == 6 and len(att[0]) > 0
    assert len(lines) == 4 and lines[0].startswith("epoch 1 train_loss ") and "valid_loss nan" in lines[0]
