"""The two classifier step runners in TRAIN mode, dropout on, against the fp64 restatement of their steps
(tests/engine_oracle.py) with the engines' own Philox masks:
  * DrnnEngine (configuration 5, GAN_FFN_DialogueRNN; what `bench.py --config drnn` times), with and without listener state:
    dropout at the reference script's values (recurrence 0.1, dropout_rec 0.75, hidden 0.6; generators 0.2 / 0.1);
  * Phase2Engine (phase 2 of train_IEMOCAP.py: three generators -> sum -> fc -> weighted MaskedNLLLoss).
lr, L2 and class weights are the reference scripts' numbers (train_IEMOCAP_DialogueRNN.py:555-606,738,746;
train_IEMOCAP.py:453-456,653,661), not read back from the engines.

Each compared step is captured just before and just after it runs, and the oracle starts from the captured state (every
parameter slab, Adam moments and step count).  Per compared step:
  * offsets: every dropout-bearing launch (generator encoders / heads, the recurrence, the join of the two directions, the
    hidden layer) carries its slot of the step's block (EO.gen_adds, b + 6, b + 7) and the sites of the contract, every
    backward the offset of its own forward; the forward offsets of a step are distinct and the next block starts after them;
  * the generators' outputs at 1e-4 of scale;
  * the head, fed the ENGINE's fusion (so the generators' fp32 noise does not mix in): log-probabilities, the loss (2e-5
    relative), every head gradient tensor, dL/dfusion; the hidden layer's ReLU pattern is the engine's where the unit is
    kept, with a kink audit (a unit whose pattern differs from the oracle's own has a pre-activation within rounding of 0);
  * every element of every generator gradient tensor, fed the engine's dL/dfusion, on the ReLU patterns the HIP passes took
    (read from their saved activations), 1e-3 of the tensor's scale, no outliers;
  * Adam: fp64 Adam with L2 applied to the engine's own fp32 gradient and pre-step moments against the new parameters,
    moments and step count of every slab; the slabs' padding floats stay 0;
  * one chained oracle loss from the raw modalities (its own ReLU patterns everywhere), at a looser bound."""
import copy

import numpy as np
import pytest
import torch

import engine_oracle as EO
from util import _assert_close, relu_masks

pytestmark = pytest.mark.gpu

SEED = 20261016
W = [1.2, 0.60072, 0.38066, 0.94019, 0.67924, 0.34332]           # train_IEMOCAP_DialogueRNN.py:738 = train_IEMOCAP.py:653
DRNN_LR, DRNN_L2 = 1e-4, 1e-5                                    # train_IEMOCAP_DialogueRNN.py:555-567,746
P2_LR, P2_L2 = 1e-4, 0.008                                       # train_IEMOCAP.py:453-456,661
BETAS = (0.9, 0.999)                                             # torch.optim.Adam's defaults (both scripts)
DIMS = dict(D_m=100, D_g=500, D_p=500, D_e=100, D_h=100, D_a=100)

WORST = {}        # check kind -> largest error / tolerance seen in this module (printed at its end)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nclassifier engines train-mode oracle, largest error / tolerance per check: " +
          ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _close(kind, got, want, rtol, atol, label):
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu() if torch.is_tensor(want) else want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    _assert_close(got, want, rtol, atol, label, 0.0, 1.0)
    tol = atol + rtol * max(np.abs(want).max(), 1e-30)
    WORST[kind] = max(WORST.get(kind, 0.0), float(np.abs(got - want).max() / tol))


def _within(kind, err, tol, label):
    """elementwise bound, no outliers"""
    r = float((err / tol).max())
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    assert r <= 1.0, (label, r, int((err > tol).sum()), err.size)


class _Slab:
    """one Adam-stepped slab of an engine: parameters, gradient, moments, step count, its lr / L2, the (offset, numel) of
    the tensors on it (the rest is padding)"""

    def __init__(self, name, slab, grad, m, v, step, lr, wd, ranges):
        self.name, self.slab, self.grad, self.m, self.v, self.step = name, slab, grad, m, v, step
        self.lr, self.wd = lr, wd
        pad = np.ones(slab.numel(), dtype=bool)
        for o, n in ranges:
            assert pad[o:o + n].all(), (name, o, n)          # the tensors do not overlap
            pad[o:o + n] = False
        self.pad = pad

    def host(self, grad=False):
        d = dict(slab=self.slab.cpu().clone(), m=self.m.cpu().clone(), v=self.v.cpu().clone(), t=int(self.step.item()))
        if grad:
            d["grad"] = self.grad.cpu().clone()
        return d


def _gen_slabs(eng, lr, wd):
    return [_Slab(k, st.slab, st.grad, st.exp_avg, st.exp_avg_sq, st.step, lr, wd,
                  [(o, int(np.prod(s))) for o, s in st.named.values()]) for k, st in eng.G.items()]


def _check_adam(sl, pre, post, tag):
    """fp64 Adam (L2-coupled weight decay, the reference's lr) on the engine's own fp32 gradient and pre-step moments.
    The Adam kernels take their betas as fp32 and form 1 - beta and the bias corrections 1 - beta^t from them: they run
    Adam at beta2 = fl32(0.999) = 0.99900001287, whose new term (1 - beta2) of exp_avg_sq is 1.3e-5 smaller than the
    exact 0.001 (torch rounds the difference itself to fp32).  The oracle runs at the fp32 betas too."""
    t = pre["t"] + 1
    assert post["t"] == t, (tag, sl.name, pre["t"], post["t"])
    b1, b2 = (float(np.float32(b)) for b in BETAS)
    g = post["grad"].double().numpy()
    p0, m0, v0 = pre["slab"].double().numpy(), pre["m"].double().numpy(), pre["v"].double().numpy()
    p_o, m_o, v_o = EO.adam_wd(p0, g, m0, v0, t, sl.lr, b1, b2, sl.wd)
    # fp32 error of the kernel: g + wd p, m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g^2 round a few times (<= 2e-7 of the
    # terms' magnitude; the bound is on the terms, which may cancel: with L2 0.008, g + wd p nearly cancels on a few elements).
    # The new parameter rounds once to the fp32 grid of p, carries the update's own relative error (a few 1e-7 of an update
    # of at most ~lr: inside 1e-5 lr), the moments' error through m / (sqrt(v / bc2) + eps) (large only where g + wd p is
    # ~eps: there the update is lr * g / (|g| + eps), steep in g), and the rounding of the bias corrections: powf(beta, t) is
    # within 2 ulps, 1 - beta^t carries that absolutely (t >= 2; t = 1 is exact).  1e-37: fp32 denormals.
    tiny = 1e-37
    label = "%s %s" % (tag, sl.name)
    ge = np.abs(g) + np.abs(sl.wd * p0)
    dm = 1e-6 * (b1 * np.abs(m0) + (1 - b1) * ge) + tiny
    dv = 1e-6 * (b2 * np.abs(v0) + (1 - b2) * ge ** 2) + tiny
    _within("adam exp_avg", np.abs(post["m"].double().numpy() - m_o), dm, label + " exp_avg")
    _within("adam exp_avg_sq", np.abs(post["v"].double().numpy() - v_o), dv, label + " exp_avg_sq")
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    bc_rel = 0.0
    if t >= 2:
        u1, u2 = (float(np.spacing(np.float32(b ** t))) for b in (b1, b2))
        bc_rel = 2.0 * (u1 / bc1 + 0.5 * u2 / bc2)
    D = np.sqrt(v_o / bc2) + 1e-8
    dD = np.minimum(dv / (2.0 * np.sqrt(v_o * bc2) + tiny), np.sqrt(dv / bc2))
    d_upd = sl.lr / bc1 * (dm / D + np.abs(m_o) * dD / D ** 2)
    ulp = np.spacing(np.maximum(np.abs(p0), np.abs(p_o)).astype(np.float32)).astype(np.float64)
    _within("adam parameter", np.abs(post["slab"].double().numpy() - p_o),
            4 * ulp + 1e-5 * sl.lr + bc_rel * np.abs(p_o - p0) + d_upd, label + " parameter")
    # padding between the tensors: never written by a gradient, so parameters and moments stay 0
    for k in ("slab", "m", "v", "grad"):
        assert (post[k].numpy()[sl.pad] == 0).all(), (label, "padding", k)


def _kink_audit(pre, pattern, kept, tag):
    """where the engine's ReLU pattern (on kept units) differs from the fp64 pre-activation's sign, that pre-activation is
    rounding noise, and there are few such units"""
    own = pre > 0
    diff = kept & (own != pattern)
    scale = max(1.0, float(pre.abs().max()))
    worst = float(pre[diff].abs().max()) if bool(diff.any()) else 0.0
    WORST["hidden kink"] = max(WORST.get("hidden kink", 0.0), worst / (1e-4 * scale))
    assert worst <= 1e-4 * scale, (tag, worst, scale)
    assert int(diff.sum()) <= max(2, int(1e-3 * int(kept.sum()))), (tag, int(diff.sum()))


# ---- launch taps -------------------------------------------------------------------------------------------------------
OPS_TAPS = {"encoder_fwd_raw": 8, "head_fwd_raw": 12, "head_bwd_raw": 16, "encoder_bwd_raw": 9}     # position of `add`
# _lib.call names of the head's dropout-bearing launches -> position of the offset among the arguments
CALL_TAPS = {"ganffn_drnn_fwd": -2, "ganffn_drnn_bwd": -2, "ganffn_drnn_listener_fwd": -2, "ganffn_drnn_listener_bwd": -2,
             "ganffn_drnn_join_fwd": -3, "ganffn_drnn_join_bwd": -3, "ganffn_ffn_linear1_fwd": -3}


class _Taps:
    def __init__(self, monkeypatch):
        from gan_ffn_amd import _lib, ops
        self.log = None
        for name, pos in OPS_TAPS.items():
            monkeypatch.setattr(ops, name, self._tap_op(name, getattr(ops, name), pos))
        monkeypatch.setattr(_lib, "call", self._tap_call(_lib.call))

    def _tap_op(self, name, fn, pos):
        def tapped(*a, **kw):
            if self.log is not None:
                self.log.append((name, int(a[pos]), ()))
            return fn(*a, **kw)
        return tapped

    def _tap_call(self, fn):
        def tapped(name, *a):
            if self.log is not None and name in CALL_TAPS:
                vals = [getattr(x, "value", x) for x in a]
                # join: (p, site_f, site_b, rng, add, train); linear1: (p, site, rng, add, train); drnn: the offset only
                extra = tuple(vals[-7:-4] + vals[-2:-1]) if "join" in name else \
                    tuple(vals[-6:-4] + vals[-2:-1]) if "linear1" in name else ()
                self.log.append((name, int(vals[CALL_TAPS[name]]), extra))
            return fn(name, *a)
        return tapped


def _fl(x):
    return float(np.float32(x))


def _want_drnn_launches(b, listener, train, p_join, p_hid):
    ga = EO.gen_adds(b)
    fwd = []
    for k in EO.GEN_KEYS:
        fwd += [("encoder_fwd_raw", ga[k][0], ()), ("head_fwd_raw", ga[k][1], ())]
    rec = "ganffn_drnn_listener" if listener else "ganffn_drnn"
    t = 1 if train else 0
    fwd += [(rec + "_fwd", b + EO.A_REC, ()),
            ("ganffn_drnn_join_fwd", b + EO.A_HEAD, (_fl(p_join), EO.SITE_JOIN_F, EO.SITE_JOIN_B, t)),
            ("ganffn_ffn_linear1_fwd", b + EO.A_HEAD, (_fl(p_hid), EO.SITE_HIDDEN, t))]
    if not train:
        return fwd
    bwd = [("ganffn_drnn_join_bwd", b + EO.A_HEAD, (_fl(p_join), EO.SITE_JOIN_F, EO.SITE_JOIN_B, 1)), (rec + "_bwd", b + EO.A_REC, ())]
    for k in EO.GEN_KEYS:
        bwd += [("head_bwd_raw", ga[k][1], ()), ("encoder_bwd_raw", ga[k][0], ())]
    return fwd + bwd


def _want_phase2_launches(b, train):
    ga = EO.gen_adds(b)
    out = []
    for k in EO.GEN_KEYS:
        out += [("encoder_fwd_raw", ga[k][0], ()), ("head_fwd_raw", ga[k][1], ())]
    if train:
        for k in EO.GEN_KEYS:
            out += [("head_bwd_raw", ga[k][1], ()), ("encoder_bwd_raw", ga[k][0], ())]
    return out


def _check_blocks(bases, n):
    """each step's block of n offsets starts after the previous one (no two steps share a mask)"""
    for a_, b_ in zip(bases, bases[1:]):
        assert b_ >= a_ + n, bases


# ---- batches -----------------------------------------------------------------------------------------------------------
def _batch(S, B, seed, lens=None, single=None):
    """a ragged batch with the lengths given (default: random, with S and 1 among them), qmask one-hot on valid steps,
    dialogue `single` spoken by one party only"""
    g = torch.Generator().manual_seed(seed)
    if lens is None:
        lens = torch.randint(1, S + 1, (B,), generator=g)
        lens[0] = S
        if B > 1:
            lens[1] = 1
    lens = torch.as_tensor(lens)
    assert int(lens.max()) == S and int(lens.min()) >= 1
    valid = (torch.arange(S).unsqueeze(1) < lens.unsqueeze(0)).float()             # (S, B)
    out = {}
    for k, d in (("acoustic", 100), ("visual", 512), ("text", 100)):
        out[k] = torch.rand(S, B, d, generator=g) * valid.unsqueeze(2)
    spk = torch.randint(0, 2, (S, B), generator=g)
    if single is None:
        single = min(2, B - 1)
    spk[:, single] = 1
    out["qmask"] = torch.nn.functional.one_hot(spk, 2).float() * valid.unsqueeze(2)
    out["umask"] = valid.t().contiguous()
    out["label"] = torch.randint(0, 6, (B, S), generator=g) * valid.t().long()
    return {k: v.cuda() for k, v in out.items()}


def _host_batch(batch):
    return {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items()}


# ================================================================================================================
# DrnnEngine
# ================================================================================================================
def _drnn_net(listener, seed=3):
    from gan_ffn_amd import model as M
    torch.manual_seed(seed)
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                listener_state=listener, context_attention="general", dropout_rec=0.1, dropout=0.6, **DIMS)
    return net.cuda().train()


class _DrnnHarness:
    """wraps one DrnnEngine's _step: state before and after, the launches in between, the engine's intermediates"""

    def __init__(self, eng, net, monkeypatch, compare=True):
        self.eng, self.compare = eng, compare
        self.taps = _Taps(monkeypatch)
        self.bases, self.compared = [], 0
        names = {id(p): n for n, p in net.named_parameters()}
        self.hnames = [names[id(p)][len("bi_model."):] for p in eng._hparams]
        assert all(names[id(p)].startswith("bi_model.") for p in eng._hparams)
        self.bm = copy.deepcopy(net.bi_model).cpu().double()
        assert set(self.hnames) == {n for n, _ in self.bm.named_parameters()}
        self.slabs = _gen_slabs(eng, DRNN_LR, DRNN_L2) + [
            _Slab("head", eng.h_slab, eng.h_grad, eng.h_m, eng.h_v, eng.h_step, DRNN_LR, DRNN_L2,
                  [(o, p.numel()) for o, p in zip(eng._hoffs, eng._hparams)])]
        step = eng._step
        eng._step = lambda batch, train=True: self._run(step, batch, train)

    def _load_head(self, slab):
        params = dict(self.bm.named_parameters())
        with torch.no_grad():
            for n, o, p in zip(self.hnames, self.eng._hoffs, self.eng._hparams):
                params[n].copy_(slab[o:o + p.numel()].view(p.shape).double())
        return self.bm

    def _run(self, step, batch, train):
        eng = self.eng
        torch.cuda.synchronize()
        pre = [sl.host() for sl in self.slabs]
        self.taps.log = []
        out = step(batch, train)
        torch.cuda.synchronize()
        log, self.taps.log = self.taps.log, None
        b = eng._base_add
        self.bases.append(b)
        post = [sl.host(grad=True) for sl in self.slabs]
        p_join, p_hid = eng.p_join, eng.p_hid
        assert log == _want_drnn_launches(b, eng.listener, train, p_join, p_hid), (b, log)
        fwd = [a for n, a, _ in log if "fwd" in n]
        assert len(set(fwd)) == len(fwd) - 1 and set(fwd) == set(range(b, b + 8)), (b, fwd)   # (join + linear1 share b + 7)
        if not self.compare:
            return out
        S, B = batch["text"].shape[:2]
        T, f = S * B, eng._f
        hb = _host_batch(batch)
        tag = "step %d (%d, %d)%s" % (len(self.bases) - 1, S, B, "" if train else " eval")
        if train:
            self._check_train(b, S, B, T, f, hb, pre, post, tag)
        else:
            self._check_eval(S, B, T, f, hb, pre, post, tag)
        self.compared += 1
        return out

    def _engine(self, S, B, T, f):
        eng = self.eng
        Dm, Dh2, Cn = eng.Dm, eng.Dh2, eng.n_classes
        return dict(outs={k: eng.pass_G[k].out.cpu().double() for k in EO.GEN_KEYS},
                    fusion=f["fusion"][:T * Dm].view(S, B, Dm).cpu().double(),
                    hidden=f["hidden"][:T * Dh2].view(S, B, Dh2).cpu().double(),
                    log_prob=f["log_prob"][:T * Cn].view(S, B, Cn).cpu().double(),
                    d_fusion=f["dU_f"][:T * Dm].view(S, B, Dm).cpu().double(), loss=float(eng.loss))

    def _check_train(self, b, S, B, T, f, hb, pre, post, tag):
        eng = self.eng
        e = self._engine(S, B, T, f)
        gens = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"]) for i, k in enumerate(EO.GEN_KEYS)}
        masks_g = {k: relu_masks(eng.pass_G[k], eng.pass_G[k].cfg_train, S, B) for k in EO.GEN_KEYS}
        # generators, on the HIP ReLU patterns
        outs = EO.generators(gens, hb, SEED, EO.gen_adds(b), masks_g)
        for k in EO.GEN_KEYS:
            _close("generator output", e["outs"][k], outs[k], 1e-4, 0.0, "%s %s output" % (tag, k))
        # head on the engine's fusion and its hidden ReLU pattern
        bm = self._load_head(pre[3]["slab"])
        masks = EO.drnn_masks(bm, S, B, SEED, b + EO.A_REC, b + EO.A_HEAD)
        kept = masks["hidden"] > 0
        pattern = e["hidden"] > 0
        res = EO.drnn_head(bm, e["fusion"], hb["qmask"], hb["umask"], hb["label"], W, masks, pattern)
        _kink_audit(res["pre"], pattern, kept, tag)
        _close("hidden", e["hidden"], res["hidden"], 1e-4, 0.0, tag + " hidden")
        _close("log_prob", e["log_prob"], res["log_prob"], 1e-4, 0.0, tag + " log_prob")
        _within("loss", np.array([abs(e["loss"] - res["loss"])]), np.array([2e-5 * abs(res["loss"])]), tag + " loss")
        hg = post[3]["grad"]
        assert len(self.hnames) == (40 if eng.listener else 32)
        for n, o, p in zip(self.hnames, eng._hoffs, eng._hparams):
            _close("head gradient", hg[o:o + p.numel()].view(p.shape), res["grads"][n], 1e-3, 1e-12, "%s grad %s" % (tag, n))
        _close("d_fusion", e["d_fusion"], res["d_fusion"], 1e-3, 1e-12, tag + " d_fusion")
        # generator gradients from the engine's dL/dfusion
        gg = EO.generator_grads(gens, outs, e["d_fusion"])
        for i, k in enumerate(EO.GEN_KEYS):
            st = eng.G[k]
            assert set(gg[k]) == set(st.named)
            for n, (o, shape) in st.named.items():
                _close("generator gradient", post[i]["grad"][o:o + int(np.prod(shape))].view(*shape), gg[k][n], 1e-3, 1e-12,
                       "%s %s grad %s" % (tag, k, n))
        for sl, a, z in zip(self.slabs, pre, post):
            _check_adam(sl, a, z, tag)
        # chained: the whole step from the raw modalities, every ReLU pattern the oracle's own
        gens0 = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"]) for i, k in enumerate(EO.GEN_KEYS)}
        ch = EO.drnn_step(gens0, bm, hb, SEED, b, True, class_w=W)
        _within("chained loss", np.array([abs(e["loss"] - ch["loss"])]), np.array([2e-4 * abs(ch["loss"])]), tag + " chained loss")

    def _check_eval(self, S, B, T, f, hb, pre, post, tag):
        """eval: no dropout anywhere, nothing trained (slabs, moments and step counts bit-unchanged)"""
        eng = self.eng
        e = self._engine(S, B, T, f)
        gens = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"], requires_grad=False) for i, k in enumerate(EO.GEN_KEYS)}
        with torch.no_grad():
            outs = EO.generators(gens, hb, SEED, None)
        for k in EO.GEN_KEYS:
            _close("generator output", e["outs"][k], outs[k], 1e-4, 0.0, "%s %s output" % (tag, k))
        bm = self._load_head(pre[3]["slab"])
        pattern = e["hidden"] > 0
        res = EO.drnn_head(bm, e["fusion"], hb["qmask"], hb["umask"], hb["label"], W, None, pattern)
        _kink_audit(res["pre"], pattern, torch.ones_like(pattern), tag)
        _close("log_prob", e["log_prob"], res["log_prob"], 1e-4, 0.0, tag + " log_prob")
        _within("loss", np.array([abs(e["loss"] - res["loss"])]), np.array([2e-5 * abs(res["loss"])]), tag + " loss")
        for sl, a, z in zip(self.slabs, pre, post):
            for k in ("slab", "m", "v"):
                assert torch.equal(a[k], z[k]), (tag, sl.name, k)
            assert a["t"] == z["t"], (tag, sl.name)


def _drnn_run(monkeypatch, listener, shapes, n_streams=1, compare=True, eval_after=False, seed=3):
    from gan_ffn_amd import engine as E, ops
    net = _drnn_net(listener, seed)
    eng = E.DrnnEngine(net, lr=DRNN_LR, weight_decay=DRNN_L2, class_weights=W, n_streams=n_streams)
    assert (eng.p_rec, eng.p_join, eng.p_hid) == (0.1, 0.75, 0.6) and eng.listener == listener
    for st in eng.G.values():
        assert (st.p_pe, st.p_enc, st.p_head) == (0.2, 0.1, 0.2)
    h = _DrnnHarness(eng, net, monkeypatch, compare)
    eng.reserve(max(S for S, _, _ in shapes), max(B for _, B, _ in shapes))
    ops.manual_seed(SEED)
    losses = []
    for i, (S, B, kw) in enumerate(shapes):
        loss, _ = eng.step(_batch(S, B, 100 * S + B + i, **kw), train=True)
        losses.append(float(loss))
    if eval_after:
        S, B, kw = shapes[-1]
        eng.step(_batch(S, B, 7 + S, **kw), train=False)
    torch.cuda.synchronize()
    _check_blocks(h.bases, EO.DRNN_ADDS)
    assert h.compared == (len(shapes) + (1 if eval_after else 0) if compare else 0)
    return eng, net, losses


DRNN_CASES = {
    "13x4": [(13, 4, {}), (13, 4, {})],          # (then an eval step)
    "33x7_three_steps": [(33, 7, dict(lens=[33, 1, 20, 33, 7, 12, 2])), (21, 7, dict(lens=[21, 3, 1, 21, 15, 9, 21])),
                         (33, 5, dict(lens=[1, 33, 30, 4, 33], single=0))],
    "94x30": [(94, 30, {})],            # the bench batch
    "110x32": [(110, 32, {})],          # the largest batch the engine takes (DrnnEngine._prepare5: B <= 32; PE table: S <= 110)
}


@pytest.mark.parametrize("case", list(DRNN_CASES))
def test_drnn_engine_train_step_matches_fp64_oracle(case, monkeypatch):
    _drnn_run(monkeypatch, False, DRNN_CASES[case], eval_after=(case == "13x4"))


@pytest.mark.parametrize("S,B", [(13, 4), (94, 30)])
def test_drnn_engine_listener_train_step_matches_fp64_oracle(S, B, monkeypatch):
    _drnn_run(monkeypatch, True, [(S, B, {}), (S, B, {})] if S < 50 else [(S, B, {})])


def test_drnn_engine_three_streams_bit_equal_one_stream_and_match_the_oracle(monkeypatch):
    shapes = [(33, 7, {}), (33, 7, dict(lens=[33, 1, 5, 33, 2, 30, 17]))]
    eng1, net1, l1 = _drnn_run(monkeypatch, False, shapes, n_streams=1, compare=False)
    monkeypatch.undo()
    eng3, net3, l3 = _drnn_run(monkeypatch, False, shapes, n_streams=3, compare=True)
    assert eng3.streams is not None and len(eng3.streams) == 3
    assert l1 == l3, (l1, l3)
    for a, b in ((eng1.h_slab, eng3.h_slab), (eng1.h_m, eng3.h_m), (eng1.h_v, eng3.h_v)):
        assert torch.equal(a, b)
    for k in EO.GEN_KEYS:
        for a, b in ((eng1.G[k].slab, eng3.G[k].slab), (eng1.G[k].exp_avg, eng3.G[k].exp_avg),
                     (eng1.G[k].exp_avg_sq, eng3.G[k].exp_avg_sq)):
            assert torch.equal(a, b), k


# ================================================================================================================
# Phase2Engine
# ================================================================================================================
class _Phase2Harness:
    def __init__(self, eng, monkeypatch):
        self.eng = eng
        self.taps = _Taps(monkeypatch)
        self.bases, self.compared = [], 0
        nw, nb = eng.fc_w.numel(), eng.fc_b.numel()
        self.slabs = _gen_slabs(eng, P2_LR, P2_L2) + [
            _Slab("fc", eng.fc_slab, eng.fc_grad, eng.fc_m, eng.fc_v, eng.fc_step, P2_LR, P2_L2, [(0, nw), (eng.fc_off_b, nb)])]
        step = eng.step
        eng.step = lambda batch, train=True: self._run(step, batch, train)

    def _run(self, step, batch, train):
        eng = self.eng
        torch.cuda.synchronize()
        pre = [sl.host() for sl in self.slabs]
        self.taps.log = []
        out = step(batch, train)
        torch.cuda.synchronize()
        log, self.taps.log = self.taps.log, None
        b = eng._base_add
        self.bases.append(b)
        assert log == _want_phase2_launches(b, train), (b, log)
        post = [sl.host(grad=True) for sl in self.slabs]
        S, B = batch["text"].shape[:2]
        tag = "phase2 step %d (%d, %d)" % (len(self.bases) - 1, S, B)
        hb = _host_batch(batch)
        nw, C_ = eng.fc_w.numel(), eng.n_classes
        fc_w = pre[3]["slab"][:nw].view(C_, 100)
        fc_b = pre[3]["slab"][eng.fc_off_b:eng.fc_off_b + C_]
        gens = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"]) for i, k in enumerate(EO.GEN_KEYS)}
        masks_g = {k: relu_masks(eng.pass_G[k], eng.pass_G[k].cfg_train, S, B) for k in EO.GEN_KEYS}
        outs = EO.generators(gens, hb, SEED, EO.gen_adds(b), masks_g)
        for k in EO.GEN_KEYS:
            _close("generator output", eng.pass_G[k].out.cpu(), outs[k], 1e-4, 0.0, "%s %s output" % (tag, k))
        res = EO.phase2_head(eng.fusion.cpu().double(), fc_w, fc_b, hb["label"], hb["umask"], W)
        _close("log_prob", eng.log_prob.cpu(), res["log_prob"], 1e-4, 0.0, tag + " log_prob")
        _within("loss", np.array([abs(float(eng.loss) - res["loss"])]), np.array([2e-5 * abs(res["loss"])]), tag + " loss")
        g = post[3]["grad"]
        _close("head gradient", g[:nw].view(C_, 100), res["grad_fc_weight"], 1e-3, 1e-12, tag + " grad fc.weight")
        _close("head gradient", g[eng.fc_off_b:eng.fc_off_b + C_], res["grad_fc_bias"], 1e-3, 1e-12, tag + " grad fc.bias")
        d_fusion = eng.d_fusion.cpu().double()
        _close("d_fusion", d_fusion, res["d_fusion"], 1e-3, 1e-12, tag + " d_fusion")
        gg = EO.generator_grads(gens, outs, d_fusion)
        for i, k in enumerate(EO.GEN_KEYS):
            for n, (o, shape) in eng.G[k].named.items():
                _close("generator gradient", post[i]["grad"][o:o + int(np.prod(shape))].view(*shape), gg[k][n], 1e-3, 1e-12,
                       "%s %s grad %s" % (tag, k, n))
        for sl, a, z in zip(self.slabs, pre, post):
            _check_adam(sl, a, z, tag)
        gens0 = {k: EO.Net.from_state(eng.G[k], pre[i]["slab"]) for i, k in enumerate(EO.GEN_KEYS)}
        ch = EO.phase2_step(gens0, fc_w, fc_b, hb, SEED, EO.gen_adds(b), class_w=W)
        _within("chained loss", np.array([abs(float(eng.loss) - ch["loss"])]), np.array([2e-4 * abs(ch["loss"])]),
                tag + " chained loss")
        self.compared += 1
        return out


@pytest.mark.parametrize("shapes", [[(7, 2, dict(lens=[7, 1]))], [(33, 5, {})], [(94, 32, {}), (94, 32, {})]],
                         ids=["7x2", "33x5_ragged", "94x32_two_steps"])
def test_phase2_engine_train_step_matches_fp64_oracle(shapes, monkeypatch):
    from gan_ffn_amd import engine as E, model, ops
    gens, _ = E.build_networks(device="cuda", seed=11)
    net = model.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6).cuda()
    eng = E.Phase2Engine(net, lr=P2_LR, weight_decay=P2_L2, class_weights=W)
    for st in eng.G.values():
        assert (st.p_pe, st.p_enc, st.p_head) == (0.2, 0.1, 0.2)
    h = _Phase2Harness(eng, monkeypatch)
    ops.manual_seed(SEED)
    for i, (S, B, kw) in enumerate(shapes):
        batch = _batch(S, B, 31 * S + B + i, **kw)
        eng.step({k: batch[k] for k in ("acoustic", "visual", "text", "umask", "label")}, train=True)
    torch.cuda.synchronize()
    assert h.compared == len(shapes)
    _check_blocks(h.bases, EO.PHASE2_ADDS)
