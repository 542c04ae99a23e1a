"""The step runner `bench.py` times (GanEngine.iteration, n_streams = 1) in TRAIN mode, dropout on, against the fp64
restatement of its sub-steps (tests/engine_oracle.py) with the engine's own Philox masks.

Each compared sub-step is captured just before and just after it runs, and the oracle starts from the captured
pre-sub-step state (parameters, Adam moments and step of the trained network, parameters of its partner), so any subset
of the sub-steps can be compared on its own.  Per compared sub-step:
  * offsets: the engine's dropout-bearing launches carry exactly the offsets of the sub-step's slots (b + 4i + 0..3:
    generator encoder / head, discriminator encoder / head), every backward the offset of its own forward; the 4n offsets
    of an iteration are distinct and the next iteration's block starts after them;
  * the generator's eval-mode fake (train_disc) or its train-mode output (train_gen) at 1e-4 of scale; the oracle's
    discriminator is then fed the ENGINE's fake, so D's gradients are not mixed with G's fp32 noise;
  * the loss, 2e-5 relative;
  * EVERY element of EVERY parameter tensor's gradient of the trained network (8 layers x 12 tensors, fc*, object.*), on the
    ReLU patterns the HIP passes took (read from their saved activations), 1e-3 of the tensor's scale, no outliers;
  * Adam: fp64 Adam applied to the engine's own fp32 gradient and pre-step moments (the reference's lr of that network,
    betas (0.5, 0.6), step t) against the engine's new parameters, moments and step count;
  * the partner is bit-unchanged (its slab, moments and step).
GANFFN_ADAM_PARTS=0 keeps the summed gradient in net.grad; that the unreduced-chunk path gives the same bits is
tests/test_hip_engine.py::test_unreduced_weight_gradient_chunks_give_the_reduce_launchs_bits."""
import numpy as np
import pytest
import torch

import engine_oracle as EO
import formula as F_
from util import DIN, DISC, GEN, MELD_DIN, MELD_DISC, MELD_GEN, _assert_close, formula_sd, relu_masks

pytestmark = pytest.mark.gpu

SEED = 20261015
# optimizers of train_IEMOCAP.py:292-297 with the call's lr and betas (:603-606): generators lr, the text generator 1.1 lr,
# discriminators lr / 2 — the oracle's own numbers, not read back from the engine
LR, BETAS = 1e-4, (0.5, 0.6)


def _ref_lr(kind, who):
    return LR / 2 if kind == "D" else LR * (1.1 if who == "text" else 1.0)


WORST = {}        # check kind -> largest error / tolerance seen in this module (printed at its end)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nengine train-mode oracle, largest error / tolerance per check: " +
          ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _close(kind, got, want, rtol, atol, label):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    _assert_close(got, want, rtol, atol, label, 0.0, 1.0)
    tol = atol + rtol * max(np.abs(want).max(), 1e-30)
    WORST[kind] = max(WORST.get(kind, 0.0), float(np.abs(got - want).max() / tol))


def _within(kind, err, tol, label):
    """elementwise bound, no outliers"""
    r = float((err / tol).max())
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    assert r <= 1.0, (label, r, int((err > tol).sum()), err.size)


def _networks(gen_table, disc_table):
    from gan_ffn_amd import model
    out = []
    for table in (gen_table, disc_table):
        nets = {}
        for k, cls in table.items():
            m = getattr(model, cls)(100, dropout=0.2)       # dropout ON: 0.2 head / 0.2 positional / 0.1 encoder layers
            missing = m.load_state_dict({a: torch.from_numpy(b) for a, b in formula_sd(cls).items()}, strict=False)
            assert missing.missing_keys == ["position_encoding.pe"] and not missing.unexpected_keys
            nets[k] = m.cuda()
        out.append(nets)
    return out


def _host(st):
    return dict(slab=st.slab.cpu().clone(), m=st.exp_avg.cpu().clone(), v=st.exp_avg_sq.cpu().clone(), t=int(st.step.item()))


class _Harness:
    """wraps one engine's train_disc / train_gen and the raw launches that take a dropout offset"""
    TAPS = {"encoder_fwd_raw": 8, "head_fwd_raw": 12, "head_bwd_raw": 16, "encoder_bwd_raw": 9}   # position of `add`

    def __init__(self, eng, compare, monkeypatch):
        from gan_ffn_amd import ops
        self.eng, self.compare = eng, compare
        self.it, self.sub = 0, None
        self.launches = {}            # (iteration, sub-step) -> [(launch, offset)]
        self.base = {}                # iteration -> eng._base_add
        self.compared = 0
        for name, pos in self.TAPS.items():
            monkeypatch.setattr(ops, name, self._tap(name, getattr(ops, name), pos))
        td, tg = eng.train_disc, eng.train_gen
        eng.train_disc = lambda who, partner, batch, i: self._run("D", td, who, partner, batch, i)
        eng.train_gen = lambda who, partner, batch, i, g_adds=None: self._run("G", tg, who, partner, batch, i, g_adds)

    def _tap(self, name, fn, pos):
        def tapped(*a, **kw):
            assert self.sub is not None, name
            self.launches.setdefault((self.it, self.sub), []).append((name, int(a[pos])))
            return fn(*a, **kw)
        return tapped

    def _run(self, kind, fn, who, partner, batch, i, *extra):
        eng = self.eng
        b = self.base.setdefault(self.it, eng._base_add)
        assert eng._base_add == b
        self.sub = i
        if (self.it, i) not in self.compare:
            fn(who, partner, batch, i, *extra)
            self.sub = None
            return
        tr, pa = (eng.D[who], eng.G[partner]) if kind == "D" else (eng.G[who], eng.D[partner])
        torch.cuda.synchronize()
        pre, pre_p = _host(tr), _host(pa)
        fn(who, partner, batch, i, *extra)
        torch.cuda.synchronize()
        S, B = batch[who].shape[:2]
        post, post_p = _host(tr), _host(pa)
        post["grad"] = tr.grad.cpu().clone()
        loss = float(eng.losses[i])
        xs = {k: batch[k].cpu().double() for k in (who, partner)}
        self.sub = None
        if kind == "D":
            pd = eng.pass_D2[who]
            masks = relu_masks(pd, pd.cfg_train, S, 2 * B)
            fake = eng.pass_G_nosave[partner].out.cpu().double()
            self._check_disc(tr, pa, xs[who], xs[partner], b, i, pre, pre_p, post, loss, masks, fake, _ref_lr(kind, who))
        else:
            pg, pd = eng.pass_G[who], eng.pass_D1[partner]
            masks_g = relu_masks(pg, pg.cfg_train, S, B)
            masks_d = relu_masks(pd, pd.cfg_eval, S, B)        # the frozen discriminator ran in eval mode
            out = pg.out.cpu().double()
            self._check_gen(tr, pa, xs[who], b, i, pre, pre_p, post, loss, masks_g, masks_d, out, _ref_lr(kind, who))
        # the partner only lends its parameters: bit-unchanged
        assert torch.equal(post_p["slab"], pre_p["slab"]) and torch.equal(post_p["m"], pre_p["m"]) and \
            torch.equal(post_p["v"], pre_p["v"]) and post_p["t"] == pre_p["t"], (kind, who, partner, i)
        self.compared += 1

    def _check_disc(self, st, gst, xr, xp, b, i, pre, pre_p, post, loss, masks, fake, lr):
        tag = "it%d sub-step %d D %s" % (self.it, i, st.m.__class__.__name__)
        D = EO.Net.from_state(st, pre["slab"])
        G = EO.Net.from_state(gst, pre_p["slab"], requires_grad=False)
        with torch.no_grad():
            fake_o = G.forward(xp, SEED, b + 4 * i + EO.G_ENC, b + 4 * i + EO.G_HEAD, False)
        _close("fake (G eval)", fake, fake_o, 1e-4, 0.0, tag + " fake")
        res = EO.disc_substep(D, G, xr, xp, SEED, b, i, fake=fake, relu_masks=masks)
        self._check_common(st, tag, res, pre, post, loss, lr)

    def _check_gen(self, st, dst, x, b, i, pre, pre_p, post, loss, masks_g, masks_d, out, lr):
        tag = "it%d sub-step %d G %s" % (self.it, i, st.m.__class__.__name__)
        G = EO.Net.from_state(st, pre["slab"])
        D = EO.Net.from_state(dst, pre_p["slab"], requires_grad=False)
        res = EO.gen_substep(G, D, x, SEED, b, i, masks_g, masks_d)
        _close("G train output", out, res["out"], 1e-4, 0.0, tag + " output")
        self._check_common(st, tag, res, pre, post, loss, lr)

    def _check_common(self, st, tag, res, pre, post, loss, lr):
        # loss: fp32 means over <= 6016 positions of the same probabilities
        err = abs(loss - res["loss"])
        _within("loss", np.array([err]), np.array([2e-5 * abs(res["loss"])]), tag + " loss")
        # every parameter tensor in the slab has a gradient in the oracle, and every one is compared
        assert set(res["grads"]) == set(st.named), set(res["grads"]) ^ set(st.named)
        assert len(st.named) == 12 * st.L + 2 * (2 if st.kind == 0 else 3) + (2 if st.has_obj else 0)
        g32 = post["grad"]
        for k, (off, shape) in st.named.items():
            n = int(np.prod(shape))
            _close("gradient", g32[off:off + n].view(*shape).double().numpy(), res["grads"][k].numpy(), 1e-3, 1e-8,
                   "%s grad %s" % (tag, k))
        # Adam step t on the engine's own fp32 gradient and moments
        t = pre["t"] + 1
        assert post["t"] == t, (tag, pre["t"], post["t"])
        b1, b2 = BETAS
        g = g32.double().numpy()
        m0, v0, p0 = pre["m"].double().numpy(), pre["v"].double().numpy(), pre["slab"].double().numpy()
        p_o, m_o, v_o = EO.adam(p0, g, m0, v0, t, lr, b1, b2)
        # fp32 error of the kernel: m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g^2 round three times (<= 2e-7 of the
        # terms' magnitude; for m the terms may cancel, so the bound is on the terms, not on the result); the new parameter
        # rounds once to the fp32 grid of p (a few ulps) and carries the update's own relative error (lr / bc1, powf,
        # sqrtf, the division: a few 1e-7 of an update that is at most ~2 lr), inside 1e-5 lr.  1e-37: fp32 denormals.
        tiny = 1e-37
        _within("adam exp_avg", np.abs(post["m"].double().numpy() - m_o),
                1e-6 * (b1 * np.abs(m0) + (1 - b1) * np.abs(g)) + tiny, tag + " exp_avg")
        _within("adam exp_avg_sq", np.abs(post["v"].double().numpy() - v_o), 1e-6 * np.abs(v_o) + tiny, tag + " exp_avg_sq")
        ulp = np.spacing(np.maximum(np.abs(p0), np.abs(p_o)).astype(np.float32)).astype(np.float64)
        _within("adam parameter", np.abs(post["slab"].double().numpy() - p_o), 4 * ulp + 1e-5 * lr, tag + " parameter")

    def check_offsets(self, n_sub):
        """the launches of every sub-step, in order, with their offsets relative to the iteration's block"""
        want = {"D": [("encoder_fwd_raw", EO.G_ENC), ("head_fwd_raw", EO.G_HEAD),        # G(partner), eval
                      ("encoder_fwd_raw", EO.D_ENC), ("head_fwd_raw", EO.D_HEAD),        # D(who) on [real | fake]
                      ("head_bwd_raw", EO.D_HEAD), ("encoder_bwd_raw", EO.D_ENC)],
                "G": [("encoder_fwd_raw", EO.G_ENC), ("head_fwd_raw", EO.G_HEAD),        # G(who), train
                      ("encoder_fwd_raw", EO.D_ENC), ("head_fwd_raw", EO.D_HEAD),        # frozen D(partner), eval
                      ("head_bwd_raw", EO.D_HEAD), ("encoder_bwd_raw", EO.D_ENC),
                      ("head_bwd_raw", EO.G_HEAD), ("encoder_bwd_raw", EO.G_ENC)]}
        its = sorted(self.base)
        for it in its:
            b = self.base[it]
            fwd = []
            for i, (kind, _, _) in enumerate(self.eng.schedule):
                got = self.launches[(it, i)]
                assert [(n, a - b - 4 * i) for n, a in got] == want[kind], (it, i, kind, b, got)
                fwd += [a for n, a in got if n.endswith("fwd_raw")]
            assert sorted(fwd) == list(range(b, b + 4 * n_sub)), (it, b, sorted(fwd))      # 4n distinct offsets
        for a_, b_ in zip(its, its[1:]):
            assert self.base[b_] >= self.base[a_] + 4 * n_sub, self.base       # blocks of iterations do not overlap


def _batch(din, S, B):
    return {k: torch.from_numpy(F_.formula_input("eng-train-oracle." + k, S, B, d, pad_from=max(1, S - 3))).cuda()
            for k, d in din.items()}


def _run(monkeypatch, shapes, compare, meld=False):
    from gan_ffn_amd import engine, ops
    assert engine.ADDS_PER_SUBSTEP == EO.ADDS_PER_SUBSTEP
    monkeypatch.setenv("GANFFN_ADAM_PARTS", "0")
    gens, discs = _networks(*((MELD_GEN, MELD_DISC) if meld else (GEN, DISC)))
    templates = {(g_, k): {n: v.clone() for n, v in m.state_dict().items() if n.startswith("encoder_layer.")}
                 for g_, grp in (("G", gens), ("D", discs)) for k, m in grp.items()}
    ops.manual_seed(SEED)
    eng = engine.GanEngine(gens, discs, n_streams=1)
    assert eng.schedule == (engine.SCHEDULE_BIMODAL if meld else engine.SCHEDULE)
    for st in list(eng.G.values()) + list(eng.D.values()):
        assert (st.p_pe, st.p_enc, st.p_head) == (0.2, 0.1, 0.2)
    n_sub = len(eng.schedule)
    cmp = {(it, i) for it, subs in compare.items() for i in (range(n_sub) if subs == "all" else subs)}
    h = _Harness(eng, cmp, monkeypatch)
    for it, (S, B) in enumerate(shapes):
        h.it = it
        eng.iteration(_batch(MELD_DIN if meld else DIN, S, B))
    torch.cuda.synchronize()
    assert h.compared == len(cmp)
    h.check_offsets(n_sub)
    # the template layer (model.py:1210) is not in the slab and nothing trains it
    for (g_, k), sd in templates.items():
        now = (gens if g_ == "G" else discs)[k].state_dict()
        for n, v in sd.items():
            assert torch.equal(now[n], v), (g_, k, n)
    return eng


# Shapes, each for a reason.  Sub-steps of the IEMOCAP schedule (engine.SCHEDULE): 0 D_v|G_a, 1 G_a|D_v, 2 D_v|G_t, 3 G_t|D_v,
# 4 D_t|G_a, 5 G_a|D_t, 6 D_a|G_t, 7 G_t|D_a, 8 D_t|G_v, 9 G_v|D_t, 10 D_a|G_v, 11 G_v|D_a.
CASES = {
    # small launches: the attention kernels hand their keep words from forward to backward (B * H <= 384); two iterations,
    # so every network reaches Adam step 3 or 4 and the bias corrections are exercised.  (7, 2) also gives ragged token
    # chunks: the discriminators' [real | fake] passes are 28 tokens
    "7x2_all": ([(7, 2), (7, 2)], {0: "all", 1: "all"}),
    "12x4_all": ([(12, 4), (12, 4)], {0: "all", 1: "all"}),
    # the generators' passes have S * B % 64 == 32 (160 tokens): the clamped last row tile of the linear2 dgrad (see
    # tests/test_hip_modules.py::test_train_mode_matches_oracle_with_same_masks); every G sub-step, the 512-wide one included
    "5x32_gen": ([(5, 32)], {0: [1, 3, 5, 7, 9, 11]}),
    # discriminator passes with S * 2B % 32 != 0 (78 tokens): ragged token chunks, every D sub-step
    "13x3_disc": ([(13, 3)], {0: [0, 2, 4, 6, 8, 10]}),
    # the d = 100 discriminators' backward runs two token chunks (640 tokens)
    "40x8": ([(40, 8)], {0: [4, 5, 6, 7]}),
    # the headline shape: the weight-resident K = 100 kernels, three token chunks, attention recomputing its masks from
    # Philox; the text / acoustic sub-steps only (the fp64 oracle runs on the host)
    "94x32": ([(94, 32)], {0: [4, 5, 6, 7]}),
    # passes resized inside capacity (_Pass.resize): the short last batch of a real loader, after a full one
    "94x32_then_23x5": ([(94, 32), (23, 5)], {1: "all"}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_engine_train_substeps_match_fp64_oracle(case, monkeypatch):
    shapes, compare = CASES[case]
    eng = _run(monkeypatch, shapes, compare)
    if case == "94x32_then_23x5":
        assert (eng._alloc_S, eng._alloc_B) == (94, 32) and eng._shape == (23, 5)


# The MELD-dimension bi-modal schedule (engine.SCHEDULE_BIMODAL: 0 D_t|G_a, 1 G_a|D_t, 2 D_a|G_t, 3 G_t|D_a; generators
# 600 / 300 wide, discriminators with a 600 / 300 -> 100 `object` layer): tests/test_hip_meld.py compares its iteration
# with dropout off and the first updates by sign only.
@pytest.mark.parametrize("shapes,compare", [([(9, 2), (9, 2)], {0: "all", 1: "all"}), ([(33, 32)], {0: [0, 1]})],
                         ids=["9x2_all", "33x32_first_pair"])
def test_bimodal_engine_train_substeps_match_fp64_oracle(shapes, compare, monkeypatch):
    _run(monkeypatch, shapes, compare, meld=True)
