"""GanEngine(causal=True) on the GPU, from the kernels up: the generators never look ahead, the discriminators still do.
  1. ganffn_encoder_fwd_pair_mask with GANFFN_ATTN_CAUSAL against the two ganffn_encoder_fwd_mask calls it replaces, bit for bit
     (eval output, train output, the whole saved block), without lengths and with ragged ones; flags = 0 has
     ganffn_encoder_fwd_pair_len's bits; an unknown flag bit is refused and writes nothing.  Shapes (S, B): those of
     tests/test_hip_gen_pair.py (S = 7, 9, 16: one 16-row tile, partial and exact; S = 94: six tiles, the cut form) and (33, 5)
     (three tiles, whole workgroups, two skipped tiles), (50, 2) (four tiles, the cut form; head_dim 64 past S = 48 on the 32-row
     kernel);
  2. ganffn_encoder_bwd_parts_mask + ganffn_adam_step_parts against ganffn_encoder_bwd_mask + ganffn_adam_step, bit for bit;
  3. the engine's train-mode sub-steps against the fp64 restatement with causal generators and bidirectional discriminators
     (tests/gan_causal_oracle.py) on the engine's own Philox masks and ReLU patterns, with the harness and the bounds of
     tests/test_hip_engine_train_oracle.py unchanged: outputs 1e-4 of scale, loss 2e-5 relative, every gradient element 1e-3 of
     its tensor's scale with no outliers, Adam as there.  Networks: the formula networks with the discriminators' fc weights
     times FC_SHARPEN = 1.5 (tests/test_hip_gan_mask_padding.py says why that factor).  Each compared sub-step first shows, on the
     oracle alone, that the BIDIRECTIONAL restatement of the same sub-step is more than 10x the bound away in the generator
     output involved and in the most separated gradient tensor.  A discriminator answers near 0.5, so the losses of the two
     restatements are close in the discriminator sub-steps (from 182x down to less than once the bound with these batches, on the
     CPU): the loss is held to its bound and its gap is printed, it is not part of the condition.  With mask_padding the
     generator outputs are compared over the real utterances, as in tests/test_hip_gan_mask_padding.py;
  4. a spy on the four encoder calls of ops over one iteration: every call on a generator's slab carries causal=True, every call
     on a discriminator's slab causal=False;
  5. bit equalities between launch shapes of the same causal step: paired and unpaired generator forwards, unreduced and reduced
     weight gradients, three streams and one, graph replay and eager launches — and the same with mask_padding;
     and a one-rank process group (the in-line all-reduce) keeps every flag and has the bits of the reduced step;
  6. causal=False is the default engine bit for bit, causal=True is another step; train_GAN(causal=True) and
     run_training(causal_gan=...).  run_training reads a corpus from disk, so only its signature is checked here: that
     train_GAN receives the flag is one line of gan_ffn_amd/artifacts.py, not run by this file."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import engine_oracle as EO
import gan_causal_oracle as GC
import gan_mask_oracle as GM
import test_hip_engine_train_oracle as TO
import test_hip_gan_mask_padding as MP
from key_len_oracle import valid_rows
from test_hip_classifier_engines_train_oracle import _batch
from test_hip_engine import build_all
from test_hip_gen_pair import SHAPES, _case, pair_cases
from util import DIN

pytestmark = pytest.mark.gpu

SEED = TO.SEED
MODS = MP.MODS
RAGGED_33 = [33, 1, 20, 7, 12]
_kl, _bits, _ragged = MP._kl, MP._bits, MP._ragged


# ================================================================================================================
# 1. the two-segment forward under the causal mask
# ================================================================================================================
def _pair_buffers(cfg, S, B, E):
    from gan_ffn_amd import ops
    f32 = dict(device="cuda", dtype=torch.float32)
    n_saved, _ = ops.enc_sizes(cfg)
    return (torch.zeros(S * B * E, **f32), torch.zeros(S * B * E, **f32), torch.full((n_saved,), -7.0, **f32),
            torch.zeros(ops.encoder_fwd_pair_workspace_floats(cfg), **f32))


@pytest.mark.parametrize("S,B,E,H", pair_cases(SHAPES + [(33, 5), (50, 2)]))
def test_causal_pair_pass_equals_the_two_causal_single_passes(S, B, E, H):
    from gan_ffn_amd import ops
    cfg, cfg_eval, params, x, pe = _case(S, B, E, H)
    n_saved, n_ws = ops.enc_sizes(cfg)
    ops.manual_seed(4321)
    rng, add = ops.DeviceRng.get("cuda").state, 17
    f32 = dict(device="cuda", dtype=torch.float32)
    assert ops.encoder_fwd_pair_supported(cfg)
    lens = _ragged(S, B)
    assert S in lens and 1 in lens

    def single(kl):
        out_e, out_t = torch.zeros(S * B * E, **f32), torch.zeros(S * B * E, **f32)
        saved, ws = torch.full((n_saved,), -7.0, **f32), torch.zeros(n_ws, **f32)
        ops.encoder_fwd_raw(cfg_eval, x, pe, params, out_e, None, ws, rng, add, key_len=kl, causal=True)
        ops.encoder_fwd_raw(cfg, x, pe, params, out_t, saved, ws, rng, add, key_len=kl, causal=True)
        return out_e, out_t, saved

    def pair(kl, causal, through_len_entry=False):
        p_e, p_t, p_saved, p_ws = _pair_buffers(cfg, S, B, E)
        if through_len_entry:
            ops._lib.call("ganffn_encoder_fwd_pair_len", C.byref(cfg), ops._ptr(kl), ops._ptr(x), ops._ptr(pe), ops._ptr(params),
                          ops._ptr(p_e), ops._ptr(p_t), ops._ptr(p_saved), ops._ptr(p_ws), ops._ptr(rng), C.c_uint64(add), ops._stream())
        else:
            ops.encoder_fwd_pair_raw(cfg, x, pe, params, p_e, p_t, p_saved, p_ws, rng, add, key_len=kl, causal=causal)
        return p_e, p_t, p_saved

    names = ("eval output", "train output", "saved block")
    for kl in (None, _kl(lens)):
        tag = "key_len=None" if kl is None else "ragged"
        want, got = single(kl), pair(kl, True)
        plain, old = pair(kl, False), pair(kl, False, through_len_entry=True)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in want[:2]) and not torch.equal(want[0], want[1]), tag
        for name, a, b in zip(names, got, want):
            assert torch.equal(_bits(a), _bits(b)), (tag, name)
        # the mask was used: the causal pair is another function than the pair without it (S = 1 would be the same one)
        assert not torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1]), tag
        # flags = 0 through the new entry point: ganffn_encoder_fwd_pair_len's bits
        for name, a, b in zip(names, plain, old):
            assert torch.equal(_bits(a), _bits(b)), (tag, name)


@pytest.mark.parametrize("E,H", [(100, 10), (512, 8)])
def test_an_unknown_flag_bit_is_refused_and_nothing_is_written(E, H):
    from gan_ffn_amd import _lib, ops
    S, B = 9, 4
    cfg, _, params, x, pe = _case(S, B, E, H)
    ops.manual_seed(4321)
    rng = ops.DeviceRng.get("cuda").state
    for flags in (2, 3, 0x80000001):
        p_e, p_t, p_saved, p_ws = _pair_buffers(cfg, S, B, E)
        for t in (p_e, p_t, p_ws):
            t.fill_(-7.0)
        with pytest.raises(_lib.GanffnError, match="unknown flag bits"):
            _lib.call("ganffn_encoder_fwd_pair_mask", C.byref(cfg), None, C.c_uint32(flags), ops._ptr(x), ops._ptr(pe), ops._ptr(params),
                      ops._ptr(p_e), ops._ptr(p_t), ops._ptr(p_saved), ops._ptr(p_ws), ops._ptr(rng), C.c_uint64(17), ops._stream())
        torch.cuda.synchronize()
        for t in (p_e, p_t, p_saved, p_ws):
            assert bool((t == -7.0).all()), flags


# ================================================================================================================
# 2. unreduced weight gradients under the causal mask
# ================================================================================================================
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("S,B,lens", [(33, 5, RAGGED_33), (64, 8, [64, 1, 63, 17, 33, 5, 48, 2])], ids=["33x5", "64x8"])
def test_causal_parts_backward_equals_the_causal_reduced_backward(S, B, lens, ragged):
    from gan_ffn_amd import ops
    lib = ops._lib.load()
    E, H, L = 100, 10, 2
    cfg, _, params, x, pe = _case(S, B, E, H, L)
    assert ops.encoder_bwd_parts_supported(cfg)
    per, _ = ops.layer_layout(E)
    n = L * per
    covered = int(lib.ganffn_encoder_bwd_parts_covered(E, 2048))
    n_saved, n_ws = ops.enc_sizes(cfg)
    g = torch.Generator().manual_seed(7 * S + B)
    dout = torch.randn(S, B, E, generator=g).cuda()
    m0, v0 = (torch.randn(n, generator=g) * 0.01).cuda(), (torch.rand(n, generator=g) * 1e-4).cuda()
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    f32 = dict(device="cuda", dtype=torch.float32)
    kl = _kl(lens) if ragged else None

    def run(path, causal):
        out, saved, ws = torch.zeros(S * B * E, **f32), torch.zeros(n_saved, **f32), torch.zeros(n_ws, **f32)
        ops.encoder_fwd_raw(cfg, x, pe, params, out, saved, ws, rng, 5, key_len=kl, causal=causal)
        p, m, v = params.clone(), m0.clone(), v0.clone()
        step = torch.tensor([3], dtype=torch.int32, device="cuda")
        dx = dout.clone()
        ws.fill_(float("nan"))
        n_parts = 1
        if path == "parts":
            grad = torch.full((n,), float("nan"), **f32)
            parts, stride, n_parts, off = ops.encoder_bwd_parts_raw(cfg, dx, p, grad, saved, ws, rng, 5, True, key_len=kl, causal=causal)
            ops.adam_step_parts_raw(p, grad, m, v, step, n, 1e-4, 0.5, 0.6, parts, stride, n_parts, n, per, covered)
        else:
            grad = torch.zeros(n, **f32)
            ops.encoder_bwd_raw(cfg, 0, L, dx, p, grad, saved, ws, rng, 5, True, key_len=kl, causal=causal)
            ops.adam_step_raw(p, grad, m, v, step, n, 1e-4, 0.5, 0.6)
        torch.cuda.synchronize()
        return dict(p=p, m=m, v=v, dx=dx, step=step), n_parts

    a, n_parts = run("parts", True)
    b, _ = run("reduced", True)
    plain, _ = run("parts", False)
    print("T = %d: %d weight-gradient chunks" % (S * B, n_parts))
    assert n_parts > 1 or S * B < 512
    for k in a:
        assert bool(torch.isfinite(a[k].float()).all()), k
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert int(a["step"]) == 4 and not torch.equal(a["p"], params)
    assert not torch.equal(a["m"], plain["m"]) and not torch.equal(a["dx"], plain["dx"])      # the mask was used


# ================================================================================================================
# 3. the engine's causal sub-steps against the fp64 oracle
# ================================================================================================================
class _CausalHarness(TO._Harness):
    """the harness of the bidirectional test with the causal restatement in place of it, and the condition on the inputs: the
    bidirectional restatement of the same sub-step is further away than 10x the bounds.  lens: the key lengths of a
    mask_padding engine, or None"""

    def __init__(self, eng, compare, monkeypatch, lens=None):
        super().__init__(eng, compare, monkeypatch)
        self.lens = None if lens is None else list(lens)
        self.gaps = []

    def _rows(self, t):
        """the rows a generator's output is compared over: all of them, or with lengths the real utterances"""
        return t if self.lens is None else t[valid_rows(t.shape[0], self.lens)]

    def _bidirectional(self, kind, *a, **kw):
        """the same sub-step with generators that look ahead: engine_oracle's, or gan_mask_oracle's with the lengths"""
        if self.lens is None:
            return (EO.disc_substep if kind == "D" else EO.gen_substep)(*a, **kw)
        return (GM.disc_substep if kind == "D" else GM.gen_substep)(*a, self.lens, **kw)

    def _discriminates(self, tag, what, out, out_plain, res, plain):
        go = float((self._rows(out) - self._rows(out_plain)).abs().max() / self._rows(out).abs().max())
        gg = max(float((res["grads"][k] - plain["grads"][k]).abs().max() / res["grads"][k].abs().max().clamp_min(1e-300))
                 for k in res["grads"])
        gl = abs(res["loss"] - plain["loss"]) / abs(res["loss"])
        self.gaps.append((go / 1e-4, gg / 1e-3, gl / 2e-5))
        print("%s: causal vs bidirectional oracle, %s %.3g of scale = %.0f x bound, most separated gradient tensor %.3g of scale = "
              "%.0f x bound; loss %.3g relative = %.0f x bound (printed, not part of the condition)" %
              (tag, what, go, go / 1e-4, gg, gg / 1e-3, gl, gl / 2e-5))
        assert go > 10 * 1e-4 and gg > 10 * 1e-3, (tag, go, gg)

    def _close_rows(self, kind, got, want, label):
        TO._close(kind, self._rows(got).numpy(), self._rows(want).numpy(), 1e-4, 0.0, label)

    def _check_disc(self, st, gst, xr, xp, b, i, pre, pre_p, post, loss, masks, fake, lr):
        tag = "it%d sub-step %d D %s" % (self.it, i, st.m.__class__.__name__)
        D = EO.Net.from_state(st, pre["slab"])
        G = EO.Net.from_state(gst, pre_p["slab"], requires_grad=False)
        fake_o = GC.generator_eval(G, xp, SEED, b, i, self.lens)
        self._close_rows("fake (G eval)", fake, fake_o, tag + " fake")
        res = GC.disc_substep(D, G, xr, xp, SEED, b, i, self.lens, fake=fake, relu_masks=masks)
        plain = self._bidirectional("D", D, G, xr, xp, SEED, b, i)
        self._discriminates(tag, "fake", fake_o, plain["fake"], res, plain)
        self._check_common(st, tag, res, pre, post, loss, lr)

    def _check_gen(self, st, dst, x, b, i, pre, pre_p, post, loss, masks_g, masks_d, out, lr):
        tag = "it%d sub-step %d G %s" % (self.it, i, st.m.__class__.__name__)
        G = EO.Net.from_state(st, pre["slab"])
        D = EO.Net.from_state(dst, pre_p["slab"], requires_grad=False)
        res = GC.gen_substep(G, D, x, SEED, b, i, self.lens, masks_g, masks_d)
        plain = self._bidirectional("G", G, D, x, SEED, b, i)
        self._discriminates(tag, "G train output", res["out"], plain["out"], res, plain)
        self._close_rows("G train output", out, res["out"], tag + " output")
        self._check_common(st, tag, res, pre, post, loss, lr)


# sub-steps compared: all 12 at (7, 2) and, with mask_padding, at the ragged (33, 5); at (50, 2) those that run the 512-wide
# generator, the one network S = 50 moves to the 32-row attention kernel
ORACLE_CASES = {"7x2": (7, 2, None, "all"), "50x2": (50, 2, None, [8, 9, 10, 11]), "33x5_mask_padding": (33, 5, RAGGED_33, "all")}


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_causal_engine_train_substeps_match_fp64_oracle(case, monkeypatch):
    """Largest error / tolerance per check on an MI355X when the test was added ((7, 2) / (50, 2) / (33, 5) with mask_padding):
    fake 0.037 / 0.054 / 0.064, G train output 0.027 / 0.045 / 0.025, loss 0.015 / 0.010 / 0.010, gradient 0.049 / 0.081 / 0.040,
    Adam moments and parameter <= 0.22.  Smallest causal / bidirectional gap over the compared sub-steps: generator output 59 / 45 /
    215 x its bound (the 512-wide generator's sub-steps are the closest), gradient 236 / 128 / 149 x its bound; the loss gap falls to
    0 x its bound in discriminator sub-steps, which is why it is not part of the condition.  The same gaps from the initial
    parameters on the CPU, before the GPU run: output >= 45 x, gradient >= 77 x in every compared sub-step."""
    from gan_ffn_amd import engine, ops
    S, B, lens, subs = ORACLE_CASES[case]
    monkeypatch.setenv("GANFFN_ADAM_PARTS", "0")           # the summed gradient stays in net.grad (case 5 covers the other form)
    monkeypatch.setattr(TO, "WORST", {})
    gens, discs = MP._sharp_networks()
    ops.manual_seed(SEED)
    eng = engine.GanEngine(gens, discs, n_streams=1, mask_padding=lens is not None, causal=True)
    cmp = {(0, i) for i in (range(12) if subs == "all" else subs)}
    h = _CausalHarness(eng, cmp, monkeypatch, lens)
    if lens is None:
        batch = TO._batch(DIN, S, B)
    else:
        batch = _batch(S, B, 31 * S + B, lens=lens)
        batch = {k: batch[k] for k in MODS + ("umask",)}
    eng.iteration(batch)
    torch.cuda.synchronize()
    assert h.compared == len(cmp) == len(h.gaps)
    h.check_offsets(12)
    print("causal engine oracle %s, largest error / tolerance per check: %s; smallest causal / bidirectional gap: generator output "
          "%.0f x bound, gradient %.0f x bound, loss %.0f x bound" %
          (case, ", ".join("%s %.3g" % kv for kv in sorted(TO.WORST.items())), min(g[0] for g in h.gaps), min(g[1] for g in h.gaps),
           min(g[2] for g in h.gaps)))


# ================================================================================================================
# 4. which calls carry the flag
# ================================================================================================================
@pytest.mark.parametrize("mask_padding", [False, True])
def test_generator_calls_carry_the_flag_and_discriminator_calls_do_not(mask_padding, monkeypatch):
    from gan_ffn_amd import engine, ops
    monkeypatch.delenv("GANFFN_GEN_PAIR", raising=False)
    monkeypatch.delenv("GANFFN_ADAM_PARTS", raising=False)
    gens, discs = build_all(zero_dropout=False)
    ops.manual_seed(SEED)
    eng = engine.GanEngine(gens, discs, n_streams=3, mask_padding=mask_padding, causal=True)
    owner = {st.slab.data_ptr(): "G" for st in eng.G.values()}
    owner.update({st.slab.data_ptr(): "D" for st in eng.D.values()})
    assert len(owner) == 6
    seen = []
    # position of the parameter slab in each call
    for name, pos in (("encoder_fwd_raw", 3), ("encoder_fwd_pair_raw", 3), ("encoder_bwd_raw", 4), ("encoder_bwd_parts_raw", 2)):
        def spy(*a, _fn=getattr(ops, name), _name=name, _pos=pos, **kw):
            seen.append((_name, owner[a[_pos].data_ptr()], kw.get("causal")))
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    eng.iteration(MP._gan_batch(33, 5, RAGGED_33))
    eng.synchronize()
    torch.cuda.synchronize()
    for name, who, causal in seen:
        assert causal is (who == "G"), (name, who, causal)
    # every form was reached, by the networks that use it: the paired forward and the parts backward included
    kinds = {(n, w) for n, w, _ in seen}
    assert kinds >= {("encoder_fwd_raw", "G"), ("encoder_fwd_raw", "D"), ("encoder_fwd_pair_raw", "G"), ("encoder_bwd_raw", "G"),
                     ("encoder_bwd_raw", "D"), ("encoder_bwd_parts_raw", "G"), ("encoder_bwd_parts_raw", "D")}, kinds
    assert ("encoder_fwd_pair_raw", "D") not in kinds


# ================================================================================================================
# 5. - 6. whole iterations
# ================================================================================================================
def _iterate(batches, causal=True, mask_padding=False, n_streams=1, use_graph=False, default_engine=False):
    """a fresh engine over fresh formula networks, the same seed and dropout offsets every time -> (losses of every iteration,
    the six parameter slabs with their moments and step counts).  default_engine: built without naming the option at all"""
    from gan_ffn_amd import engine, ops
    gens, discs = build_all(zero_dropout=False)
    ops.manual_seed(SEED)
    kw = {} if default_engine else dict(causal=causal)
    eng = engine.GanEngine(gens, discs, n_streams=n_streams, use_graph=use_graph, mask_padding=mask_padding, **kw)
    assert eng.n_streams == n_streams and eng.use_graph == use_graph and eng.causal == (causal and not default_engine)
    losses = []
    for b in batches:
        ls = eng.iteration(b)
        eng.synchronize()
        losses.append(ls.clone())
    torch.cuda.synchronize()
    return torch.stack(losses), MP._state(eng)


def _shape_batch(S, B, mask_padding):
    return MP._gan_batch(S, B, RAGGED_33 if (S, B) == (33, 5) else [S] + [3] * (B - 1))


@pytest.mark.parametrize("S,B,mask_padding", [(33, 5, False), (50, 2, False), (33, 5, True)], ids=["33x5", "50x2", "33x5_mask_padding"])
def test_paired_generator_forwards_equal_unpaired_under_the_causal_mask(S, B, mask_padding, monkeypatch):
    batch = _shape_batch(S, B, mask_padding)
    res = {}
    for mode in ("0", "1", "all"):
        monkeypatch.setenv("GANFFN_GEN_PAIR", mode)
        res[mode] = _iterate([batch, batch], mask_padding=mask_padding)
    MP._same(res["1"], res["0"])
    MP._same(res["all"], res["0"])


@pytest.mark.parametrize("mask_padding", [False, True], ids=["plain", "mask_padding"])
def test_unreduced_weight_gradients_equal_reduced_under_the_causal_mask(mask_padding, monkeypatch):
    batch = _shape_batch(33, 5, mask_padding)
    monkeypatch.setenv("GANFFN_ADAM_PARTS", "1")
    parts = _iterate([batch, batch], mask_padding=mask_padding)
    monkeypatch.setenv("GANFFN_ADAM_PARTS", "0")
    MP._same(parts, _iterate([batch, batch], mask_padding=mask_padding))


@pytest.mark.parametrize("mask_padding", [False, True], ids=["plain", "mask_padding"])
def test_three_streams_equal_one_under_the_causal_mask(mask_padding, monkeypatch):
    """(nothing set: three streams pair the 512-wide generator's forwards, one stream pairs none)"""
    monkeypatch.delenv("GANFFN_GEN_PAIR", raising=False)
    batch = _shape_batch(33, 5, mask_padding)
    MP._same(_iterate([batch, batch], mask_padding=mask_padding, n_streams=3), _iterate([batch, batch], mask_padding=mask_padding))


@pytest.mark.parametrize("S,B,mask_padding", [(9, 3, False), (33, 5, True)], ids=["9x3", "33x5_mask_padding"])
def test_graph_replay_equals_eager_under_the_causal_mask(S, B, mask_padding):
    """replay k is execution k + 1 of the iteration (tests/test_hip_engine.py::test_graph_replay_matches_eager): graph mode over
    [b1, b2] executes b1 (warm-up), b1 (first replay), b2 (second replay)"""
    if mask_padding:
        b1, b2 = MP._gan_batch(S, B, RAGGED_33, seed=1), MP._gan_batch(S, B, [2, 33, 7, 19, 1], seed=2)
    else:
        b1, b2 = MP._gan_batch(S, B, [9, 1, 4], seed=1), MP._gan_batch(S, B, [2, 9, 7], seed=2)
    replay = _iterate([b1, b2], mask_padding=mask_padding, use_graph=True)
    eager = _iterate([b1, b1, b2], mask_padding=mask_padding)
    assert torch.equal(replay[0][1], eager[0][2]) and torch.equal(replay[0][0], eager[0][1])
    for k in replay[1]:
        assert torch.equal(replay[1][k], eager[1][k]), k


@pytest.mark.parametrize("n_streams", [1, 3])
def test_a_process_group_keeps_the_flags_and_the_bits(n_streams, monkeypatch):
    """a one-rank gloo group made in this process (the all-reduce is then the identity and Adam divides by 1), the default in-line
    all-reduce: with it the engine leaves the unreduced path for the whole reduced backward, every one of those calls carries the
    network's flag, and the step has the bits of the reduced single-GPU step.  (The bucketed mode issues the same
    ops.encoder_bwd_raw call per layer range, with the same flag argument; it is not run here.)"""
    import torch.distributed as dist
    from gan_ffn_amd import engine, ops
    monkeypatch.delenv("GANFFN_DP_MODE", raising=False)
    monkeypatch.delenv("GANFFN_GEN_PAIR", raising=False)
    monkeypatch.delenv("GANFFN_COMM_PER_STREAM", raising=False)
    batch = MP._gan_batch(33, 5, RAGGED_33)
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        gens, discs = build_all(zero_dropout=False)
        ops.manual_seed(SEED)
        eng = engine.GanEngine(gens, discs, n_streams=n_streams, process_group=dist.group.WORLD, causal=True)
        owner = {st.slab.data_ptr(): "G" for st in eng.G.values()}
        owner.update({st.slab.data_ptr(): "D" for st in eng.D.values()})
        seen = []
        real_bwd = ops.encoder_bwd_raw

        def spy(*a, **kw):
            seen.append((owner[a[4].data_ptr()], kw.get("causal"), (a[1], a[2])))
            return real_bwd(*a, **kw)
        monkeypatch.setattr(ops, "encoder_bwd_raw", spy)
        monkeypatch.setattr(ops, "encoder_bwd_parts_raw", lambda *a, **kw: pytest.fail("the unreduced path under a process group"))
        losses = []
        for _ in range(2):
            ls = eng.iteration(batch)
            eng.synchronize()
            losses.append(ls.clone())
        torch.cuda.synchronize()
        got = (torch.stack(losses), MP._state(eng))
    finally:
        dist.destroy_process_group()
    monkeypatch.undo()
    assert bool(torch.isfinite(got[0]).all())
    assert {w for w, _, _ in seen} == {"G", "D"} and all(c is (w == "G") for w, c, _ in seen), seen
    monkeypatch.setenv("GANFFN_ADAM_PARTS", "0")
    MP._same(got, _iterate([batch, batch], n_streams=n_streams))


def test_causal_false_is_the_default_engine_and_causal_true_is_another_step():
    batch = MP._gan_batch(7, 2, [7, 5])
    default = _iterate([batch, batch], default_engine=True)
    MP._same(_iterate([batch, batch], causal=False), default)
    causal = _iterate([batch, batch], causal=True)
    assert bool(torch.isfinite(causal[0]).all())
    assert not bool((causal[0] == default[0]).any())        # all 12 losses of both iterations: a generator is in each sub-step
    assert not any(torch.equal(causal[1][k], default[1][k]) for k in causal[1] if k[2] != "step")


def test_training_entry_points_take_the_flag():
    from gan_ffn_amd import artifacts, engine
    gens, discs = build_all(zero_dropout=False)
    batch = MP._gan_batch(7, 2, [7, 5])
    rows = engine.train_GAN(gens, discs, [batch, batch], epochs=2, n_streams=1, causal=True)
    assert len(rows) == 2 and all(np.isfinite(v) for r in rows for v in r.values())
    assert inspect.signature(engine.train_GAN).parameters["causal"].default is False
    assert inspect.signature(engine.GanEngine.__init__).parameters["causal"].default is False
    sig = inspect.signature(artifacts.run_training).parameters
    assert sig["causal_gan"].default is False and sig["causal"].default is False and sig["mask_padding_gan"].default is False
