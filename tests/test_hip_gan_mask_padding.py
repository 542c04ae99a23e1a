"""GanEngine(mask_padding=True) on the GPU, from the kernels up:
  1. ganffn_encoder_fwd_pair_len against the two ganffn_encoder_fwd_len calls it replaces, bit for bit;
  2. ganffn_encoder_bwd_parts_len + ganffn_adam_step_parts against ganffn_encoder_bwd_len + ganffn_adam_step, bit for bit;
  3. ganffn_bce_len_fwd / _bwd against an fp64 restatement (stock binary_cross_entropy over the valid positions), at the bounds
     tests/test_hip_bce_adam.py holds ganffn_bce2 to, and against ganffn_bce2 itself at full lengths, bit for bit;
  4. the engine's train-mode sub-steps against the fp64 restatement with masked attention and masked losses
     (tests/gan_mask_oracle.py) on the engine's own Philox masks and ReLU patterns, with the harness and the bounds of
     tests/test_hip_engine_train_oracle.py unchanged: outputs 1e-4 of scale, loss 2e-5 relative, every gradient element 1e-3 of
     its tensor's scale with no outliers, Adam as there.  The discriminators' fc1 / fc2 / fc3 weights are the formula weights
     times FC_SHARPEN = 1.5 (see there for why not more): with the formula weights every discriminator answers about 0.5
     everywhere and the masked and the unmasked loss are 3.6e-5 to 5e-4 apart (relative), too close to the 2e-5 bound to tell an
     engine that ignored the lengths from one that did not.  Each compared sub-step first shows, on the oracle alone, that its
     inputs tell the two functions apart by more than 10x the bounds;
  5. finite values at padded positions of the batch change no bit of a whole iteration (and do, without mask_padding);
  6. five more rows of padding change the losses by rounding only;
  7. bit equalities between launch shapes that compute the same step: full lengths and mask_padding=False, three streams and
     one, paired and unpaired generator forwards, unreduced and reduced weight gradients, graph replay and eager launches;
  8. a batch without umask is refused.
Padded rows of a generator's output (case 4): the outputs are held to 1e-4 of scale over the real utterances.  Over ALL rows the
(33, 5) case reads 1.08 of that bound at ONE padded token (sub-step 11, the 512-wide generator, row 22 of the length-1 dialogue: 3
of 16500 elements; every other sub-step and shape <= 0.061) — and the engine WITHOUT mask_padding, on the same networks, batch, seed
and harness against the unmasked restatement, reads 1.44 of the bound at the same token (16 elements, and 1.24 of the gradient
bound on one tensor): an fp32 property of that all-zero input row under that sub-step's dropout masks, older than this option and
smaller with it.  Nothing reads a generator's output at a padded row when the option is on, so the bound is not widened: the
padded rows are printed instead of bounded.  Gradients, Adam and losses are compared in full.
Ragged shapes: those of tests/test_hip_key_len_engines.py, and (50, 2, [50, 3]), which takes the 512-wide generator (head_dim 64)
past S = 48 onto the 32-row attention kernel."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import engine_oracle as EO
import gan_mask_oracle as GM
import test_hip_engine_train_oracle as TO
from bce_cases import UNDERFLOW
from key_len_oracle import masked_attention, valid_rows
from test_hip_classifier_engines_train_oracle import _batch
from test_hip_engine import build_all
from test_hip_gen_pair import SHAPES, _case, pair_cases
from util import DISC, GEN

pytestmark = pytest.mark.gpu

SEED = TO.SEED
ENGINE_SHAPES = [(7, 2, [7, 1]), (33, 5, [33, 1, 20, 7, 12]), (50, 2, [50, 3])]
MODS = ("acoustic", "visual", "text")


def _kl(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def _ragged(S, B):
    """lengths with S and 1 among them, the rest no multiple of 4"""
    return ([S, 1] + [max(1, (S * (j + 2)) // (B + 1) | 1) for j in range(B - 2)])[:B]


def _bits(t):
    return t.view(torch.int32)


# ================================================================================================================
# 1. the two-segment forward with key lengths
# ================================================================================================================
@pytest.mark.parametrize("S,B,E,H", pair_cases(SHAPES + [(50, 2)]))
def test_pair_pass_with_key_lengths_equals_the_two_single_passes(S, B, E, H):
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
        ops.encoder_fwd_raw(cfg_eval, x, pe, params, out_e, None, ws, rng, add, key_len=kl)
        ops.encoder_fwd_raw(cfg, x, pe, params, out_t, saved, ws, rng, add, key_len=kl)
        return out_e, out_t, saved

    def pair(kl, through_len_entry=False):
        p_e, p_t = torch.zeros(S * B * E, **f32), torch.zeros(S * B * E, **f32)
        p_saved = torch.full((n_saved,), -7.0, **f32)
        p_ws = torch.zeros(ops.encoder_fwd_pair_workspace_floats(cfg), **f32)
        if through_len_entry:       # key_len == NULL handed to the new entry point itself
            ops._lib.call("ganffn_encoder_fwd_pair_len", C.byref(cfg), None, ops._ptr(x), ops._ptr(pe), ops._ptr(params), ops._ptr(p_e),
                          ops._ptr(p_t), ops._ptr(p_saved), ops._ptr(p_ws), ops._ptr(rng), C.c_uint64(add), ops._stream())
        else:
            ops.encoder_fwd_pair_raw(cfg, x, pe, params, p_e, p_t, p_saved, p_ws, rng, add, key_len=kl)
        return p_e, p_t, p_saved

    want, got = single(_kl(lens)), pair(_kl(lens))
    plain = pair(None)
    null, full = pair(None, through_len_entry=True), pair(_kl([S] * B))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in want[:2]) and not torch.equal(want[0], want[1])
    for name, a, b in zip(("eval output", "train output", "saved block"), got, want):
        assert torch.equal(_bits(a), _bits(b)), name
    # the lengths were used: the ragged pass is another function than the plain one
    assert not torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1])
    # key_len = NULL and full lengths: ganffn_encoder_fwd_pair's bits
    for other in (null, full):
        for name, a, b in zip(("eval output", "train output", "saved block"), other, plain):
            assert torch.equal(_bits(a), _bits(b)), name


# ================================================================================================================
# 2. unreduced weight gradients with key lengths
# ================================================================================================================
@pytest.mark.parametrize("S,B,lens", [(33, 5, [33, 1, 20, 7, 12]), (64, 8, [64, 1, 63, 17, 33, 5, 48, 2])], ids=["33x5", "64x8"])
def test_parts_backward_with_key_lengths_equals_the_reduced_backward(S, B, lens):
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

    def run(path, kl):
        out, saved, ws = torch.zeros(S * B * E, **f32), torch.zeros(n_saved, **f32), torch.zeros(n_ws, **f32)
        ops.encoder_fwd_raw(cfg, x, pe, params, out, saved, ws, rng, 5, key_len=kl)
        p, m, v = params.clone(), m0.clone(), v0.clone()
        step = torch.tensor([3], dtype=torch.int32, device="cuda")
        dx = dout.clone()
        ws.fill_(float("nan"))
        n_parts = 1
        if path == "parts":
            grad = torch.full((n,), float("nan"), **f32)
            parts, stride, n_parts, off = ops.encoder_bwd_parts_raw(cfg, dx, p, grad, saved, ws, rng, 5, True, key_len=kl)
            ops.adam_step_parts_raw(p, grad, m, v, step, n, 1e-4, 0.5, 0.6, parts, stride, n_parts, n, per, covered)
        else:
            grad = torch.zeros(n, **f32)
            ops.encoder_bwd_raw(cfg, 0, L, dx, p, grad, saved, ws, rng, 5, True, key_len=kl)
            ops.adam_step_raw(p, grad, m, v, step, n, 1e-4, 0.5, 0.6)
        torch.cuda.synchronize()
        return dict(p=p, m=m, v=v, dx=dx, step=step), n_parts

    a, n_parts = run("parts", _kl(lens))
    b, _ = run("reduced", _kl(lens))
    plain, _ = run("parts", None)
    print("T = %d: %d weight-gradient chunks" % (S * B, n_parts))
    assert n_parts > 1 or S * B < 512
    for k in a:
        assert bool(torch.isfinite(a[k].float()).all()), k
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert int(a["step"]) == 4 and not torch.equal(a["p"], params)
    assert not torch.equal(a["m"], plain["m"]) and not torch.equal(a["dx"], plain["dx"])      # the lengths were used


# ================================================================================================================
# 3. the BCE pair with lengths
# ================================================================================================================
def _bce_probs(S, Bt, lens_cols, seed):
    """seeded probabilities; exact 0 and 1 (the -100 log clamp, the 1e-12 clamp of the backward) planted inside the valid region
    and, where there is one, in the padded region"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(S, Bt, generator=g)
    valid = valid_rows(S, GM.clamp_lengths(lens_cols, S))
    vi, pi = valid.nonzero(), (~valid).nonzero()
    for (s, c), v in zip(vi[[0, len(vi) // 2, len(vi) - 1]].tolist(), (0.0, 1.0, 0.0)):
        p[s, c] = v
    if len(pi):
        for (s, c), v in zip(pi[[0, len(pi) - 1]].tolist(), (0.0, 1.0)):
            p[s, c] = v
    return p, valid


def _bce_len(lib, p_d, kl, n_len, ta, tb, S, Bt, split, scale):
    from gan_ffn_amd import ops
    loss, again = torch.full((1,), 0.25, device="cuda"), torch.full((1,), 0.25, device="cuda")
    for t in (loss, again):
        ops.bce_len_fwd_raw(p_d, kl, n_len, ta, tb, S, Bt, split, scale, t, False)
    acc = torch.full((1,), 0.25, device="cuda")
    ops.bce_len_fwd_raw(p_d, kl, n_len, ta, tb, S, Bt, split, scale, acc, True)
    d = torch.full((S * Bt,), float("nan"), device="cuda")
    ops.bce_len_bwd_raw(p_d, kl, n_len, ta, tb, S, Bt, split, scale, d)
    torch.cuda.synchronize()
    assert torch.equal(loss, again)                    # one workgroup, a fixed-order tree
    return loss, acc, d.view(S, Bt)


# (S, B, lengths): the engine shapes, and (94, 32): 6016 positions of a discriminator pass, past the 1024-thread stride
BCE_SHAPES = ENGINE_SHAPES + [(94, 32, [94, 1] + [3 * j + 2 for j in range(30)])]


@pytest.mark.parametrize("kind", ["disc", "gen"])
@pytest.mark.parametrize("S,B,lens", BCE_SHAPES, ids=["7x2", "33x5", "50x2", "94x32"])
def test_bce_with_lengths_matches_fp64_over_the_valid_positions(S, B, lens, kind):
    from gan_ffn_amd import _lib as lib
    Bt, split = (2 * B, B) if kind == "disc" else (B, B)
    cols = (lens + lens)[:Bt]
    p, valid = _bce_probs(S, Bt, cols, 100 * S + Bt)
    assert bool((p[valid] == 0).any()) and bool((p[valid] == 1).any())
    if not bool(valid.all()):
        assert bool((p[~valid] == 0).any()) and bool((p[~valid] == 1).any())
    p_d, kl = p.cuda(), _kl(lens)
    for (ta, tb), scale in (((1.0, 0.0), 1.0), ((0.9, 0.1), 0.5)):
        y = torch.where(torch.arange(Bt) < split, torch.tensor(float(np.float32(ta)), dtype=torch.float64),
                        torch.tensor(float(np.float32(tb)), dtype=torch.float64)).expand(S, Bt)
        p64 = p.double().requires_grad_(True)
        ref = F.binary_cross_entropy(p64, y, weight=valid.double(), reduction="sum") / float(int(valid.sum())) * scale
        (gref,) = torch.autograd.grad(ref, p64)
        ref = float(ref)
        assert abs(ref - scale * float(GM.masked_bce(p.double(), y, cols))) <= 1e-12 * abs(ref)       # the helper's restatement
        loss, acc, d = _bce_len(lib, p_d, kl, B, ta, tb, S, Bt, split, scale)
        tag = "%s (%d, %d) targets (%g, %g) scale %g" % (kind, S, Bt, ta, tb, scale)
        dh = d.cpu().double()
        nz = gref != 0
        worst = float(((dh - gref).abs()[nz] / gref.abs()[nz]).max())
        print("bce_len %s: loss %.9g, fp64 %.9g (rel %.3g); dprob largest elementwise relative error %.3g" %
              (tag, float(loss), ref, abs(float(loss) - ref) / abs(ref), worst))
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref), tag
        assert abs(float(acc) - (ref + 0.25)) <= 1e-5 * abs(ref + 0.25), tag
        assert bool(torch.isfinite(dh).all()), tag
        assert float((dh - gref).abs().max() / gref.abs().max()) < 1e-5, tag
        assert bool(((dh - gref).abs() <= 1e-5 * gref.abs() + UNDERFLOW).all()), tag
        # padded entries: written, and exactly +0.0
        assert bool((_bits(d.cpu())[~valid] == 0).all()), tag


@pytest.mark.parametrize("S,Bt,split,n_len", [(7, 4, 2, 2), (33, 10, 5, 5), (33, 5, 5, 5), (94, 64, 32, 32), (3, 512, 256, 256)])
def test_bce_with_null_or_full_lengths_is_bce2_and_bad_lengths_are_clamped(S, Bt, split, n_len):
    from gan_ffn_amd import _lib as lib, ops
    n = S * Bt
    p, _ = _bce_probs(S, Bt, [S] * Bt, n)
    p_d = p.cuda()
    for (ta, tb), scale in (((1.0, 0.0), 1.0), ((0.9, 0.1), 0.5)):
        want_l, want_d = torch.full((1,), 0.25, device="cuda"), torch.full((n,), float("nan"), device="cuda")
        lib.call("ganffn_bce2_fwd", ops._ptr(p_d), C.c_float(ta), C.c_float(tb), Bt, split, n, C.c_float(scale), ops._ptr(want_l), 0,
                 ops._stream())
        lib.call("ganffn_bce2_bwd", ops._ptr(p_d), C.c_float(ta), C.c_float(tb), Bt, split, n, C.c_float(scale), ops._ptr(want_d),
                 ops._stream())
        for kl in (None, _kl([S] * n_len), _kl([S + 5] * n_len)):          # NULL, full, above S (clamped to S)
            loss, _, d = _bce_len(lib, p_d, kl, n_len, ta, tb, S, Bt, split, scale)
            assert torch.equal(loss, want_l) and torch.equal(_bits(d.reshape(-1)), _bits(want_d))
    # a length of 0 (or below) is one utterance, a length above S is S: clamped like the attention kernels', not refused
    odd = [0, S + 9, -3] + [2] * (n_len - 3) if n_len >= 3 else [0, S + 9][:n_len]
    a = _bce_len(lib, p_d, _kl(odd), n_len, 1.0, 0.0, S, Bt, split, 1.0)
    b = _bce_len(lib, p_d, _kl(GM.clamp_lengths(odd, S)), n_len, 1.0, 0.0, S, Bt, split, 1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[2]), _bits(b[2])) and bool(torch.isfinite(a[0]).all())


def test_bce_with_lengths_refuses_bad_arguments():
    from gan_ffn_amd import _lib, ops
    p, out = torch.rand(2 * 513, device="cuda"), torch.zeros(2 * 513, device="cuda")
    for S, Bt, split, n_len in ((2, 513, 1, 1), (2, 4, 5, 2), (2, 4, 2, 0), (2, 4, 2, 5), (0, 4, 2, 2)):
        kl = _kl([1] * max(n_len, 1))
        with pytest.raises(_lib.GanffnError):
            _lib.call("ganffn_bce_len_bwd", ops._ptr(p), ops._ptr(kl), n_len, C.c_float(1.0), C.c_float(0.0), S, Bt, split,
                      C.c_float(1.0), ops._ptr(out), ops._stream())
        with pytest.raises(_lib.GanffnError):
            _lib.call("ganffn_bce_len_fwd", ops._ptr(p), ops._ptr(kl), n_len, C.c_float(1.0), C.c_float(0.0), S, Bt, split,
                      C.c_float(1.0), ops._ptr(out), 0, ops._stream())
    with pytest.raises(ValueError):
        ops.bce_len_bwd_raw(p, _kl([1, 1, 1]), 2, 1.0, 0.0, 2, 4, 2, 1.0, out)
    torch.cuda.synchronize()
    assert not out.any()


# ================================================================================================================
# 4. the engine's masked sub-steps against the fp64 oracle
# ================================================================================================================
# The factor on the discriminators' fc1 / fc2 / fc3 weights.  A factor of 4 separates the masked from the unmasked step well with
# dropout OFF (fp64, on the CPU: losses >= 1.2e-2 relative apart), but this test runs in TRAIN mode, and with the 1 / (1 - p)
# factors of the dropout sites the discriminators' logits then leave the range in which an fp32 probability can carry them: the
# fp64 restatement's own probabilities reach 1 - 4e-9 on the fake half and 4e-41 on the real half at valid positions, fp32 rounds
# them to 1.0 and to a denormal, BCELoss's -log(1 - p) term becomes the clamp's 100 instead of 19.3, and rounding the fp64
# probabilities to fp32 alone moves the fp64 loss by 9 % to 99 % on these shapes (every D sub-step of (33, 5) and (50, 2)).  No fp32
# step, masked or not, can meet a 2e-5 loss bound there; on the GPU the first such sub-step, (7, 2) sub-step 4, had 73 % of a
# gradient tensor outside its bound while sub-steps 0 to 3 passed.  With 1.5 (the same CPU check, dropout on, the test's seed and
# batches): valid probabilities stay inside [0.0049, 0.9954], rounding them to fp32 moves the loss by <= 3.3e-8 relative, and
# the masked and the unmasked losses are still >= 79x the bound apart in every sub-step ((7, 2): 79x to 5844x; (33, 5): 143x to
# 3656x; the compared sub-steps of (50, 2): 169x to 462x), the most separated gradient tensor >= 0.84 of its scale.  2 already fails the rounding check (3.4e-5 at (33, 5) sub-step 2).
# The bounds and the 10x condition are unchanged, and asserted per sub-step below.
FC_SHARPEN = 1.5


def _sharp_networks():
    """the formula networks of tests/test_hip_engine_train_oracle.py, the discriminators' fc1 / fc2 / fc3 weights times
    FC_SHARPEN: their probabilities leave 0.5, and the masked and the unmasked losses separate"""
    gens, discs = TO._networks(GEN, DISC)
    with torch.no_grad():
        for m in discs.values():
            for fc in (m.fc1, m.fc2, m.fc3):
                fc.weight.mul_(FC_SHARPEN)
    return gens, discs


class _MaskedHarness(TO._Harness):
    """the harness of the unmasked test with the masked restatement in place of the unmasked one, and the condition on the
    inputs: the unmasked oracle of the same sub-step is further away than 10x the bounds"""

    def __init__(self, eng, compare, monkeypatch, lens):
        super().__init__(eng, compare, monkeypatch)
        self.lens = list(lens)
        self.gaps = []
        self.all_rows = 0.0           # generator outputs over ALL rows, padded ones included: largest error / (1e-4 of scale)

    def _discriminates(self, tag, res, plain):
        """plain: the restatement at full lengths = the unmasked sub-step of tests/engine_oracle.py (tests/test_gan_mask_oracle_cpu.py),
        with a loss whose autograd stays finite where an fp64 sigmoid saturates at a padded row"""
        gl = abs(res["loss"] - plain["loss"]) / abs(res["loss"])
        gg = max(float((res["grads"][k] - plain["grads"][k]).abs().max() / res["grads"][k].abs().max().clamp_min(1e-300))
                 for k in res["grads"])
        self.gaps.append((gl / 2e-5, gg / 1e-3))
        print("%s: masked vs unmasked oracle, loss %.3g relative = %.0f x bound, most separated gradient tensor %.3g of scale = "
              "%.0f x bound" % (tag, gl, gl / 2e-5, gg, gg / 1e-3))
        assert gl > 10 * 2e-5 and gg > 10 * 1e-3, (tag, gl, gg)

    def _close_valid(self, kind, got, want, label):
        """a generator's output at 1e-4 of scale over the REAL utterances: the rows the option defines.  What a generator puts
        out at a padded row is read by nothing (a masked key, a loss term that is left out, a gradient of exactly 0: case 5
        feeds garbage there and no bit of the step moves), so it is printed, not bounded (module docstring, `padded rows`)."""
        valid = valid_rows(got.shape[0], self.lens)
        scale = float(want.abs().max())
        self.all_rows = max(self.all_rows, float((got - want).abs().max()) / (1e-4 * scale))
        TO._close(kind, got[valid].numpy(), want[valid].numpy(), 1e-4, 0.0, label)

    def _check_disc(self, st, gst, xr, xp, b, i, pre, pre_p, post, loss, masks, fake, lr):
        tag = "it%d sub-step %d D %s" % (self.it, i, st.m.__class__.__name__)
        D = EO.Net.from_state(st, pre["slab"])
        G = EO.Net.from_state(gst, pre_p["slab"], requires_grad=False)
        with torch.no_grad(), masked_attention(self.lens):
            fake_o = G.forward(xp, SEED, b + 4 * i + EO.G_ENC, b + 4 * i + EO.G_HEAD, False)
        self._close_valid("fake (G eval)", fake, fake_o, tag + " fake")
        res = GM.disc_substep(D, G, xr, xp, SEED, b, i, self.lens, fake=fake, relu_masks=masks)
        self._discriminates(tag, res, GM.disc_substep(D, G, xr, xp, SEED, b, i, [xr.shape[0]] * len(self.lens)))
        self._check_common(st, tag, res, pre, post, loss, lr)

    def _check_gen(self, st, dst, x, b, i, pre, pre_p, post, loss, masks_g, masks_d, out, lr):
        tag = "it%d sub-step %d G %s" % (self.it, i, st.m.__class__.__name__)
        G = EO.Net.from_state(st, pre["slab"])
        D = EO.Net.from_state(dst, pre_p["slab"], requires_grad=False)
        res = GM.gen_substep(G, D, x, SEED, b, i, self.lens, masks_g, masks_d)
        self._discriminates(tag, res, GM.gen_substep(G, D, x, SEED, b, i, [x.shape[0]] * len(self.lens)))
        self._close_valid("G train output", out, res["out"], tag + " output")
        self._check_common(st, tag, res, pre, post, loss, lr)


# sub-steps compared: every one of the 12 (one D and one G sub-step per ordered modality pair) at the two shapes of
# tests/test_hip_key_len_engines.py; at (50, 2) those that run the 512-wide generator, the one network S = 50 moves to another kernel
ORACLE_CASES = {"7x2": (ENGINE_SHAPES[0], "all"), "33x5": (ENGINE_SHAPES[1], "all"), "50x2": (ENGINE_SHAPES[2], [8, 9, 10, 11])}


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_masked_engine_train_substeps_match_fp64_oracle(case, monkeypatch):
    """Largest error / tolerance per check on an MI355X when the test was added ((7, 2) / (33, 5) / (50, 2)): fake 0.057 / 0.061 /
    0.052, G train output 0.024 / 0.018 / 0.031, loss 0.016 / 0.008 / 0.008, gradient 0.071 / 0.11 / 0.011, Adam moments and
    parameter <= 0.21."""
    from gan_ffn_amd import engine, ops
    (S, B, lens), subs = ORACLE_CASES[case]
    monkeypatch.setenv("GANFFN_ADAM_PARTS", "0")           # the summed gradient stays in net.grad (case 7 covers the other form)
    monkeypatch.setattr(TO, "WORST", {})
    gens, discs = _sharp_networks()
    ops.manual_seed(SEED)
    eng = engine.GanEngine(gens, discs, n_streams=1, mask_padding=True)
    cmp = {(0, i) for i in (range(12) if subs == "all" else subs)}
    h = _MaskedHarness(eng, cmp, monkeypatch, lens)
    batch = _batch(S, B, 31 * S + B, lens=lens)
    eng.iteration({k: batch[k] for k in MODS + ("umask",)})
    torch.cuda.synchronize()
    assert h.compared == len(cmp) == len(h.gaps)
    h.check_offsets(12)
    print("masked engine oracle %s, largest error / tolerance per check: %s; smallest masked / unmasked gap: loss %.0f x bound, "
          "gradient %.0f x bound; generator outputs over all rows, padded ones included: %.3g of the bound" %
          (case, ", ".join("%s %.3g" % kv for kv in sorted(TO.WORST.items())), min(g[0] for g in h.gaps), min(g[1] for g in h.gaps),
           h.all_rows))


# ================================================================================================================
# 5. - 8. whole iterations
# ================================================================================================================
def _state(eng):
    out = {}
    for grp, nets in (("G", eng.G), ("D", eng.D)):
        for k, st in nets.items():
            for name in ("slab", "exp_avg", "exp_avg_sq", "step"):
                out[(grp, k, name)] = getattr(st, name).detach().clone()
    return out


def _iterate(batches, mask_padding, zero_dropout=False, n_streams=1, use_graph=False, seed=SEED):
    """a fresh engine over fresh formula networks, the same seed and dropout offsets every time -> (losses of every iteration,
    the six parameter slabs with their moments and step counts)"""
    from gan_ffn_amd import engine, ops
    gens, discs = build_all(zero_dropout=zero_dropout)
    ops.manual_seed(seed)
    eng = engine.GanEngine(gens, discs, n_streams=n_streams, use_graph=use_graph, mask_padding=mask_padding)
    assert eng.n_streams == n_streams and eng.use_graph == use_graph
    losses = []
    for b in batches:
        ls = eng.iteration(b)
        eng.synchronize()
        losses.append(ls.clone())
    torch.cuda.synchronize()
    return torch.stack(losses), _state(eng)


def _same(a, b):
    assert bool(torch.isfinite(a[0]).all())
    assert torch.equal(a[0], b[0]), (a[0] - b[0]).abs().max()
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def _gan_batch(S, B, lens, seed=None):
    b = _batch(S, B, 31 * S + B if seed is None else seed, lens=lens)
    return {k: b[k] for k in MODS + ("umask",)}


def test_padded_values_change_no_bit_of_an_iteration():
    S, B, lens = 33, 5, [33, 1, 20, 7, 12]
    batch = _gan_batch(S, B, lens)
    other = dict(batch)
    pad = (~valid_rows(S, lens)).cuda().unsqueeze(2)
    g = torch.Generator().manual_seed(1)
    for k in MODS:
        other[k] = torch.where(pad, (torch.randn(batch[k].shape, generator=g) * 3.0).cuda(), batch[k])
        assert not torch.equal(other[k], batch[k])
    _same(_iterate([batch], True), _iterate([other], True))
    a, b = _iterate([batch], False), _iterate([other], False)
    assert not torch.equal(a[0], b[0]) and not all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_more_padding_changes_the_losses_by_rounding_only():
    """dropout off; the same dialogues at S = 33 and with five more zero rows.  Each loss is an fp32 mean of the same <= 146
    real positions (330 for a discriminator), 2e-5 relative from the same fp64 value (the loss bound of the oracle test), so the
    two are within 4e-5 of each other"""
    S, B, lens = 33, 5, [33, 1, 20, 7, 12]
    batch = _gan_batch(S, B, lens)
    longer = {k: torch.cat((batch[k], torch.zeros(5, *batch[k].shape[1:], device="cuda"))) for k in MODS}
    longer["umask"] = torch.cat((batch["umask"], torch.zeros(B, 5, device="cuda")), dim=1)
    a, b = _iterate([batch], True, zero_dropout=True)[0][0], _iterate([longer], True, zero_dropout=True)[0][0]
    rel = ((a - b).abs() / a.abs()).cpu()
    print("12 losses at S = 33 and S = 38, relative differences: " + " ".join("%.2g" % float(r) for r in rel))
    assert bool((rel <= 4e-5).all()), rel
    # the unmasked step is not invariant: its means run over the padded positions too
    ua, ub = _iterate([batch], False, zero_dropout=True)[0][0], _iterate([longer], False, zero_dropout=True)[0][0]
    assert float(((ua - ub).abs() / ua.abs()).max()) > 10 * 4e-5


def test_full_lengths_give_the_unmasked_engines_bits():
    batch = _gan_batch(7, 2, [7, 7])
    assert bool((batch["umask"] == 1).all())
    _same(_iterate([batch, batch], True), _iterate([batch, batch], False))


def test_three_streams_equal_one_with_mask_padding(monkeypatch):
    """(nothing set: three streams pair the 512-wide generator's forwards, one stream pairs none)"""
    monkeypatch.delenv("GANFFN_GEN_PAIR", raising=False)
    batch = _gan_batch(33, 5, [33, 1, 20, 7, 12])
    _same(_iterate([batch, batch], True, n_streams=3), _iterate([batch, batch], True, n_streams=1))


@pytest.mark.parametrize("S,B,lens", [ENGINE_SHAPES[1], ENGINE_SHAPES[2]], ids=["33x5", "50x2"])
def test_paired_generator_forwards_equal_unpaired_with_mask_padding(S, B, lens, monkeypatch):
    batch = _gan_batch(S, B, lens)
    res = {}
    for mode in ("0", "1", "all"):
        monkeypatch.setenv("GANFFN_GEN_PAIR", mode)
        res[mode] = _iterate([batch, batch], True)
    _same(res["1"], res["0"])
    _same(res["all"], res["0"])


def test_unreduced_weight_gradients_equal_reduced_with_mask_padding(monkeypatch):
    batch = _gan_batch(33, 5, [33, 1, 20, 7, 12])
    default = _iterate([batch, batch], True)
    monkeypatch.setenv("GANFFN_ADAM_PARTS", "0")
    _same(default, _iterate([batch, batch], True))


def test_graph_replay_with_another_batchs_umask_equals_eager():
    """replay k is execution k + 1 of the iteration (tests/test_hip_engine.py::test_graph_replay_matches_eager): graph mode over
    [b1, b2] executes b1 (warm-up), b1 (first replay), b2 (second replay, its lengths copied into the captured tensors)"""
    S, B = 9, 3
    b1, b2 = _gan_batch(S, B, [9, 1, 4], seed=1), _gan_batch(S, B, [2, 9, 7], seed=2)
    replay = _iterate([b1, b2], True, use_graph=True)
    eager = _iterate([b1, b1, b2], True)
    assert torch.equal(replay[0][1], eager[0][2]) and torch.equal(replay[0][0], eager[0][1])
    for k in replay[1]:
        assert torch.equal(replay[1][k], eager[1][k]), k
    # and b2's lengths were used: with b1's umask the last execution is another step
    stale = _iterate([b1, b1, dict(b2, umask=b1["umask"])], True)
    assert not torch.equal(stale[0][2], eager[0][2])


def test_mask_padding_without_umask_is_refused():
    from gan_ffn_amd import engine
    gens, discs = build_all(zero_dropout=False)
    batch = _gan_batch(7, 2, [7, 1])
    del batch["umask"]
    with pytest.raises(ValueError, match="umask"):
        engine.train_GAN(gens, discs, [batch], mask_padding=True, n_streams=1)
    with pytest.raises(ValueError, match="umask"):
        engine.GanEngine(gens, discs, mask_padding=True).iteration(dict(batch, umask=torch.ones(7, 2, device="cuda")))
