"""The ranges the C ABI accepts beyond the four workload widths (d_model 100, 512, 600, 300), and inputs beyond order 1.

1. Attention at every head_dim that runs the generic (run-time head_dim) instantiations of csrc/attention.hip
   (`attention_fwd_kernel<0, NT>` / `attention_bwd_kernel<0, NT>`: load_heads_generic, scores_T's run-time k loop, the
   `d < hd` stores): any even head_dim <= 64 other than 10, 30 (16-row kernels) and 60, 64 (compiled-in variants).
2. Every column-chunk count NC of the LayerNorm dispatch of csrc/elementwise.hip, both sides of each boundary.
3. Two-layer encoder stacks at widths off the workload against the fp64 oracle: output, input gradient and EVERY parameter
   gradient (the pair-versus-single bit equalities of tests/test_hip_gen_pair.py pass when a kernel is wrong twice the same
   way).
4. Inputs that punish a dropped row max in a softmax, a one-pass variance in a LayerNorm, an overflowing gate.

Every expected value is the fp64 oracle's (oracle/ganffn_oracle.py, pinned to stock torch at these widths by
tests/test_oracle_widths_cpu.py) or plain fp64 torch on the same seeded inputs.

Bounds of the range checks (part 4, attention and LayerNorm): no bound for __expf / rsqrtf at these magnitudes is derived
here; the yardstick is the oracle itself evaluated in fp32 on the CPU on the same inputs — its error against the fp64
oracle is what fp32 arithmetic costs on this input.  bound = max(the assertion's existing tolerance, 8 x that error); the
factor 8 allows for another summation order and the fast intrinsics.  The module's report line prints the largest
error / bound ratio per check; on an MI355X when the module was added: attention o 0.14, d_qkv 0.26, lse 0.17; LayerNorm
out / dz / dy / gw 0.12 - 0.13, gb 0.02; row-chain LayerNorm 0.19 — the kernels are no further from fp64 than the fp32
oracle is."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ganffn_oracle as O
from oracle import lstm_oracle as LO
from oracle import philox
from test_hip_ops import (attention_case, attention_inputs, attention_oracle, dev, layernorm_case, layernorm_inputs,
                          layernorm_oracle, lib, ptr, rel_err, stream)  # noqa: F401  (lib: the fixture)
from util import _assert_close

pytestmark = pytest.mark.gpu

WORST = {}        # check -> largest error / bound seen in this module (printed at its end)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ndispatch / range checks, largest error / bound per check: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _bounded(kind, err, bound, label):
    WORST[kind] = max(WORST.get(kind, 0.0), err / bound)
    print("%s %s: error %.3e, bound %.3e" % (kind, label, err, bound))
    assert err <= bound, (kind, label, err, bound)


def _range_bound(existing, fp32_err):
    return max(existing, 8.0 * fp32_err)


# ------------------------------------------------------------------------------------------------------------------------
# 1. generic head-dim attention
# ------------------------------------------------------------------------------------------------------------------------
# (S, B, E, H): NT = 1..4 of the 32-row tiling (S across 32 / 64 / 96), head_dim on both sides of the 32-column tile, the
# smallest legal sizes, 320 problems in one launch; (7, 3, 18, 3): E no multiple of 4 (head_dim 6; the loads are float2)
GENERIC_ATTN = [(1, 1, 4, 2), (33, 2, 8, 2), (32, 2, 64, 4), (31, 3, 64, 4), (65, 1, 128, 4), (64, 2, 128, 4), (110, 2, 68, 2),
                (97, 3, 192, 4), (96, 1, 192, 4), (64, 2, 124, 2), (110, 1, 124, 2), (94, 40, 128, 8), (7, 3, 18, 3)]


@pytest.mark.parametrize("S,B,E,H", GENERIC_ATTN)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_generic_head_dim_attention(lib, S, B, E, H, p):
    assert E // H not in (10, 30, 60, 64)          # none of the specialised kernels
    err = attention_case(lib, S, B, E, H, p)
    assert "lse" not in err
    assert err["o"] < 2e-5
    assert err["dq"] < 5e-5


@pytest.mark.parametrize("S,B,E,H,what", [(9, 2, 15, 3, "head_dim=5"), (9, 2, 132, 2, "head_dim=66"), (113, 1, 64, 4, "S=113")])
def test_attention_refusals_leave_the_outputs_untouched(lib, S, B, E, H, what):
    """odd head_dim, head_dim > 64, S = GANFFN_MAX_SEQ + 1: GanffnError with a message that names the value, nothing written"""
    from gan_ffn_amd._lib import GanffnError
    qkv, do = attention_inputs(S, B, E, H)
    qd, dod = dev(qkv), dev(do)
    rng = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
    od = torch.full((S, B, E), -7.0, device="cuda")
    dq = torch.full((S, B, 3 * E), -7.0, device="cuda")
    lse = torch.full((B * H, S), -7.0, device="cuda")
    keep = torch.full((int(lib.load().ganffn_attention_keep_words(B, H)),), -7, dtype=torch.int32, device="cuda")
    tail = (S, B, E, H, C.c_float(0.1), C.c_uint32(16), ptr(rng), C.c_uint64(0), stream())
    with pytest.raises(GanffnError, match=what):
        lib.call("ganffn_attention_fwd", ptr(qd), ptr(od), ptr(lse), *tail)
    with pytest.raises(GanffnError, match=what):
        lib.call("ganffn_attention_bwd", ptr(qd), ptr(od), ptr(lse), ptr(dod), ptr(dq), *tail)
    with pytest.raises(GanffnError, match=what):
        lib.call("ganffn_attention_fwd_keep", ptr(qd), ptr(od), ptr(lse), ptr(keep), *tail)
    with pytest.raises(GanffnError, match=what):
        lib.call("ganffn_attention_bwd_keep", ptr(qd), ptr(od), ptr(lse), ptr(dod), ptr(keep), ptr(dq), *tail)
    torch.cuda.synchronize()
    for t in (od, dq, lse, keep):
        assert bool((t == -7).all())


# ------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm instantiations
# ------------------------------------------------------------------------------------------------------------------------
# E -> NC (64-column chunks per lane): 4, 60, 64 -> 1; 68, 128 -> 2; 132, 256 -> 4; 260, 320 -> 5; 324 -> 8; 600, 640 -> 10;
# 101: accepted by the ABI (any E > 0), no multiple of 4.  T = 1, 5: a partial 4-row group; 331: 21 workgroups, ragged tail
LN_WIDTHS = [4, 60, 64, 68, 128, 132, 256, 260, 320, 324, 600, 640, 101]


@pytest.mark.parametrize("E", LN_WIDTHS)
@pytest.mark.parametrize("T", [1, 5, 331])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layernorm_every_chunk_count(lib, T, E, p):
    err = layernorm_case(lib, T, E, p, g0_scale=1.0)
    assert err["out"] < 5e-6
    for k in ("dz", "dy", "gw", "gb"):
        assert err[k] < 2e-5, k


def test_layernorm_refuses_a_row_wider_than_its_widest_instantiation(lib):
    from gan_ffn_amd._lib import GanffnError
    T, E = 5, 644
    x, y, w, b, dout, gw0, gb0 = (dev(t) for t in layernorm_inputs(T, E))
    rng = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
    mk = lambda *s: torch.full(s, -7.0, device="cuda")
    out, xhat, rstd, dz, dy, gw, gb = mk(T, E), mk(T, E), mk(T), mk(T, E), mk(T, E), mk(E), mk(E)
    with pytest.raises(GanffnError, match="E=644"):
        lib.call("ganffn_add_dropout_layernorm_fwd", ptr(x), ptr(y), ptr(w), ptr(b), ptr(out), ptr(xhat), ptr(rstd),
                 T, E, C.c_float(1e-5), C.c_float(0.1), C.c_uint32(21), ptr(rng), C.c_uint64(0), stream())
    with pytest.raises(GanffnError, match="E=644"):
        lib.call("ganffn_add_dropout_layernorm_bwd", ptr(dout), ptr(x), ptr(rstd), ptr(w), ptr(dz), ptr(dy), ptr(gw),
                 ptr(gb), T, E, C.c_float(0.1), C.c_uint32(21), ptr(rng), C.c_uint64(0), stream())
    torch.cuda.synchronize()
    for t in (out, xhat, rstd, dz, dy, gw, gb):
        assert bool((t == -7).all())


# ------------------------------------------------------------------------------------------------------------------------
# 3. encoder stack against the oracle at off-workload widths
# ------------------------------------------------------------------------------------------------------------------------
# (E, H, F): head_dim 16 / NC 1; 32 / 2; 34 / 4; 62 / 4 with F no multiple of 64
ENC_WIDTHS = [(64, 4, 128), (128, 4, 256), (136, 4, 64), (248, 4, 132)]
ENC_SEED, ENC_ADD = 20261018, 5


def _encoder_inputs(S, B, E, H, F, L, x_offset=0.0, v_scale=1.0):
    """seeded slab / input / pe as tests/test_hip_gen_pair.py::_case builds them, and a seeded d_out; v_scale multiplies the
    v rows of every in-proj (weight and bias): the attention output, and with it the residual branch of LayerNorm 1"""
    from gan_ffn_amd import ops
    g = torch.Generator().manual_seed(1000 * S + 10 * B + E)
    per, offs = ops.layer_layout(E, F)
    slab = (torch.rand(L * per, generator=g) - 0.5) * 0.2
    x = torch.rand(S, B, E, generator=g) + x_offset
    pe = torch.rand(S, E, generator=g)
    dout = torch.randn(S, B, E, generator=g)
    if v_scale != 1.0:
        for l in range(L):
            slab[l * per + offs[0] + 2 * E * E:l * per + offs[0] + 3 * E * E] *= v_scale
            slab[l * per + offs[1] + 2 * E:l * per + offs[1] + 3 * E] *= v_scale
    return slab, x, pe, dout


def _encoder_params(slab, pe, E, F, L):
    """the oracle's parameter dict (fp64 leaves) over a slab"""
    from gan_ffn_amd import ops
    per, offs = ops.layer_layout(E, F)
    P = {"position_encoding.pe": pe.double().unsqueeze(1)}
    for l in range(L):
        for key, o, shape in zip(ops.LAYER_KEYS, offs, ops.layer_shapes(E, F)):
            P["transformer_encoder.layers.%d.%s" % (l, key)] = \
                slab[l * per + o:l * per + o + int(np.prod(shape))].view(shape).double().clone().requires_grad_(True)
    return P


def _encoder_run(S, B, E, H, F, L, train, backward=True, **kw):
    """ganffn_encoder_fwd (saved) on _encoder_inputs and the whole backward of the seeded d_out on the GPU
    -> (x, d_out, P, out, dx, parameter gradients by key, relu masks) — everything on the host"""
    from gan_ffn_amd import ops
    slab, x, pe, dout = _encoder_inputs(S, B, E, H, F, L, **kw)
    cfg = ops.enc_cfg(S, B, E, H, L, F=F, train=train)
    per, offs = ops.layer_layout(E, F)
    n_saved, n_ws = ops.enc_sizes(cfg)
    f32 = dict(device="cuda", dtype=torch.float32)
    rng = torch.tensor([ENC_SEED, 0], dtype=torch.int64, device="cuda")
    slab_d, x_d, pe_d = slab.cuda(), x.cuda(), pe.cuda()
    out = torch.full((S * B * E,), float("nan"), **f32)
    saved, ws = torch.zeros(n_saved, **f32), torch.zeros(n_ws, **f32)
    ops.encoder_fwd_raw(cfg, x_d, pe_d, slab_d, out, saved, ws, rng, ENC_ADD)
    dx = dout.cuda().clone()
    gslab = torch.zeros_like(slab_d)
    if backward:
        ops.encoder_bwd_raw(cfg, 0, L, dx, slab_d, gslab, saved, ws, rng, ENC_ADD)
    torch.cuda.synchronize()
    masks = []
    for l in range(L):
        off = int(ops._lib.load().ganffn_encoder_saved_hidden_offset(C.byref(cfg), l))
        assert off >= 0 and off + S * B * F <= n_saved
        masks.append((saved[off:off + S * B * F] != 0).view(S, B, F).double().cpu())   # dropped units read 0: gradient 0 whatever the pattern
    P, G = _encoder_params(slab, pe, E, F, L), {}
    gs = gslab.cpu()
    for l in range(L):
        for key, o, shape in zip(ops.LAYER_KEYS, offs, ops.layer_shapes(E, F)):
            G["transformer_encoder.layers.%d.%s" % (l, key)] = gs[l * per + o:l * per + o + int(np.prod(shape))].view(shape)
    return x, dout, P, out.view(S, B, E).cpu(), dx.cpu(), G, masks


@pytest.mark.parametrize("E,H,F", ENC_WIDTHS)
@pytest.mark.parametrize("S,B", [(9, 4), (33, 3)])
def test_encoder_stack_matches_oracle_off_the_workload_widths(S, B, E, H, F):
    """L = 2, train mode, default dropout rates, a non-zero rng offset: output, dx and all 24 parameter gradients against the
    fp64 oracle with the same Philox masks, run on the ReLU pattern the HIP forward took, no outliers; and the kink audit
    that licenses that: a kept hidden unit whose pattern differs from the oracle's own has an fp64 pre-activation within
    2e-5 of the layer's scale"""
    L = 2
    x, dout, P, out, dx, G, masks = _encoder_run(S, B, E, H, F, L, train=True)
    xo = x.double().requires_grad_(True)
    trace = []
    yo = O.encoder_stack(xo, P, H, O.Rng(ENC_SEED, ENC_ADD, True), n_layers=L, relu_masks=masks, trace=trace)
    (yo * dout.double()).sum().backward()
    _assert_close(out.double().numpy(), yo.detach().numpy(), 1e-4, 1e-6, "out", 0.0, 1.0)
    _assert_close(dx.double().numpy(), xo.grad.numpy(), 2e-4, 1e-8, "dx", 0.0, 1.0)
    assert len(G) == 12 * L
    for k, got in G.items():
        _assert_close(got.double().numpy(), P[k].grad.numpy(), 1e-3, 1e-8, "grad " + k, 0.0, 1.0)
    flips = 0
    for l in range(L):
        kept = torch.from_numpy(philox.keep_mask(S * B, F, O.ENC_DROPOUT, O.SITE_LAYER0 + 4 * l + 2, ENC_SEED, ENC_ADD)).view(S, B, F)
        assert not bool((masks[l] > 0)[~kept].any())         # every unit the contract drops reads 0
        diff = kept & ((trace[l] > 0) != (masks[l] > 0))
        flips += int(diff.sum())
        if diff.any():
            assert float(trace[l][diff].abs().max()) < 2e-5 * max(1.0, float(trace[l].abs().max())), (l, float(trace[l][diff].abs().max()))
    assert flips <= max(1, 1e-4 * L * S * B * F), flips


# ------------------------------------------------------------------------------------------------------------------------
# 4. input range
# ------------------------------------------------------------------------------------------------------------------------
# one case per kernel family: 16-row, 32-row compiled-in head_dim, 32-row generic.  q and k times 6: scores of +-190 at
# (65, 2, 128, 4), past the fp32 exp overflow at 88 — a softmax that dropped or mis-scaled its row max gives inf / NaN
@pytest.mark.parametrize("S,B,E,H", [(94, 2, 100, 10), (94, 2, 512, 8), (65, 2, 128, 4)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_with_scores_past_the_exp_overflow(lib, S, B, E, H, p):
    qkv, do = attention_inputs(S, B, E, H, qk_scale=6.0)
    hd = E // H
    scores = torch.einsum("sbhd,tbhd->bhst", qkv[..., :E].double().reshape(S, B, H, hd), qkv[..., E:2 * E].double().reshape(S, B, H, hd)) / hd ** 0.5
    assert float(scores.abs().max()) > 100.0
    o64, dq64 = attention_oracle(qkv, do, B, H, p)
    o32, dq32 = attention_oracle(qkv, do, B, H, p, dtype=torch.float32)
    assert bool(torch.isfinite(o64).all() and torch.isfinite(dq64).all())
    err = attention_case(lib, S, B, E, H, p, qk_scale=6.0)
    tag = "%s p=%g" % ((S, B, E, H), p)
    _bounded("attention o", err["o"], _range_bound(2e-5, rel_err(o32, o64)), tag)
    _bounded("attention d_qkv", err["dq"], _range_bound(5e-5, rel_err(dq32, dq64)), tag)
    if "lse" in err:
        q32, k32 = (qkv[..., i * E:(i + 1) * E].reshape(S, B * H, hd).transpose(0, 1) for i in (0, 1))
        lse32 = torch.logsumexp(q32 @ k32.transpose(1, 2) / hd ** 0.5, dim=-1)
        lse32_err = float((lse32.double() - torch.logsumexp(scores, dim=-1).reshape(B * H, S)).abs().max())
        _bounded("attention lse", err["lse"], _range_bound(2e-5, lse32_err), tag)


# rows with mean 1000 and spread 0.5 (x 1000 + 0.5 n, y 0.25 n): a one-pass variance E[z^2] - mean^2 loses the variance
# (~0.3) in the rounding of 10^6.  E -> NC 1, 2, 8
@pytest.mark.parametrize("E", [64, 100, 512])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layernorm_with_a_row_mean_far_above_its_spread(lib, E, p):
    T = 331
    kw = dict(mean=1000.0, spread=0.5, y_scale=0.25, g0_scale=1.0)
    inputs = layernorm_inputs(T, E, **kw)
    r64, r32 = layernorm_oracle(inputs, p), layernorm_oracle(inputs, p, dtype=torch.float32)
    err = layernorm_case(lib, T, E, p, **kw)
    existing = {"out": 5e-6, "dz": 2e-5, "dy": 2e-5, "gw": 2e-5, "gb": 2e-5}
    for k in ("out", "dz", "dy", "gw", "gb"):
        _bounded("layernorm " + k, err[k], _range_bound(existing[k], rel_err(r32[k], r64[k])), "E=%d p=%g" % (E, p))


def _rowchain_ln1_input(x, P, B, H):
    """the row LayerNorm 1 of layer 0 normalises, eval mode, in x's dtype: z = x0 + out_proj(attention(in_proj(x0))), x0 = x + pe"""
    pre = "transformer_encoder.layers.0.self_attn."
    x0 = O.positional_encoding(x, P["position_encoding.pe"])
    a = O.attention(x0 @ P[pre + "in_proj_weight"].T + P[pre + "in_proj_bias"], B, H, 0, None)
    return x0 + a @ P[pre + "out_proj.weight"].T + P[pre + "out_proj.bias"]


ROWCHAIN_RANGE = dict(S=9, B=4, E=100, H=10, F=2048, L=1, x_offset=1000.0, v_scale=1e-3)


def test_rowchain_layernorm_with_a_row_mean_far_above_its_spread():
    """d_model 100 runs its LayerNorms inside the row-chain kernels (csrc/rowchain.hip: one LayerNorm body for both norms),
    not in the kernels above: one ganffn_encoder_fwd layer, eval mode, x = 1000 + uniform(0, 1).  With the seeded slab as it
    is, the v projection of such an x is +-500 and LayerNorm 1 sees a spread of hundreds; the v rows of the in-proj are
    therefore scaled by 1e-3, which leaves z = x + pe + (a term of order 0.1).  Asserted from the fp64 oracle: every row of
    z has |mean| / std > 1000 — there a one-pass variance E[z^2] - mean^2 has lost the variance (~0.2) in the rounding
    of 10^6.  Output of the layer against the fp64 oracle, bounded by the fp32 oracle's error."""
    kw = ROWCHAIN_RANGE
    x, dout, P, out, dx, G, masks = _encoder_run(train=False, backward=False, **kw)
    with torch.no_grad():
        z = _rowchain_ln1_input(x.double(), P, kw["B"], kw["H"])
        assert float((z.mean(-1).abs() / z.std(-1)).min()) > 1000.0
        y64 = O.encoder_stack(x.double(), P, kw["H"], None, n_layers=1)
        y32 = O.encoder_stack(x, {k: v.detach().float() for k, v in P.items()}, kw["H"], None, n_layers=1)
    assert bool(torch.isfinite(out).all())
    _bounded("rowchain layernorm out", rel_err(out, y64), _range_bound(1e-4, rel_err(y32, y64)), "E=100")


@pytest.mark.parametrize("shift", [0.0, 80.0, -80.0])
def test_logsoftmax_nll_is_shift_invariant_at_large_logits(lib, shift):
    """logits with a spread of 30 shifted by +-80 give the log-probabilities of the unshifted fp64 ones.  The logits are
    multiples of 1/64 below 2^9, so the shift is exact in fp32 and the property holds for the kernel's actual input."""
    S, B, Cn = 7, 3, 6
    g = torch.Generator().manual_seed(17)
    base = torch.round(torch.randn(S, B, Cn, generator=g) * 30 * 64) / 64
    labels = torch.randint(0, Cn, (B, S), generator=g)
    umask = (torch.rand(B, S, generator=g) > 0.2).float()
    umask[0, 0] = 1.0
    logits = (base + shift)
    assert torch.equal(logits.double() - shift, base.double())
    x = base.double().requires_grad_(True)
    lp_ref = torch.log_softmax(x, 2)
    w = torch.tensor(O.CLASS_WEIGHTS)
    loss_ref = O.masked_nll(lp_ref, labels, umask.double(), w.double())
    loss_ref.backward()
    ld, lbd, umd, wd = dev(logits), dev(labels), dev(umask), dev(w)
    lp, dl = torch.full((S, B, Cn), float("nan"), device="cuda"), torch.full((S, B, Cn), float("nan"), device="cuda")
    loss, ws2 = torch.full((1,), float("nan"), device="cuda"), torch.zeros(2, device="cuda")
    lib.call("ganffn_logsoftmax_nll", ptr(ld), ptr(lbd), ptr(umd), ptr(wd), ptr(lp), ptr(loss), ptr(dl), ptr(ws2), S, B, Cn, stream())
    e = (lp.double().cpu() - lp_ref.detach()).abs() / lp_ref.detach().abs().clamp_min(1.0)
    assert float(e.max()) < 2e-6, float(e.max())
    assert abs(float(loss) - float(loss_ref)) < 2e-6 * max(1.0, abs(float(loss_ref)))
    assert rel_err(dl, x.grad) < 1e-5


def test_logsoftmax_nll_with_every_token_masked_is_zero_not_nan(lib):
    """sum of the mask weights = 0: the loss and its gradient are defined as 0 (include/ganffn.h), not 0 / 0"""
    S, B, Cn = 5, 2, 6
    g = torch.Generator().manual_seed(3)
    logits = dev(torch.randn(S, B, Cn, generator=g))
    labels = dev(torch.randint(0, Cn, (B, S), generator=g))
    umask = torch.zeros(B, S, device="cuda")
    w = torch.tensor(O.CLASS_WEIGHTS, device="cuda")
    for cw in (w, None):
        lp, dl = torch.full((S, B, Cn), float("nan"), device="cuda"), torch.full((S, B, Cn), float("nan"), device="cuda")
        loss, ws2 = torch.full((1,), float("nan"), device="cuda"), torch.zeros(2, device="cuda")
        lib.call("ganffn_logsoftmax_nll", ptr(logits), ptr(labels), ptr(umask), ptr(cw), ptr(lp), ptr(loss), ptr(dl), ptr(ws2),
                 S, B, Cn, stream())
        assert float(loss) == 0.0 and bool((dl == 0).all())
        assert float((lp.cpu().double() - torch.log_softmax(logits.cpu().double(), 2)).abs().max()) < 2e-6


def test_lstm_layer_with_saturated_gates():
    """every weight of a (5, 3, 8, 4) layer times 40: gate pre-activations beyond +-100, where __expf overflows to inf on one
    side and underflows to 0 on the other — sigmoid = 1 / (1 + inf) and 1 / (1 + 0) must come out as clean 0 / 1, nothing
    NaN; the tolerances of tests/test_hip_lstm.py::test_one_bidirectional_layer_forward_and_backward (the oracle in fp32
    on the CPU is within 3e-7 / 1e-6 / 2.1e-6 of its fp64 self on these inputs)"""
    from gan_ffn_amd import ops
    from test_hip_lstm import make_lstm, rel
    S, B, In, H = 5, 3, 8, 4
    lstm = make_lstm(In, H, 1, seed=S * 7 + B)
    with torch.no_grad():
        for p in lstm.parameters():
            p.mul_(40.0)
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    keys = names + [n + "_reverse" for n in names]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(S, B, In, generator=g)
    gy = torch.randn(S, B, 2 * H, generator=g)
    P = {k: p.detach().double().requires_grad_(True) for k, p in lstm.named_parameters()}
    pre = x.double() @ P["weight_ih_l0"].detach().T + P["bias_ih_l0"].detach() + P["bias_hh_l0"].detach()
    assert float(pre.max()) > 60 and float(pre.min()) < -60 and float(pre.abs().max()) > 89     # up to and past exp's overflow
    xo = x.double().requires_grad_(True)
    yo = LO.lstm_forward(xo, P, 1)
    (yo * gy.double()).sum().backward()
    pc = [getattr(lstm, k).detach().cuda().requires_grad_(True) for k in keys]
    xc = x.cuda().requires_grad_(True)
    y = ops.LstmLayerFn.apply(xc, *pc)
    (y * gy.cuda()).sum().backward()
    for t in [y, xc.grad] + [t.grad for t in pc]:
        assert bool(torch.isfinite(t).all())
    assert rel(y.detach(), yo.detach()) < 2e-6
    assert rel(xc.grad, xo.grad) < 2e-5
    for k, t in zip(keys, pc):
        assert rel(t.grad, P[k].grad) < 3e-5, k


def test_dialogue_rnn_cell_with_saturated_gates():
    """the GRU gates of the three cells pushed to +-60 and beyond through their input biases (times 1000: +-67, plus the
    products), through the harness and tolerances of tests/test_hip_drnn_kernel.py.  The biases and not the matrices: a
    500-wide GRU with its matrices scaled up is chaotic — the module itself in fp32 on the CPU then misses the emotion
    tolerance against its fp64 self (2.4e-5 at a factor 10) — while with saturating biases it stays at 2.5e-7.
    What this checks: the emotions and attention weights at the harness's tolerances, and that nothing anywhere is NaN or
    inf.  It is NOT a parity check of saturated gradients: the candidate gate's tanh saturates with the others, most
    gradients are close to 0, and the harness compares each against the tensor's maximum."""
    import copy
    import test_hip_drnn_kernel as TK
    S, B = 7, 3
    U, qmask = TK.make_inputs(S, B, seed=S * 100 + B)
    m_cpu = TK.build().double().eval()
    big = 0.0
    with torch.no_grad():
        for n, p in m_cpu.named_parameters():
            if n.endswith("bias_ih"):
                p.mul_(1000.0)
                big = max(big, float(p.abs().max()))
    assert big > 60.0
    m_gpu = copy.deepcopy(m_cpu).float().cuda().eval()
    TK.compare(m_gpu, m_cpu, U, qmask)                     # its tolerances; a NaN anywhere fails its comparison
    e, alpha = m_gpu(U.cuda(), qmask.cuda())
    assert bool(torch.isfinite(e).all()) and all(bool(torch.isfinite(a).all()) for a in alpha)
    for k, p in m_gpu.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), k
