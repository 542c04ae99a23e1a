"""encoder_bwd_impl (gan_ffn_amd/csrc/api.hip) beyond the one shape the rest of the suite runs it in (layer_lo = 0,
layer_hi = L, L in {1, 2, 8}): the backward as a sequence of layer ranges, stacks deep enough for second launches of the
grouped weight-gradient kernel and of the LayerNorm reduce, and the unreduced chunk slabs at the raw ABI.

1. Layer ranges.  One forward with `saved`, then ganffn_encoder_bwd2 once per range, top range first, on one dx buffer and one
   gradient slab that starts as seeded non-zero values (so += is checked); dx after the last range and all 12 L parameter
   gradients against the fp64 oracle with the same Philox masks, run on the ReLU pattern the HIP forward took.  The
   workspace is refilled with NaN before every call: a range may not read what the range above left in scratch.  Also:
   grads = NULL and need_dx_in = 0 over an upper range, need_dx_in = 0 at the bottom range, key lengths, refusals.
2. Deep stacks, whole range, (S, B) = (5, 2): d_model 100 at L = 10, 11, 16, 17, 21 and 64-wide at L = 11, 17, 64.
3. ganffn_encoder_bwd_parts + ganffn_adam_step_parts against ganffn_encoder_bwd2 + ganffn_adam_step at L = 1, 2, 10 and
   T = 320, 564, 1100, and at L = 8, T = 1100: identical bits, and the chunk count the rule of gemm_tn100.hip gives
   (tests/encoder_range_cases.py).  At L = 10, T = 1100 this test found the two forms on different counts (3 chunks unreduced,
   2 in the reduce launch, whose workspace clamp asks for one slab more): other bits in the Adam step.  Both run 2 now.

What splitting the range does NOT promise: the bits of the whole-range call.  At d_model 100 a layer below a range boundary
reads dx from a plain GEMM (d_qkv W_in + dz1 in its epilogue) where the whole-range pass computes that product inside the
LayerNorm-2 backward kernel of the layer below, in another summation order; at the other widths the boundary GEMM is
unsplit where the inner one cuts K into slabs; and a smaller group of weight-gradient problems may cut its token range into
another number of chunks (from 512 tokens on).  So split and whole-range results agree to rounding — both are held to the
oracle here — not to the bit.  What IS bit-equal, and asserted: the parameter gradients of the layers of the TOP range
below 512 tokens at d_model 100 and 64 (same inputs, one token chunk either way, per-element arithmetic independent of the
group); at d_model 512 the grouped kernel changes its tile shape with the size of the group, so nothing is claimed there.

Inputs: tests/test_hip_dispatch_range.py's seeded ones with 1 added to the LayerNorm weights (encoder_range_cases.inputs:
as seeded, the gradients shrink tenfold per layer and the lower layers of a deep stack would be compared at 1e-36).

Bounds: out 1e-4, dx 2e-4, gradients 1e-3 (test_encoder_stack_matches_oracle_off_the_workload_widths), or 8 x the error of
the oracle evaluated in fp32 on the CPU on the same inputs, masks and ReLU pattern where that is larger (_range_bound); no
element is left out.  The fp32 oracle's error is below 3e-6 on every case here, so every bound is the existing tolerance.
The module's report line prints the largest error / bound per check; on an MI355X when the module was added: ranges out 0.012,
dx 0.018, grad 0.0039; key lengths out 0.0054, dx 0.0023, grad 0.00055; deep stacks out 0.011, dx 0.0052, grad 0.0026 — at
depth 64 as at depth 4 the kernels are some fifty times closer to fp64 than the tolerances ask."""
import ctypes as C

import pytest
import torch

import encoder_range_cases as RC
from test_hip_dispatch_range import ENC_ADD, _bounded
from util import _assert_close

pytestmark = pytest.mark.gpu

KINDS = ("ranges", "len", "deep")
_CASES = {}          # case id -> (forward, fp64 oracle, fp32 oracle, initial gradient slab)
_WHOLE = {}          # case id -> gradient slab of the whole-range backward


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    from test_hip_dispatch_range import WORST
    mine = sorted((k, v) for k, v in WORST.items() if k.split(" ")[0] in KINDS)
    print("\nencoder ranges / deep stacks, largest error / bound per check: " + ", ".join("%s %.3g" % kv for kv in mine))
    _CASES.clear()
    _WHOLE.clear()


def _case(c):
    """forward on the GPU, the fp64 / fp32 oracle on its ReLU pattern, the seeded initial gradients: once per case"""
    key = RC.case_id(c)
    if key not in _CASES:
        fw = RC.forward(c)
        g0 = RC.seeded_gradients(fw.ins[0].numel())
        r64, r32 = RC.expected(c, fw.ins, g0, fw.masks)
        _CASES[key] = (fw, r64, r32, g0)
    return _CASES[key]


def _compare(tag, label, c, got, r64, r32, which=("out", "dx", "grad")):
    """every quantity of `got` (namespace out / dx / grads) through _assert_close, no outliers, at the bound of its kind"""
    worst = {}
    n = 0
    for (kind, name, ref), (_, _, ref32) in zip(RC.quantities(r64, c.L), RC.quantities(r32, c.L)):
        if kind not in which:
            continue
        t = got.out if kind == "out" else got.dx if kind == "dx" else got.grads[name[5:]]
        assert bool(torch.isfinite(t).all()), name
        rtol, atol = RC.bound(kind, RC.rel_err(ref32, ref)), RC.EXISTING[kind][1]
        scale = max(float(ref.abs().max()), 1e-30)
        tol = atol + rtol * scale
        err = float((t.double() - ref).abs().max())
        if kind not in worst or err / tol > worst[kind][0] / worst[kind][1]:
            worst[kind] = (err, tol, name)
        n += 1
    for kind, (err, tol, name) in sorted(worst.items()):
        _bounded("%s %s" % (tag, kind), err, tol, "%s %s (worst: %s)" % (RC.case_id(c), label, name))
    # the gate itself, after the figures are out
    for (kind, name, ref) in RC.quantities(r64, c.L):
        if kind in which:
            t = got.out if kind == "out" else got.dx if kind == "dx" else got.grads[name[5:]]
            r32q = r32.out if kind == "out" else r32.dx if kind == "dx" else r32.grads[name[5:]]
            _assert_close(t.double().numpy(), ref.numpy(), RC.bound(kind, RC.rel_err(r32q, ref)), RC.EXISTING[kind][1], name, 0.0, 1.0)
    return n


def _got(c, fw, dx, gs):
    import types
    return types.SimpleNamespace(out=fw.out, dx=dx.view(c.S, c.B, c.E), grads=RC.slab_views(gs, c.E, c.F, c.L))


# ------------------------------------------------------------------------------------------------------------------------
# 1. layer ranges
# ------------------------------------------------------------------------------------------------------------------------
def _range_case(tag, c, ranges):
    fw, r64, r32, g0 = _case(c)
    dx, gs = RC.run_ranges(fw, ranges, g0)
    got = _got(c, fw, dx, gs)
    assert _compare(tag, RC.ranges_id(ranges), c, got, r64, r32) == 2 + 12 * c.L
    flips = RC.kink_flips(c, fw, r64)
    assert flips <= max(1, 1e-4 * c.L * c.S * c.B * c.F), flips
    return fw, g0, got


@pytest.mark.parametrize("c,ranges", RC.RANGE_CASES, ids=[RC.case_id(c) + "-" + RC.ranges_id(r) for c, r in RC.RANGE_CASES])
def test_backward_over_layer_ranges_matches_the_oracle(c, ranges):
    fw, g0, got = _range_case("ranges", c, ranges)
    if c.S * c.B < 512 and (c.E, c.H, c.F) in (RC.ROWCHAIN, RC.GENERIC):
        # the layers of the top range: the whole-range call's bits (module docstring)
        key = RC.case_id(c)
        if key not in _WHOLE:
            _WHOLE[key] = RC.run_ranges(fw, [(0, c.L)], g0)[1]
        whole = RC.slab_views(_WHOLE[key], c.E, c.F, c.L)
        lo, hi = ranges[0]
        for l in range(lo, hi):
            for k in RC.keys(c.L)[12 * l:12 * l + 12]:
                assert RC.same_bits(got.grads[k], whole[k]), k


@pytest.mark.parametrize("c,ranges", RC.LEN_CASES, ids=[RC.case_id(c) for c, _ in RC.LEN_CASES])
def test_backward_over_layer_ranges_with_key_lengths(c, ranges):
    """ganffn_encoder_fwd_len, then ganffn_encoder_bwd_len over [2,4) [0,2) with ragged key lengths (one dialogue of a single
    utterance, one of full length) against the masked oracle of tests/key_len_oracle.py"""
    _range_case("len", c, ranges)


@pytest.mark.parametrize("w", RC.WIDTHS, ids=lambda w: "E%d" % w[0])
def test_null_gradients_and_no_input_gradient_over_an_upper_range(w):
    """[2,4) of a 4-layer stack alone.  grads = NULL: dx has the bits of the run with gradients, and a NaN-filled gradient
    slab that is passed nowhere stays NaN.  need_dx_in = 0: the flag acts only at layer_lo == 0, so dx is written and both
    dx and the gradients have the need_dx_in = 1 bits."""
    c = RC.case(w, 4, 9, 4)
    fw, _, _, g0 = _case(c)
    dx1, gs1 = RC.run_ranges(fw, [(2, 4)], g0)
    assert not RC.same_bits(dx1, fw.dout_d.cpu()) and bool(torch.isfinite(dx1).all())
    bystander = torch.full_like(fw.slab_d, float("nan"))
    dx0, none = RC.run_ranges(fw, [(2, 4)], grads=False)
    assert none is None and RC.same_bits(dx0, dx1)
    assert bool(torch.isnan(bystander).all())
    dx2, gs2 = RC.run_ranges(fw, [(2, 4)], g0, need_dx_in=False)
    assert RC.same_bits(dx2, dx1) and RC.same_bits(gs2, gs1)
    per = g0.numel() // c.L
    assert RC.same_bits(gs1[:2 * per], g0[:2 * per])           # the layers below the range: untouched
    v1, v0 = RC.slab_views(gs1, c.E, c.F, c.L), RC.slab_views(g0, c.E, c.F, c.L)
    for k in RC.keys(c.L)[24:]:
        assert float((v1[k] - v0[k]).abs().max()) > 1e-3, k     # every parameter of the range: added to


@pytest.mark.parametrize("w", RC.WIDTHS, ids=lambda w: "E%d" % w[0])
def test_no_input_gradient_at_the_bottom_range_leaves_the_parameter_gradients(w):
    """[2,4) [0,2) with need_dx_in = 0: layer 0's in-proj dgrad and the PE dropout backward are skipped (dx is undefined
    afterwards), every parameter gradient has the need_dx_in = 1 bits"""
    c = RC.case(w, 4, 9, 4)
    fw, _, _, g0 = _case(c)
    ranges = RC.PARTITIONS[4][0]
    _, gs1 = RC.run_ranges(fw, ranges, g0)
    _, gs0 = RC.run_ranges(fw, ranges, g0, need_dx_in=False)
    assert RC.same_bits(gs0, gs1)


@pytest.mark.parametrize("w", [RC.ROWCHAIN, RC.GENERIC], ids=lambda w: "E%d" % w[0])
@pytest.mark.parametrize("lo,hi", [(2, 2), (3, 2), (-1, 2), (2, 5)])
def test_bad_layer_ranges_are_refused_and_write_nothing(w, lo, hi):
    from gan_ffn_amd import ops
    from gan_ffn_amd._lib import GanffnError
    from test_hip_ops import ptr, stream
    c = RC.case(w, 4, 9, 4)
    fw = _case(c)[0]
    dx = torch.full_like(fw.dout_d, -7.0)
    gs = torch.full_like(fw.slab_d, -7.0)
    fw.ws.fill_(-7.0)
    key_len = torch.full((c.B,), c.S, dtype=torch.int32, device="cuda")
    with pytest.raises(GanffnError, match="bad layer range"):
        ops.encoder_bwd_raw(fw.cfg, lo, hi, dx, fw.slab_d, gs, fw.saved, fw.ws, fw.rng, ENC_ADD)
    with pytest.raises(GanffnError, match="bad layer range"):
        ops.encoder_bwd_raw(fw.cfg, lo, hi, dx, fw.slab_d, gs, fw.saved, fw.ws, fw.rng, ENC_ADD, key_len=key_len)
    with pytest.raises(GanffnError, match="bad layer range"):
        ops._lib.call("ganffn_encoder_bwd", C.byref(fw.cfg), lo, hi, ptr(dx), ptr(fw.slab_d), ptr(gs), ptr(fw.saved), ptr(fw.ws),
                      ptr(fw.rng), C.c_uint64(ENC_ADD), stream())
    torch.cuda.synchronize()
    for t in (dx, gs, fw.ws):
        assert bool((t == -7).all())


# ------------------------------------------------------------------------------------------------------------------------
# 2. deep stacks
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.DEEP_CASES, ids=RC.case_id)
def test_deep_stack_matches_the_oracle(c):
    """whole-range forward and backward, train mode: output, dx and all 12 L gradients.  4 L weight-gradient problems against
    the 40 of one grouped launch, 2 L LayerNorm instances against the 32 of one reduce launch (encoder_range_cases.DEEP_L)"""
    fw, r64, r32, g0 = _case(c)
    dx, gs = RC.run_ranges(fw, [(0, c.L)], g0)
    assert _compare("deep", "[0,%d)" % c.L, c, _got(c, fw, dx, gs), r64, r32) == 2 + 12 * c.L


@pytest.mark.parametrize("c", RC.DEEP_EVAL_CASES, ids=RC.case_id)
def test_deep_eval_forward_without_saved_has_the_bits_of_the_one_with(c):
    from gan_ffn_amd import ops
    fw, r64, r32, _ = _case(c)
    import types
    _compare("deep", "eval", c, types.SimpleNamespace(out=fw.out), r64, r32, which=("out",))
    out = torch.full((c.S * c.B * c.E,), float("nan"), device="cuda")
    ws = torch.full((fw.n_ws,), float("nan"), device="cuda")
    ops.encoder_fwd_raw(fw.cfg, fw.x_d, fw.pe_d, fw.slab_d, out, None, ws, fw.rng, ENC_ADD)
    torch.cuda.synchronize()
    assert RC.same_bits(out.cpu().view(c.S, c.B, c.E), fw.out)


def test_unreduced_form_ends_at_ten_layers_and_its_refusal_writes_nothing():
    from gan_ffn_amd import ops
    from gan_ffn_amd._lib import GanffnError
    from test_hip_ops import ptr, stream
    S, B = RC.DEEP_S, RC.DEEP_B
    E, H, F = RC.ROWCHAIN
    lib = ops._lib.load()
    for L, want in ((1, 1), (10, 1), (11, 0), (64, 0)):
        assert int(lib.ganffn_encoder_bwd_parts_supported(C.byref(ops.enc_cfg(S, B, E, H, L, F=F, train=True)))) == want, L
    assert int(lib.ganffn_encoder_bwd_parts_supported(C.byref(ops.enc_cfg(S, B, 64, 4, 2, F=128, train=True)))) == 0
    c = RC.case(RC.ROWCHAIN, 11, S, B)
    fw = _case(c)[0]
    dx = torch.full_like(fw.dout_d, -7.0)
    gs = torch.full_like(fw.slab_d, -7.0)
    fw.ws.fill_(-7.0)
    off, stride, n = C.c_int64(-7), C.c_int64(-7), C.c_int(-7)
    with pytest.raises(GanffnError, match="ganffn_encoder_bwd_parts_supported"):
        ops._lib.call("ganffn_encoder_bwd_parts", C.byref(fw.cfg), ptr(dx), ptr(fw.slab_d), ptr(gs), ptr(fw.saved), ptr(fw.ws),
                      ptr(fw.rng), C.c_uint64(ENC_ADD), 1, C.byref(off), C.byref(stride), C.byref(n), stream())
    torch.cuda.synchronize()
    assert (off.value, stride.value, n.value) == (-7, -7, -7)
    for t in (dx, gs, fw.ws):
        assert bool((t == -7).all())


# ------------------------------------------------------------------------------------------------------------------------
# 3. chunk slabs at the raw ABI
# ------------------------------------------------------------------------------------------------------------------------
ADAM = dict(lr=1e-4, b1=0.5, b2=0.6, eps=1e-8, wd=1e-5, gscale=0.5)
TAIL = 16            # floats behind the encoder region (heads, `object` in a network): gradients that still accumulate


@pytest.mark.parametrize("L,S,B", RC.SLAB_CASES, ids=["L%d-T%d" % (L, S * B) for L, S, B in RC.SLAB_CASES])
def test_unreduced_chunk_slabs_give_the_reduce_launchs_adam_step(L, S, B):
    """path A: encoder region of the gradient slab filled with NaN, ganffn_encoder_bwd_parts, ganffn_adam_step_parts;
    path B: encoder region zeroed, ganffn_encoder_bwd2 over [0, L), ganffn_adam_step.  Same forward, same saved, same seeded
    Adam state: parameters, both moments, the step counter and dx have identical bits, and no NaN survives in path A (the
    workspace is NaN before the backward too: a chunk that was not written would surface).  n_parts is what the rule gives."""
    from gan_ffn_amd import ops
    lib = ops._lib.load()
    c = RC.case(RC.ROWCHAIN, L, S, B)
    T = S * B
    fw = RC.forward(c)
    per, _ = ops.layer_layout(c.E, c.F)
    part_floats = int(lib.ganffn_gemm_tn_grouped_workspace_floats())
    covered = int(lib.ganffn_encoder_bwd_parts_covered(c.E, c.F))
    assert (per, part_floats, covered) == (RC.LAYER_FLOATS_100, RC.PART_FLOATS, RC.COVERED_100)      # what the CPU module checked the table with
    enc, n = L * per, L * per + TAIL
    assert ops.encoder_bwd_parts_supported(fw.cfg)
    g = torch.Generator().manual_seed(100 * L + T)
    p0 = torch.cat([fw.ins[0], torch.randn(TAIL, generator=g) * 0.1])
    m0 = torch.randn(n, generator=g) * 0.01
    v0 = torch.rand(n, generator=g) * 1e-4
    gtail = torch.randn(TAIL, generator=g)
    res = []
    for path in "AB":
        p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
        step = torch.tensor([3], dtype=torch.int32, device="cuda")
        grad = torch.full((n,), float("nan") if path == "A" else 0.0, device="cuda")
        grad[enc:] = gtail.cuda()
        dx = fw.dout_d.clone()
        fw.ws.fill_(float("nan"))
        if path == "A":
            parts, stride, n_parts, off = ops.encoder_bwd_parts_raw(fw.cfg, dx, p, grad, fw.saved, fw.ws, fw.rng, ENC_ADD, True)
            want, binding = RC.expected_chunks(L, T, part_floats, per, covered)
            print("L=%d T=%d: n_parts %d (rule %d, binding term: %s)" % (L, T, n_parts, want, binding))
            assert n_parts == want == RC.SLAB_CHUNKS[(L, T)]
            if n_parts > 1:
                assert stride == enc and off > 0 and off % 4 == 0 and off + (n_parts - 1) * stride <= fw.n_ws
            ops.adam_step_parts_raw(p, grad, m, v, step, n, ADAM["lr"], ADAM["b1"], ADAM["b2"], parts, stride, n_parts, enc, per, covered,
                                    ADAM["eps"], ADAM["wd"], ADAM["gscale"])
        else:
            ops.encoder_bwd_raw(fw.cfg, 0, L, dx, p, grad, fw.saved, fw.ws, fw.rng, ENC_ADD, True)
            ops.adam_step_raw(p, grad, m, v, step, n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], ADAM["gscale"])
        torch.cuda.synchronize()
        res.append((p.cpu(), m.cpu(), v.cpu(), step.cpu(), dx.cpu()))
    (pa, ma, va, sa, da), (pb, mb, vb, sb, db) = res
    for t in (pa, ma, va, da):
        assert bool(torch.isfinite(t).all())
    assert int(sa) == int(sb) == 4
    assert RC.same_bits(da, db)
    assert RC.same_bits(ma, mb) and RC.same_bits(va, vb) and RC.same_bits(pa, pb)
    assert not bool((pa == p0).all()) and float((ma[:enc] - m0[:enc] * ADAM["b1"]).abs().max()) > 0      # the step did something
