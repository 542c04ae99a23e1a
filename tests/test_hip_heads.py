"""ganffn_head_fwd / ganffn_head_bwd alone against the fp64 head oracle (tests/head_oracle.py), both kinds, at the widths and
token counts at which the code takes another path:

  generator      the two EPI_DROP_GELU products and the EPI_GELU_BWD_DROP products behind them: on the generic 64 x 64 kernel
                 (full and partial tiles, K <= 128 and above, N % 64 != 0, K % 16 != 0) and, at E = 100 with D1 >= 1024, on the
                 persistent weight-resident kernel — which the workload only ever sends the ReLU epilogues;
  discriminator  csrc/disc_head.hip at (100, 64, 16): 4 tokens per wave, 16 per workgroup — T = 1, T < 4, workgroups whose
                 waves 1..3 are all inactive, one partial row more than the 64 lanes of the fc3 reduce (T = 1029); the
                 unfused sequence (GELU pass, two products, disc_tail_fwd / _bwd / _reduce) at every other width, at 65
                 tail blocks (T = 16389), and at (100, 64, 16) under bit 5 of the debug mode word.

Every case: output, dx, saved and workspace start as NaN, the gradient buffers from seeded non-zero values (the reference is
initial + gradient), the rng is {seed > 2^32, offset 3} with rng_offset_add 11.  Three modes each: train with p = 0.2, train
with p = 0, eval with p = 0.2 (= the dropout-free oracle).  Asserted: out, dx and every parameter gradient against the
oracle; a second forward + backward gives the same bits; in train mode the zero pattern of the output is exactly the Philox
contract's; all gradient pointers NULL gives the bits of dx, weight gradients without bias gradients the bits of gw1 / gw2.

Bounds, as in tests/test_hip_dispatch_range.py.  Metric: tests/test_hip_ops.py rel_err (largest absolute error over largest
absolute reference value).  Nobody has measured these kernels alone, so the yardstick is the oracle itself in fp32 on the CPU
on the same inputs and masks: its error against fp64 is what fp32 arithmetic costs on that input.
bound = max(floor, 8 x that error); floor = the project's GEMM tolerance for the quantity's longest reduction,
2e-6 * max(1, sqrt(max(E, D1, D2))) for out and dx, 3e-6 * max(1, sqrt(T)) for the parameter gradients; the factor 8 allows
for another summation order and erff / __expf.  The module's report line prints the largest error / bound ratio per quantity.

The saturation case is held to two references.  First the plain one: the fp64 chain head -> BCELoss -> backward with torch's
BCELoss semantics (log clamped at -100 forward, p (1 - p) clamped at 1e-12 backward), bounds as above.  There the fp32
yardstick is large by construction — a probability that rounds to 1.0 in fp32 has p (1 - p) = 0 and passes no gradient, in the
kernel as in the fp32 oracle (23 of the 64 tokens) — so for dx and the gradients that comparison is NOT a check (its bound is
8 x 0.06 - 0.9 relative: it would pass almost anything finite); it is kept as the statement it is, and only its `out` row
binds.  The comparison that carries the case is the second: the chain behind the device's OWN fp32 probabilities (d_u3 = dprob(p) p (1 - p) from them,
then the head's backward from its logits): both oracles then agree on which tokens pass no gradient, the yardstick is back
at 4e-7, and the bounds are the floors.  Besides: nothing is NaN or inf, and the loss is the fp64 BCE of those probabilities.

Largest error / bound on an MI355X when the module was added (the case that gave it):
  generator      out 0.061 and dx 0.052 (33, 4, 4, 4); gw1 0.097, gb2 0.134, gw2 0.131 (1, 100, 1024, 100); gb1 0.080 (1, 100, 512, 100)
  discriminator  out 0.037 and dx 0.040 (16389, 4, 4, 4); gw1 0.018, gb1 0.015 (1, 100, 64, 16); gw2 0.024, gb2 0.018
                 (4, 100, 64, 16); gw3 0.044 (70, 512, 64, 16); gb3 0.125 (16, 100, 64, 16: the one quantity whose bound is
                 8 x the fp32 oracle's error, 1.2e-5, and not the floor)
  saturated      against the fp64 chain: out 0.026, dx and every gradient 0.125 (error 0.06 - 0.9 relative, the fp32 oracle's
                 own); behind the device's probabilities: out 0.026, dx 0.019, gradients 0.0003 - 0.011
Everywhere else the bound is the floor or within a factor 1.1 of it: the kernels sit at 2 - 13 % of the project's GEMM tolerances.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import head_cases as HC
import head_oracle as HO
from oracle import ganffn_oracle as O
from oracle import philox
from test_hip_ops import lib, ptr, rel_err, stream  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

SEED, OFF, ADD = (5 << 32) + 20261019, 3, 11
MODES = [(1, 0.2), (1, 0.0), (0, 0.2)]               # (train, p)
MODE_IDS = ["train-p0.2", "train-p0", "eval-p0.2"]
WORST = {}        # quantity -> largest error / bound seen in this module (printed at its end)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nhead checks, largest error / bound per quantity: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _bounded(fails, what, err, bound, tag):
    WORST[what] = max(WORST.get(what, 0.0), err / bound)
    print("%s %s: error %.3e, bound %.3e" % (what, tag, err, bound))
    if not err <= bound:                                   # (a NaN fails too)
        fails.append((what, tag, err, bound))


def _expect(fails, cond, what, tag):
    if not cond:
        fails.append((what, tag))


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, train, p):
    """inputs, and the oracle in fp64 and in fp32 on them (computed once per case, never modified)"""
    tensors, d_out, g0 = HC.head_inputs(kind, *shape)
    rng = O.Rng(SEED, OFF + ADD, bool(train))
    o64, g64 = HO.head_run(kind, tensors, d_out, p, rng)
    o32, g32 = HO.head_run(kind, tensors, d_out, p, rng, dtype=torch.float32)
    return tensors, d_out, g0, (o64, g64, o32, g32)


def _nan(n):
    return torch.full((max(int(n), 1),), float("nan"), device="cuda")


def _launch(kind, shape, train, p, dt, d_out_d, g0, which="all"):
    """one ganffn_head_fwd + ganffn_head_bwd from NaN-filled out / dx / saved / workspace and fresh copies of the initial
    gradients.  which: "all" gradient pointers | "none" (all NULL) | "weights" (gw1, gw2 only) -> (out, dx, {name: grad})"""
    from gan_ffn_amd import ops
    T, E, D1, D2 = shape
    cfg = ops.head_cfg(T, E, D1, D2, kind, p, bool(train))
    n_saved, n_ws = ops.head_sizes(cfg)
    out, dx, saved, ws = _nan(T * (D2 if kind == HO.GEN else 1)), _nan(T * E), _nan(n_saved), _nan(n_ws)
    assert ws.data_ptr() % 16 == 0
    keys = {"all": HO.GRAD_KEYS, "none": (), "weights": ("w1", "w2")}[which]
    G = {k: g0[k].cuda().clone() for k in keys if k in g0}
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    x, w1, b1, w2, b2, w3, b3 = dt
    ops.head_fwd_raw(cfg, x, w1, b1, w2, b2, w3, b3, out, saved, ws, rng, ADD)
    ops.head_bwd_raw(cfg, d_out_d, x, w1, w2, w3, G.get("w1"), G.get("b1"), G.get("w2"), G.get("b2"), G.get("w3"), G.get("b3"),
                     dx, saved, ws, rng, ADD)
    torch.cuda.synchronize()
    return out.view(T, -1), dx.view(T, E), G


def _compare(fails, kind, shape, tag, got, g0, refs, who=None):
    """out, dx and the accumulated parameter gradients against fp64, each bounded by its floor and the fp32 oracle's error"""
    out, dx, G = got
    o64, g64, o32, g32 = refs
    T, E, D1, D2 = shape
    floor_a, floor_g = 2e-6 * max(1.0, math.sqrt(max(E, D1, D2))), 3e-6 * max(1.0, math.sqrt(T))
    who = who or ("gen" if kind == HO.GEN else "disc")
    items = [("out", out, o64, o32, floor_a), ("dx", dx, g64["x"], g32["x"], floor_a)]
    items += [("g" + k, G[k], g0[k].double() + g64[k], g0[k] + g32[k], floor_g) for k in HO.GRAD_KEYS if k in G]
    for name, have, r64, r32, floor in items:
        _expect(fails, have.shape == r64.shape, "shape of " + name, tag)
        _bounded(fails, "%s %s" % (who, name), rel_err(have.reshape(r64.shape), r64), max(floor, 8.0 * rel_err(r32, r64)), tag)


def _head_case(kind, shape, train, p):
    T, E, D1, D2 = shape
    tag = "%s train=%d p=%g" % (shape, train, p)
    tensors, d_out, g0, refs = _reference(kind, shape, train, p)
    dt = tuple(None if t is None else t.cuda() for t in tensors)
    d_out_d = d_out.cuda()
    fails = []
    out, dx, G = _launch(kind, shape, train, p, dt, d_out_d, g0)
    assert sorted(G) == sorted(g0)
    _compare(fails, kind, shape, tag, (out, dx, G), g0, refs)
    # the same state again: the same bits
    out2, dx2, G2 = _launch(kind, shape, train, p, dt, d_out_d, g0)
    _expect(fails, torch.equal(out, out2) and torch.equal(dx, dx2), "second run: out / dx bits", tag)
    for k in G:
        _expect(fails, torch.equal(G[k], G2[k]), "second run: g%s bits" % k, tag)
    # the zero pattern of the Philox contract
    # (and nowhere else, short of fp32 itself: a kept output may still read exactly 0 / 0.5 where 1 + erff(u / sqrt 2) or the
    #  sigmoid rounds there — gelu(u) beyond u = -5.4 is below 2e-7 — so a kept one must be within 1e-6 of it in fp64)
    if train and p > 0:
        site, width, idle = (O.SITE_HEAD2, D2, 0.0) if kind == HO.GEN else (O.SITE_HEAD3, 1, 0.5)
        keep = torch.from_numpy(philox.keep_mask(T, width, p, site, SEED, OFF + ADD))
        at_idle = (out == idle).cpu()
        _expect(fails, bool(at_idle[~keep].all()), "out exactly %g wherever the contract's mask drops" % idle, tag)
        stray = at_idle & keep
        _expect(fails, not bool(stray.any()) or float((refs[0][stray] - idle).abs().max()) < 1e-6,
                "a kept output reads exactly %g where fp64 does not" % idle, tag)
    # NULL-gradient forms
    out3, dx3, _ = _launch(kind, shape, train, p, dt, d_out_d, g0, which="none")
    _expect(fails, torch.equal(dx3, dx) and torch.equal(out3, out), "all gradient pointers NULL: dx bits", tag)
    _, dx4, G4 = _launch(kind, shape, train, p, dt, d_out_d, g0, which="weights")
    _expect(fails, sorted(G4) == ["w1", "w2"] and torch.equal(G4["w1"], G["w1"]) and torch.equal(G4["w2"], G["w2"]),
            "gw1, gw2 without gb1, gb2: gw bits", tag)
    _expect(fails, torch.equal(dx4, dx), "gw1, gw2 without gb1, gb2: dx bits", tag)
    assert not fails, fails


# (1, 100, 1024, 100) and (67, ..): K = 100, N >= 1024 -> gemm_wres_kernel with EPI_DROP_GELU forward (one partial tile / one
# full tile + a 3-row tile) and EPI_GELU_BWD_DROP backward; (33, 4, 4, 4): everything at its minimum; (70, 68, 132, 36):
# N % 64 != 0, K % 16 != 0, K <= 128 on one product but not the other; (9, 128, 60, 200): D2 > D1
@pytest.mark.parametrize("train,p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", HC.GEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_generator_head(shape, train, p):
    _head_case(HO.GEN, shape, train, p)


# T -> workgroups / partial rows of csrc/disc_head.hip: 1, 3: one wave, a partial row group; 4, 5: the second wave starts;
# 15, 16, 17: the second workgroup starts, its waves 1..3 all inactive at 17; 63, 330: ragged tails; 1029: 65 partial rows
@pytest.mark.parametrize("train,p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", HC.DISC_FUSED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_discriminator_head_fused(shape, train, p):
    _head_case(HO.DISC, shape, train, p)


# (5, 100, 64, 32): D2 at its bound; (257, 64, 16, 4): two tail blocks; (16389, 4, 4, 4): 65 tail blocks (the reduce's lanes
# take a second stride), 65 k floats per operand
@pytest.mark.parametrize("train,p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", HC.DISC_UNFUSED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_discriminator_head_unfused_by_width(shape, train, p):
    _head_case(HO.DISC, shape, train, p)


# dx = d_pre1 W1 under EPI_GELU_BWD on the generic kernel (K = D1 = 132) and on the weight-resident one (K = 100, N = E = 1024)
@pytest.mark.parametrize("train,p", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", HC.DISC_PLAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_discriminator_head_dx_past_the_short_k_class(shape, train, p):
    _head_case(HO.DISC, shape, train, p)


@pytest.mark.parametrize("train,p", MODES, ids=MODE_IDS)
def test_discriminator_head_unfused_by_mode_bit_at_the_fused_widths(train, p):
    """bit 5 of the debug mode word: the separate launches at (100, 64, 16), held to the same fp64 bounds as the fused kernel
    (the header promises no bit equality between the two)"""
    from gan_ffn_amd import _lib
    _lib.load().ganffn_debug_set_ffn_mode(1 << 5)
    try:
        _head_case(HO.DISC, (330, 100, 64, 16), train, p)
    finally:
        _lib.load().ganffn_debug_set_ffn_mode(0)


def test_saturated_discriminator_through_bce(lib):
    """eval mode, (64, 100, 64, 16), fc3 scaled (on the CPU oracle) so that its pre-activation spans +-40: fp32 probabilities
    reach exactly 1.0 and go down to ~1e-18.  ganffn_bce2_fwd (period 2, split 1, targets 1 / 0) -> ganffn_bce2_bwd ->
    ganffn_head_bwd: p (1 - p) underflows to 0 on one side and sits far below the 1e-12 clamp of the BCE backward on the other"""
    from gan_ffn_amd import ops
    import torch.nn.functional as F
    kind, shape, p = HO.DISC, (64, 100, 64, 16), 0.2
    T, E, D1, D2 = shape
    tensors, _, g0 = HC.head_inputs(kind, *shape, seed=1)
    x, w1, b1, w2, b2, w3, b3 = tensors
    with torch.no_grad():
        a2 = HO.head_forward(HO.GEN, x, w1, b1, w2, b2, p=p, rng=None)              # eval: the discriminator's a2 (fp64)
        s = (a2 @ w3.double().T).squeeze(1)
        scale = 80.0 / float(s.max() - s.min())
        w3 = (w3.double() * scale).float()
        b3 = torch.tensor([-(float(s.max()) + float(s.min())) / 2 * scale])
        pre3 = (a2 @ w3.double().T + b3.double()).squeeze(1)
    assert 39.0 < float(pre3.max()) < 41.0 and -41.0 < float(pre3.min()) < -39.0
    tensors = (x, w1, b1, w2, b2, w3, b3)
    y = (torch.arange(T) % 2 < 1).double().view(T, 1)                                  # period 2, split 1: 1, 0, 1, 0, ..

    refs = []
    for dtype in (torch.float64, torch.float32):
        o, g = HO.head_run(kind, tensors, None, p, None, dtype=dtype, loss=lambda out: F.binary_cross_entropy(out, y.to(out.dtype)))
        refs += [o, g]
    assert all(bool(torch.isfinite(t).all()) for t in refs[1].values())

    dt = tuple(t.cuda() for t in tensors)
    cfg = ops.head_cfg(T, E, D1, D2, kind, p, False)
    n_saved, n_ws = ops.head_sizes(cfg)
    prob, dx, saved, ws, dprob, loss = _nan(T), _nan(T * E), _nan(n_saved), _nan(n_ws), _nan(T), _nan(1)
    G = {k: v.cuda().clone() for k, v in g0.items()}
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    ops.head_fwd_raw(cfg, *dt, prob, saved, ws, rng, ADD)
    lib.call("ganffn_bce2_fwd", ptr(prob), C.c_float(1.0), C.c_float(0.0), 2, 1, T, C.c_float(1.0), ptr(loss), 0, stream())
    lib.call("ganffn_bce2_bwd", ptr(prob), C.c_float(1.0), C.c_float(0.0), 2, 1, T, C.c_float(1.0), ptr(dprob), stream())
    ops.head_bwd_raw(cfg, dprob, dt[0], dt[1], dt[3], dt[5], G["w1"], G["b1"], G["w2"], G["b2"], G["w3"], G["b3"], dx, saved, ws,
                     rng, ADD)
    torch.cuda.synchronize()
    ph = prob.cpu()
    print("saturated head: prob in [%.3e, %.9g], %d exactly 1.0, loss %.6f" % (float(ph.min()), float(ph.max()), int((ph == 1).sum()), float(loss)))
    assert float(ph.max()) == 1.0 and 0.0 < float(ph.min()) < 1e-16
    for t in [prob, loss, dprob, dx] + list(G.values()):
        assert bool(torch.isfinite(t).all())
    loss_ref = float(F.binary_cross_entropy(ph.double().view(T, 1), y))
    assert abs(float(loss) - loss_ref) <= 1e-5 * abs(loss_ref), (float(loss), loss_ref)
    fails = []
    got = (prob.view(T, 1), dx.view(T, E), G)
    _compare(fails, kind, shape, "saturated", got, g0, refs, who="saturated")
    # the same with the saturation taken out of the yardstick: the chain behind the device's OWN fp32 probabilities —
    # d_u3 = dprob(p) * p (1 - p) from them (1 - p is exact in fp32 for p >= 0.5), then the head's backward from its logits.
    # Both the fp64 and the fp32 oracle now agree on which tokens pass no gradient, and the bounds are the floors again.
    given = []
    for dtype in (torch.float64, torch.float32):
        pv, yv = ph.to(dtype).view(T, 1), y.to(dtype)
        q = pv * (1 - pv)
        d_u3 = (pv - yv) / q.clamp_min(torch.tensor(1e-12, dtype=dtype)) / T * q
        u3, g = HO.head_run(kind, tensors, d_u3, p, None, dtype=dtype, logits=True)
        given += [torch.sigmoid(u3), g]
    _compare(fails, kind, shape, "saturated, behind the device's probabilities", got, g0, given, who="saturated-given-prob")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def _filled(n=1 << 14):
    return torch.full((n,), -7.0, device="cuda")


# (kind, T, E, D1, D2, p) -> the value the message must name
BAD_CFGS = [((1, 8, 100, 64, 36, 0.2), "D2=36"), ((0, 8, 100, 6, 16, 0.2), "D1=6"), ((1, 8, 6, 64, 16, 0.2), "E=6"),
            ((0, 0, 100, 64, 16, 0.2), "T=0"), ((2, 8, 100, 64, 16, 0.2), "kind=2"), ((1, 8, 100, 64, 16, 1.0), "p=1")]


@pytest.mark.parametrize("bad,what", BAD_CFGS, ids=[w for _, w in BAD_CFGS])
def test_bad_head_cfg_is_refused_by_name_and_nothing_is_written(bad, what):
    """both size functions and both calls: GanffnError naming the offending value; a -7 fill survives in every buffer"""
    from gan_ffn_amd import _lib, ops
    from gan_ffn_amd._lib import GanffnError
    kind, T, E, D1, D2, p = bad
    cfg = ops.head_cfg(T, E, D1, D2, kind, p, True)
    L = _lib.load()
    for fn in (L.ganffn_head_saved_floats, L.ganffn_head_workspace_floats):
        assert int(fn(C.byref(cfg))) == -1
        assert what in L.ganffn_last_error().decode()
    with pytest.raises(GanffnError, match=what):
        ops.head_sizes(cfg)
    bufs = {k: _filled() for k in ("x", "w1", "b1", "w2", "b2", "w3", "b3", "out", "saved", "ws", "d_out", "dx", "gw1", "gb1",
                                   "gw2", "gb2", "gw3", "gb3")}
    b = bufs
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    with pytest.raises(GanffnError, match=what):
        ops.head_fwd_raw(cfg, b["x"], b["w1"], b["b1"], b["w2"], b["b2"], b["w3"], b["b3"], b["out"], b["saved"], b["ws"], rng, ADD)
    with pytest.raises(GanffnError, match=what):
        ops.head_bwd_raw(cfg, b["d_out"], b["x"], b["w1"], b["w2"], b["w3"], b["gw1"], b["gb1"], b["gw2"], b["gb2"], b["gw3"],
                         b["gb3"], b["dx"], b["saved"], b["ws"], rng, ADD)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == -7).all()), k


# a bias gradient without its weight gradient (silently not accumulated before), and gw3 without gb3 (refused only after the
# fused backward kernel had written dx and the workspace): refused before the first launch
PAIRINGS = [("gw1", "gb1 given without gw1"), ("gw2", "gb2 given without gw2"), ("gw3", "gb3 given without gw3"),
            ("gb3", "gw3 given without gb3")]


@pytest.mark.parametrize("shape", [(1, 16, 100, 64, 16), (1, 16, 100, 128, 16), (0, 16, 100, 512, 100)],
                         ids=["disc-fused", "disc-unfused", "gen"])
@pytest.mark.parametrize("missing,what", PAIRINGS, ids=[m for m, _ in PAIRINGS])
def test_unpaired_head_gradient_pointers_are_refused_before_any_launch(shape, missing, what):
    from gan_ffn_amd import ops
    from gan_ffn_amd._lib import GanffnError
    kind, T, E, D1, D2 = shape
    cfg = ops.head_cfg(T, E, D1, D2, kind, 0.2, True)
    n_saved, n_ws = ops.head_sizes(cfg)
    assert max(n_saved, n_ws, D1 * E) <= 1 << 17
    bufs = {k: _filled(1 << 17) for k in ("x", "w1", "w2", "w3", "saved", "ws", "d_out", "dx", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3")}
    b = bufs
    g = {k: (None if k == missing else b[k]) for k in ("gw1", "gb1", "gw2", "gb2", "gw3", "gb3")}
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    with pytest.raises(GanffnError, match=what):
        ops.head_bwd_raw(cfg, b["d_out"], b["x"], b["w1"], b["w2"], b["w3"], g["gw1"], g["gb1"], g["gw2"], g["gb2"], g["gw3"],
                         g["gb3"], b["dx"], b["saved"], b["ws"], rng, ADD)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == -7).all()), k
