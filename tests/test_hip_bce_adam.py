"""ganffn_bce2_fwd / _bwd and the Adam entry points (ganffn_adam_step, _update + _bump, _step_parts) alone.

BCE: the reference is torch.nn.functional.binary_cross_entropy under autograd in fp64 with an explicit target tensor, on the
fp32 probabilities the kernel reads.  Loss to 1e-5 relative (the bound of tests/test_hip_ops.py::test_bce_edge_cases_and_backward);
dprob to rel_err < 1e-5 AND to 1e-5 of every single element — the kernel's expression is six correctly rounded fp32
operations on exact fp32 inputs (p - y, 1 - p, p (1 - p), scale / n, a product, a quotient: < 4e-7 relative in all), and
max(p (1 - p), 1e-12) is continuous, so an element AT the clamp (the planted 1e-12, whose fp32 and fp64 products sit 4e-9
apart on either side of it) is compared like every other: nothing is skipped.
What these bounds do NOT hold (tests/bce_cases.py and tests/test_bce_inputs_cpu.py say why): the elementwise assertion carries
one absolute term, UNDERFLOW = 1e-33, and the planted denormal with target 0 has a reference of 1.4e-33 scale / n, below it —
that one element is unchecked at every n (fp32 may flush it).  rel_err < 1e-5 is kept because the project's metric is that,
but with 0.0 or 1.0 planted the largest reference value is 1e12 / n and it says little: the elementwise assertion is the
check that does the work.  At n = 5 two clamped terms of 100 dominate the loss, so the 1e-5 relative bound holds the one
seeded term to about 0.2 % only; n = 1 (a seeded value alone) and n >= 1023 hold the seeded terms tightly.

Adam: the reference is oracle.ganffn_oracle.Adam in fp64, given the fp32 values of the hyper-parameters the kernel receives;
3e-7 absolute on parameters in (-1, 1) as in test_adam_matches_reference_fixture.  The other statements are bit equalities
between call shapes the header documents as identical."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

from bce_cases import BCE_N, BCE_PERIODS, BCE_TARGETS, UNDERFLOW, bce_probs, bce_targets, f32
from oracle import ganffn_oracle as O
from test_hip_ops import lib, ptr, rel_err, stream  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------------
# BCE
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period,split", BCE_PERIODS)
@pytest.mark.parametrize("n", BCE_N)
def test_bce2_forward_and_backward(lib, n, period, split):
    p, _ = bce_probs(n)
    pd = p.cuda()
    for (ta, tb), scale in itertools.product(BCE_TARGETS, (1.0, 0.5)):
        y = bce_targets(n, period, split, ta, tb)
        p64 = p.double().requires_grad_(True)
        ref = F.binary_cross_entropy(p64, y) * scale
        (gref,) = torch.autograd.grad(ref, p64)
        ref = float(ref)
        tag = "n=%d period=%d split=%d targets=(%g, %g) scale=%g" % (n, period, split, ta, tb, scale)
        for accumulate in (0, 1):
            want = ref + 0.25 if accumulate else ref
            loss = torch.full((1,), 0.25, device="cuda")
            lib.call("ganffn_bce2_fwd", ptr(pd), C.c_float(ta), C.c_float(tb), period, split, n, C.c_float(scale), ptr(loss),
                     accumulate, stream())
            again = torch.full((1,), 0.25, device="cuda")
            lib.call("ganffn_bce2_fwd", ptr(pd), C.c_float(ta), C.c_float(tb), period, split, n, C.c_float(scale), ptr(again),
                     accumulate, stream())
            print("bce2_fwd %s accumulate=%d: loss %.9g, fp64 %.9g" % (tag, accumulate, float(loss), want))
            assert abs(float(loss) - want) <= 1e-5 * abs(want), (tag, accumulate, float(loss), want)
            assert torch.equal(loss, again), tag
        d = torch.full((n,), float("nan"), device="cuda")
        lib.call("ganffn_bce2_bwd", ptr(pd), C.c_float(ta), C.c_float(tb), period, split, n, C.c_float(scale), ptr(d), stream())
        dh = d.cpu().double()
        nz = gref != 0
        worst = float(((dh - gref).abs()[nz] / gref.abs()[nz]).max()) if bool(nz.any()) else 0.0
        print("bce2_bwd %s: rel_err %.3e, largest elementwise relative error %.3e" % (tag, rel_err(d, gref), worst))
        assert bool(torch.isfinite(dh).all()), tag
        assert rel_err(d, gref) < 1e-5, tag            # (the project's metric; next to a planted 0.0 / 1.0 it says little)
        assert bool(((dh - gref).abs() <= 1e-5 * gref.abs() + UNDERFLOW).all()), tag      # the check that does the work


@pytest.mark.parametrize("n", BCE_N)
def test_bce_constant_target_is_bce2_with_equal_targets(lib, n):
    p, _ = bce_probs(n)
    pd = p.cuda()
    for target, scale, accumulate in itertools.product((1.0, 0.0, 0.9), (1.0, 0.5), (0, 1)):
        a, b = torch.full((1,), 0.25, device="cuda"), torch.full((1,), 0.25, device="cuda")
        lib.call("ganffn_bce_fwd", ptr(pd), C.c_float(target), n, C.c_float(scale), ptr(a), accumulate, stream())
        lib.call("ganffn_bce2_fwd", ptr(pd), C.c_float(target), C.c_float(target), 0, 0, n, C.c_float(scale), ptr(b), accumulate, stream())
        assert torch.equal(a, b), (n, target, scale, accumulate)
        da, db = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        lib.call("ganffn_bce_bwd", ptr(pd), C.c_float(target), n, C.c_float(scale), ptr(da), stream())
        lib.call("ganffn_bce2_bwd", ptr(pd), C.c_float(target), C.c_float(target), 0, 0, n, C.c_float(scale), ptr(db), stream())
        assert torch.equal(da, db), (n, target, scale)


# ------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------
ADAM_HYPERS = [(1e-4, 0.5, 0.6, 0.0, 1.0), (1e-4, 0.9, 0.999, 0.008, 1.0), (1e-3, 0.9, 0.999, 0.008, 0.125)]   # lr, b1, b2, wd, grad_scale
ADAM_N, ADAM_STEPS = 1031, 3


def adam_inputs(n, start, steps=ADAM_STEPS, seed=0):
    """parameters in (-1, 1), one gradient per step, and the state a run that is `start` steps old would hold"""
    g = torch.Generator().manual_seed(77 + n + 1000 * start + seed)
    p = torch.rand(n, generator=g) * 2 - 1
    grads = [torch.randn(n, generator=g) for _ in range(steps)]
    if start == 0:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    return p, grads, m, v


class Slabs:
    """p, g, m, v on the device, `shift` floats into their allocations (shift 1: no pointer is 16-byte aligned), + the counter"""

    def __init__(self, p, m, v, start, shift=0):
        n = p.numel()
        self.n, self.bufs = n, {}
        for k, t in (("p", p), ("g", torch.zeros(n)), ("m", m), ("v", v)):
            buf = torch.full((n + 8,), float("nan"), device="cuda")
            assert buf.data_ptr() % 16 == 0
            view = buf[shift:shift + n]
            view.copy_(t)
            self.bufs[k] = buf
            setattr(self, k, view)
        self.step = torch.tensor([start], dtype=torch.int32, device="cuda")

    def state(self):
        torch.cuda.synchronize()
        return self.p.clone(), self.m.clone(), self.v.clone(), int(self.step)


def _adam_args(s, n, hyp, lo=0):
    lr, b1, b2, wd, gs = hyp
    return (ptr(s.p[lo:]), ptr(s.g[lo:]), ptr(s.m[lo:]), ptr(s.v[lo:]), ptr(s.step), C.c_int64(n), C.c_float(lr), C.c_float(b1),
            C.c_float(b2), C.c_float(1e-8), C.c_float(wd), C.c_float(gs))


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("start", [0, 41])
@pytest.mark.parametrize("hyp", ADAM_HYPERS, ids=["gan", "phase2", "phase2-scaled"])
def test_adam_step_matches_the_fp64_oracle(lib, hyp, start):
    lr, b1, b2, wd, gs = hyp
    p, grads, m, v = adam_inputs(ADAM_N, start)
    ref_p = p.double().clone().requires_grad_(True)
    opt = O.Adam([ref_p], f32(lr), (f32(b1), f32(b2)), eps=f32(1e-8), weight_decay=f32(wd))
    opt.state[id(ref_p)] = {"t": start, "m": m.double().clone(), "v": v.double().clone()}
    s = Slabs(p, m, v, start)
    for i, g in enumerate(grads):
        s.g.copy_(g)
        lib.call("ganffn_adam_step", *_adam_args(s, ADAM_N, hyp), stream())
        ref_p.grad = g.double() * f32(gs)
        opt.step()
        got_p, got_m, got_v, t = s.state()
        st = opt.state[id(ref_p)]
        err = float((got_p.cpu().double() - ref_p.detach()).abs().max())
        print("adam %s start=%d step %d: |p - fp64| %.3e, m rel %.3e, v rel %.3e" % (hyp, start, i, err, rel_err(got_m, st["m"]), rel_err(got_v, st["v"])))
        assert t == start + i + 1 == st["t"]
        assert err <= 3e-7
        # m and v: two products and a sum per step in fp32 (< 2e-7 relative each), three steps
        assert rel_err(got_m, st["m"]) < 1e-5 and rel_err(got_v, st["v"]) < 1e-5


@pytest.mark.parametrize("start", [0, 41])
@pytest.mark.parametrize("hyp", ADAM_HYPERS, ids=["gan", "phase2", "phase2-scaled"])
def test_adam_call_shapes_give_the_bits_of_one_adam_step(lib, hyp, start):
    """a base pointer one float into the allocation (every element on the scalar kernel), and ganffn_adam_update over three
    slices followed by one ganffn_adam_bump (the first slice ends off a 16-byte boundary, so the second is scalar too)"""
    p, grads, m, v = adam_inputs(ADAM_N, start)
    whole, shifted, sliced = Slabs(p, m, v, start), Slabs(p, m, v, start, shift=1), Slabs(p, m, v, start)
    assert whole.p.data_ptr() % 16 == 0 and shifted.p.data_ptr() % 16 == 4
    for g in grads:
        for s in (whole, shifted, sliced):
            s.g.copy_(g)
        lib.call("ganffn_adam_step", *_adam_args(whole, ADAM_N, hyp), stream())
        lib.call("ganffn_adam_step", *_adam_args(shifted, ADAM_N, hyp), stream())
        for lo, hi in ((0, 257), (257, 700), (700, ADAM_N)):
            lib.call("ganffn_adam_update", *_adam_args(sliced, hi - lo, hyp, lo=lo), stream())
        lib.call("ganffn_adam_bump", ptr(sliced.step), stream())
        ref = whole.state()
        assert _same(shifted.state(), ref), "unaligned base pointer"
        assert _same(sliced.state(), ref), "update on slices + bump"
    assert int(whole.step) == start + len(grads)
    for s in (whole, shifted, sliced):            # nothing outside the views was written
        for k, buf in s.bufs.items():
            lo = 1 if s is shifted else 0
            assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + ADAM_N:]).all()), k


PARTS_GEOM = dict(n=256, layer_floats=64, covered=40, enc_floats=192)


def _parts(n_parts, part_stride, seed):
    """(n_parts - 1) chunks of part_stride floats: seeded values on the covered elements, NaN everywhere else"""
    G = PARTS_GEOM
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(G["n"])
    cov = ((i < G["enc_floats"]) & ((i % G["layer_floats"]) < G["covered"])).nonzero().squeeze(1)     # covered slab indices
    assert int(cov.max()) < G["enc_floats"] <= part_stride
    parts = torch.full((n_parts - 1, part_stride), float("nan"))
    parts[:, cov] = torch.randn(n_parts - 1, cov.numel(), generator=g)
    return parts, cov


@pytest.mark.parametrize("part_stride", [192, 200])
@pytest.mark.parametrize("n_parts", [2, 5, 8])
def test_adam_step_parts_is_adam_step_on_the_chunk_sum(lib, n_parts, part_stride):
    """the gradient of a covered element is ((g + part_0) + part_1) + ... in fp32, in chunk order; every other element of the
    chunks holds NaN, so a read outside the covered set shows in the result"""
    from gan_ffn_amd import ops
    G = PARTS_GEOM
    n = G["n"]
    for hyp, start in itertools.product(ADAM_HYPERS, (0, 41)):
        lr, b1, b2, wd, gs = hyp
        p, grads, m, v = adam_inputs(n, start, steps=2, seed=n_parts)
        direct, summed = Slabs(p, m, v, start), Slabs(p, m, v, start)
        for k, g in enumerate(grads):
            parts, cov = _parts(n_parts, part_stride, 100 * n_parts + part_stride + k)
            assert cov.numel() == 3 * G["covered"]
            gsum = g.clone()
            for z in range(n_parts - 1):
                gsum[cov] = gsum[cov] + parts[z][cov]
            assert bool(torch.isfinite(gsum).all())
            pd = parts.cuda().contiguous()
            direct.g.copy_(g)
            summed.g.copy_(gsum)
            ops.adam_step_parts_raw(direct.p, direct.g, direct.m, direct.v, direct.step, n, lr, b1, b2, pd, part_stride, n_parts,
                                    G["enc_floats"], G["layer_floats"], G["covered"], wd=wd, gscale=gs)
            lib.call("ganffn_adam_step", *_adam_args(summed, n, hyp), stream())
            got, ref = direct.state(), summed.state()
            assert bool(torch.isfinite(got[0]).all())
            assert _same(got, ref), (hyp, start, k)


def test_adam_step_parts_with_one_part_is_adam_step(lib):
    from gan_ffn_amd import ops
    hyp = ADAM_HYPERS[2]
    lr, b1, b2, wd, gs = hyp
    p, grads, m, v = adam_inputs(ADAM_N, 41)
    a, b = Slabs(p, m, v, 41), Slabs(p, m, v, 41)
    for g in grads:
        a.g.copy_(g)
        b.g.copy_(g)
        ops.adam_step_parts_raw(a.p, a.g, a.m, a.v, a.step, ADAM_N, lr, b1, b2, None, 0, 1, 0, 0, 0, wd=wd, gscale=gs)
        lib.call("ganffn_adam_step", *_adam_args(b, ADAM_N, hyp), stream())
        assert _same(a.state(), b.state())


# (n, part_stride, n_parts, enc_floats, layer_floats, covered)
# why -> ((n, part_stride, n_parts, enc_floats, layer_floats, covered), the text only that refusal's message carries)
PARTS_REFUSALS = {"n_parts=9": ((256, 192, 9, 192, 64, 40), "n_parts=9"),
                  "part_stride < enc_floats": ((256, 188, 2, 192, 64, 40), "bad partial slabs"),
                  "n % 4 != 0": ((258, 192, 2, 192, 64, 40), "multiple of 4"),
                  "covered > layer_floats": ((256, 192, 2, 192, 64, 68), "bad layer geometry"),
                  "enc_floats % layer_floats != 0": ((256, 200, 2, 196, 64, 40), "bad layer geometry")}


@pytest.mark.parametrize("why", sorted(PARTS_REFUSALS))
def test_adam_step_parts_refusals_leave_slabs_and_counter_untouched(lib, why):
    from gan_ffn_amd import ops
    from gan_ffn_amd._lib import GanffnError
    (n, part_stride, n_parts, enc_floats, layer_floats, covered), what = PARTS_REFUSALS[why]
    p, g, m, v, parts = (torch.full((4096,), -7.0, device="cuda") for _ in range(5))
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    with pytest.raises(GanffnError, match=what):
        ops.adam_step_parts_raw(p, g, m, v, step, n, 1e-4, 0.9, 0.999, parts, part_stride, n_parts, enc_floats, layer_floats, covered)
    torch.cuda.synchronize()
    assert int(step) == 5
    for t in (p, g, m, v, parts):
        assert bool((t == -7).all())
