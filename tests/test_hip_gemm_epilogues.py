"""ganffn_gemm_hook and ganffn_ffn_k100_hook alone against fp64 references of their own (tests/gemm_epi_cases.py): the three
epilogues of the generic 64 x 64 kernel in both operand modes and on both instantiations (K <= 128 and above), the split-K
slab layout, and the 1-bit ReLU / dropout pattern that linear1's epilogue writes and the linear2 dgrad reads.

Shapes: M in {1, 33, 64, 97, 130}, N in {4, 36, 64, 100, 132}, K in {4, 68, 128, 132, 516} — wave tiles wholly inside the
matrix take gemm_apply_store_full (buffer stores, bit tricks), the others gemm_apply_store (per-element bounds, clamped aux
loads); M = 33 leaves a wave wholly past M, M = 130 cuts a Philox 4-row group.

Every case: C and the slabs carry a guard of 256 floats, slabs lie slab_stride = M * N + 64 apart, and outputs, gaps and guard
start as one NaN bit pattern (0x7FC0BEEF) that no arithmetic produces: gaps, guard and unreported slabs must keep it.  The
rng is {seed > 2^32, offset 3} with rng_offset_add 11.

Bounds: metric tests/test_hip_ops.py rel_err; bound = max(floor, 8 x the error of the same reference evaluated in fp32 on the
CPU against fp64), floor = 2e-6 * max(1, sqrt(K)), K the whole reduction length also for a split product (the rule of
tests/test_hip_heads.py).  ReLU outputs are compared where |pre-activation| > 1e-5 (tests/test_gemm_epi_cases_cpu.py: at most
1e-4 of the elements lie inside).  The module's report line prints the largest error / bound ratio per quantity.

Largest error / bound on an MI355X when the module was added (the case that gave it):
  epi 0        0.025 (mode 0, (97, 64, 4)); with aux 0.014 (mode 0, (64, 64, 128))
  split K      sum of the slabs 0.021 (mode 0, (64, 64, 508), one slab); one slab against its own K range 0.021 (mode 0,
               (130, 100, 1800), max_slabs 4).  Slab counts 2, 8, 6, 4, 1 and chunks 320, 256, 320, 512 for the five cases
  epi 1        0.027 ((97, 64, 4), train, p = 0.2); K = 100 on the generic kernel 0.020 (N = 1000, train, p = 0.2)
  epi 3        train 0.021, eval 0.022 (mode 0, (130, 64, 68))
  k100 hook    linear1 0.021, dgrad 0.024 in both forms (T = 1100)
The kernels sit at 1 - 3 % of the project's GEMM tolerance; no comparison of bits failed, the subnormal included: both forms of
every epilogue give the same values, as the comment in csrc/gemm.hip says.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_epi_cases as GC
from gemm_epi_cases import ADD, OFF, SEED, SITE
from test_hip_ops import lib, ptr, rel_err, stream  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF           # a NaN with a payload: what every output, gap and guard holds before a launch
GUARD = 256
WORST = {}                  # quantity -> (largest error / bound seen in this module, its case)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ngemm epilogue checks, largest error / bound per quantity: " +
          ", ".join("%s %.3g %s" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


def _bounded(fails, what, err, bound, tag):
    if err / bound > WORST.get(what, (0.0, ""))[0]:
        WORST[what] = (err / bound, tag)
    print("%s %s: error %.3e, bound %.3e" % (what, tag, err, bound))
    if not err <= bound:                                   # (a NaN fails too)
        fails.append((what, tag, err, bound))


def _expect(fails, cond, what, tag):
    if not cond:
        fails.append((what, tag))


def _bound(K, r32, r64, where=None):
    return max(GC.floor_bound(K), 8.0 * GC.rel_err(r32, r64, where))


def _sent(n):
    return torch.full((int(n),), SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rng():
    return torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")


def _weight(w, mode):
    """w [N x K] as the mode's operand: mode 0 W [N x K], mode 1 W [K x N]"""
    return (w if mode == 0 else w.T).contiguous().cuda()


def _hook(lib, mode, epi, A, W, bias, aux, Cbuf, stride, M, N, K, p, train, max_slabs, rng, site=SITE):
    n = C.c_int(-1)
    lib.call("ganffn_gemm_hook", mode, epi, ptr(A), ptr(W), ptr(bias), ptr(aux), ptr(Cbuf), stride, M, N, K, p, site, ptr(rng),
             ADD, train, max_slabs, C.byref(n), stream())
    torch.cuda.synchronize()
    return n.value


def _ids(cases):
    return ["m%d-%s" % (m, "x".join(map(str, s))) for m, s in cases]


# ------------------------------------------------------------------------------------------------------------------------
# a. epi 0, unsplit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape", GC.EPI0_CASES, ids=_ids(GC.EPI0_CASES))
def test_epi0_unsplit_bias_and_fused_residual(lib, mode, shape):
    """product + bias and product + bias + aux against fp64; the bits of ganffn_gemm_nt / ganffn_gemm_nn (the same launch)"""
    M, N, K = shape
    x, w, bias, aux = GC.inputs(M, N, K)
    xd, wd, bd, ad, rng = x.cuda(), _weight(w, mode), bias.cuda(), aux.cuda(), _rng()
    tag, fails = "mode %d %s" % (mode, shape), []
    for given in (None, aux):
        Cb = _sent(M * N + GUARD)
        n = _hook(lib, mode, 0, xd, wd, bd, None if given is None else ad, Cb, 0, M, N, K, 0.2, 1, 1, rng)
        _expect(fails, n == 1, "n_slabs == 1", tag)
        r64, r32 = GC.ref_epi0(x, w, bias, given), GC.ref_epi0(x, w, bias, given, dtype=torch.float32)
        _bounded(fails, "epi0" if given is None else "epi0+aux", rel_err(Cb[:M * N].view(M, N), r64), _bound(K, r32, r64), tag)
        _expect(fails, _untouched(Cb[M * N:]), "guard", tag)
        if given is None:
            plain = Cb[:M * N].clone()
    same = _sent(M * N + GUARD)
    if mode == 0:
        lib.call("ganffn_gemm_nt", ptr(xd), ptr(wd), ptr(bd), ptr(same), M, N, K, stream())
    else:                                                  # ganffn_gemm_nn takes no bias: the hook without one
        lib.call("ganffn_gemm_nn", ptr(xd), ptr(wd), ptr(same), M, N, K, stream())
        plain = _sent(M * N + GUARD)
        _hook(lib, mode, 0, xd, wd, None, None, plain, 0, M, N, K, 0.0, 0, 1, rng)
        plain = plain[:M * N]
    torch.cuda.synchronize()
    _expect(fails, _same_bits(same[:M * N], plain) and _untouched(same[M * N:]), "bits of ganffn_gemm_nt / _nn", tag)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------
# b. epi 0, split K
# ------------------------------------------------------------------------------------------------------------------------
SPLIT_IDS = ["%s-max%d" % ("x".join(map(str, s)), m) for s, m, _ in GC.SPLIT_CASES]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape,max_slabs,today", GC.SPLIT_CASES, ids=SPLIT_IDS)
def test_epi0_split_k_slabs(lib, mode, shape, max_slabs, today):
    """the slab layout: the in-order fp32 sum of the slabs is the product (+ bias + aux, once: both land in slab 0 only);
    slab z >= 1 is the product over its own K range, a range that starts at a multiple of 64; nothing is written past the
    slabs reported, into the gaps between them or into the guard; a second launch gives the same bits"""
    M, N, K = shape
    x, w, bias, aux = GC.inputs(M, N, K)
    xd, wd, bd, ad, rng = x.cuda(), _weight(w, mode), bias.cuda(), aux.cuda(), _rng()
    tag, fails = "mode %d %s max %d" % (mode, shape, max_slabs), []
    stride = M * N + 64

    def run(b, a):
        buf = _sent(max_slabs * stride + GUARD)
        return buf, _hook(lib, mode, 0, xd, wd, b, a, buf, stride, M, N, K, 0.2, 1, max_slabs, rng)
    buf, n = run(bd, ad)
    print("%s: n_slabs %d (today's rule: %d)" % (tag, n, today))
    assert 1 <= n <= max_slabs, n
    assert n >= 2 if today >= 2 else n == 1, n
    slab = lambda t, z: t[z * stride:z * stride + M * N].view(M, N)
    for z in range(n):
        _expect(fails, bool(torch.isfinite(slab(buf, z)).all()), "slab %d written everywhere" % z, tag)
        _expect(fails, _untouched(buf[z * stride + M * N:(z + 1) * stride]), "gap behind slab %d" % z, tag)
    _expect(fails, _untouched(buf[n * stride:]), "slabs >= n_slabs and the guard", tag)
    total = slab(buf, 0).clone()
    for z in range(1, n):
        total += slab(buf, z)
    r64, r32 = GC.ref_epi0(x, w, bias, aux), GC.ref_epi0(x, w, bias, aux, dtype=torch.float32)
    _bounded(fails, "split sum", rel_err(total, r64), _bound(K, r32, r64), tag)
    # a second launch: the same bits, everywhere
    buf2, n2 = run(bd, ad)
    _expect(fails, n2 == n and _same_bits(buf, buf2), "second launch", tag)
    # bias and aux once: without them slabs z >= 1 keep their bits, and slab 0 is (its product + bias) + aux in fp32
    bare, n3 = run(None, None)
    _expect(fails, n3 == n and _untouched(bare[n * stride:]), "n_slabs / guard without bias and aux", tag)
    for z in range(1, n):
        _expect(fails, _same_bits(slab(bare, z), slab(buf, z)), "slab %d carries no bias / aux" % z, tag)
    _expect(fails, _same_bits((slab(bare, 0) + bd) + ad, slab(buf, 0)), "slab 0 = (product + bias) + aux", tag)
    # the K ranges: a chunk size kc, a multiple of 64 with ceil(K / kc) = n_slabs, such that slab z is the product over
    # [z kc, min(K, (z + 1) kc)) — the last chunk ragged
    if n >= 2:
        best = None
        for kc in range(64, K + 64, 64):
            if (K + kc - 1) // kc != n:
                continue
            worst = 0.0
            for z in range(n):
                k0, k1 = z * kc, min(K, (z + 1) * kc)
                p64 = x[:, k0:k1].double() @ w[:, k0:k1].double().T
                worst = max(worst, rel_err(slab(bare, z), p64) / GC.floor_bound(k1 - k0))
            if best is None or worst < best[0]:
                best = (worst, kc)
        assert best is not None, "no chunk size that is a multiple of 64 gives %d slabs" % n
        print("%s: chunk %d, last chunk %d" % (tag, best[1], K - (n - 1) * best[1]))
        _bounded(fails, "split slab", best[0], 1.0, tag + " kc %d" % best[1])
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------
# c. epi 1 (EPI_RELU_DROP)
# ------------------------------------------------------------------------------------------------------------------------
def _check_epi1(fails, what, tag, got, x, w, bias, p, train, K, site=SITE):
    """values against fp64 outside the kink band; in train mode with p > 0 the zero pattern is ~keep | (pre <= 0) there"""
    r64, pre = GC.ref_epi1(x, w, bias, p, train, site=site)
    r32, _ = GC.ref_epi1(x, w, bias, p, train, dtype=torch.float32, site=site)
    ok = pre.abs() > GC.KINK
    got = got.cpu()
    _expect(fails, bool(torch.isfinite(got).all()), what + " finite", tag)
    _bounded(fails, what, GC.rel_err(got, r64, ok), _bound(K, r32, r64, ok), tag)
    if train and p > 0:
        zero = ~GC.keep_mask(*pre.shape, p, train, site) | (pre <= 0)
        _expect(fails, bool((((got == 0) == zero) | ~ok).all()), what + " zero pattern", tag)
        _expect(fails, bool((_bits(got)[zero & ok] == 0).all()), what + " drops to +0", tag)


@pytest.mark.parametrize("train,p", GC.MODES, ids=GC.MODE_IDS)
@pytest.mark.parametrize("shape", GC.EPI1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_epi1_relu_dropout(lib, shape, train, p):
    M, N, K = shape
    x, w, bias, _ = GC.inputs(M, N, K)
    xd, wd, bd, rng = x.cuda(), w.cuda(), bias.cuda(), _rng()
    tag, fails = "%s train=%d p=%g" % (shape, train, p), []
    Cb = _sent(M * N + GUARD)
    _hook(lib, 0, 1, xd, wd, bd, None, Cb, 0, M, N, K, p, train, 1, rng)
    got = Cb[:M * N].view(M, N)
    _check_epi1(fails, "epi1", tag, got, x, w, bias, p, train, K)
    _expect(fails, _untouched(Cb[M * N:]), "guard", tag)
    Cb2 = _sent(M * N + GUARD)
    _hook(lib, 0, 1, xd, wd, bd, None, Cb2, 0, M, N, K, p, train, 1, rng)
    _expect(fails, _same_bits(Cb, Cb2), "second launch", tag)
    if (N, K) == (2048, 100):                               # the weight-resident kernel in both calls
        h = _sent(M * N + GUARD)
        lib.call("ganffn_ffn_linear1_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(h), M, K, N, p, SITE, ptr(rng), ADD, train, stream())
        torch.cuda.synchronize()
        _expect(fails, _same_bits(h, Cb), "bits of ganffn_ffn_linear1_fwd", tag)
    assert not fails, fails


@pytest.mark.parametrize("shape", [(97, 132, 132), (64, 64, 128), GC.WRES_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_epi1_relu_dropout_on_a_k_major_weight(lib, shape):
    """mode 1 (C = A W, W [K x N]) under linear1's epilogue, which no network runs: the generic, the short-K and the
    weight-resident kernel, train mode with p = 0.2, held to test_epi1_relu_dropout's bounds"""
    M, N, K = shape
    x, w, bias, _ = GC.inputs(M, N, K)
    xd, wd, bd, rng = x.cuda(), _weight(w, 1), bias.cuda(), _rng()
    tag, fails = "mode 1 %s" % (shape,), []
    Cb = _sent(M * N + GUARD)
    _hook(lib, 1, 1, xd, wd, bd, None, Cb, 0, M, N, K, 0.2, 1, 1, rng)
    _expect(fails, _untouched(Cb[M * N:]), "guard", tag)
    _check_epi1(fails, "epi1 mode 1", tag, Cb[:M * N].view(M, N), x, w, bias, 0.2, 1, K)
    assert not fails, fails


@pytest.mark.parametrize("train,p", GC.MODES, ids=GC.MODE_IDS)
def test_epi1_generic_short_k_kernel_gives_the_weight_resident_kernels_bits(lib, train, p):
    """K = 100: N = 2048 runs on the weight-resident kernel, the first 132 / 1000 columns alone on the generic K <= 128
    instantiation.  The same rows and columns must carry the same bits (test_weight_resident_short_k_kernel_gives_the_
    generic_kernels_bits states it for EPI_NONE); the dropout mask depends on N, so in train mode with p > 0 the comparison
    runs over the elements both masks keep, and each side's zero pattern is checked against its own mask"""
    M, N, K = 161, 2048, 100
    x, w, bias, _ = GC.inputs(M, N, K)
    xd, wd, bd, rng = x.cuda(), w.cuda(), bias.cuda(), _rng()
    fails = []
    big = _sent(M * N + GUARD)
    _hook(lib, 0, 1, xd, wd, bd, None, big, 0, M, N, K, p, train, 1, rng)
    big = big[:M * N].view(M, N)
    for Ns in (132, 1000):
        tag = "N %d train=%d p=%g" % (Ns, train, p)
        ws, bs = w[:Ns].contiguous(), bias[:Ns].contiguous()
        small = _sent(M * Ns + GUARD)
        _hook(lib, 0, 1, xd, ws.cuda(), bs.cuda(), None, small, 0, M, Ns, K, p, train, 1, rng)
        _expect(fails, _untouched(small[M * Ns:]), "guard", tag)
        small = small[:M * Ns].view(M, Ns)
        _check_epi1(fails, "epi1 short-K", tag, small, x, ws, bs, p, train, K)
        both = (GC.keep_mask(M, N, p, train)[:, :Ns] & GC.keep_mask(M, Ns, p, train)).cuda()
        assert float(both.float().mean()) > 0.6
        _expect(fails, torch.equal(_bits(small)[both], _bits(big[:, :Ns])[both]), "bits of the weight-resident kernel", tag)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------
# d. epi 3 (EPI_MASK_POS)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape", GC.EPI3_CASES, ids=_ids(GC.EPI3_CASES))
def test_epi3_mask_by_saved_activation(lib, mode, shape):
    """(A W) * (aux > 0) * scale with IEEE's predicate on an aux that holds +0, -0, negative values, FLT_MIN and a
    subnormal: against fp64 in train mode (scale 1 / 0.8) and in eval mode (scale 1); exactly +0 wherever aux is not
    positive; the train-mode output is the eval-mode output times 1.25 in fp32, bit for bit"""
    M, N, K = shape
    x, w, _, _ = GC.inputs(M, N, K)
    act = GC.saved_activation(M, N)
    xd, wd, ad, rng = x.cuda(), _weight(w, mode), act.cuda(), _rng()
    tag, fails = "mode %d %s" % (mode, shape), []
    outs = {}
    for train, p in ((1, 0.2), (0, 0.2)):
        Cb = _sent(M * N + GUARD)
        _hook(lib, mode, 3, xd, wd, None, ad, Cb, 0, M, N, K, p, train, 1, rng)
        got = Cb[:M * N].view(M, N).cpu()
        r64, r32 = GC.ref_epi3(x, w, act, p, train), GC.ref_epi3(x, w, act, p, train, dtype=torch.float32)
        _bounded(fails, "epi3 train" if train else "epi3 eval", rel_err(got, r64), _bound(K, r32, r64), tag)
        _expect(fails, bool((_bits(got)[~(act > 0)] == 0).all()), "+0 wherever aux <= 0", tag)
        _expect(fails, _untouched(Cb[M * N:]), "guard", tag)
        outs[train] = got
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(0.2))
    _expect(fails, _same_bits(outs[1], outs[0] * float(scale)), "train = eval * 1 / (1 - p) in fp32", tag)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------
# e. the pattern words, through ganffn_ffn_k100_hook
# ------------------------------------------------------------------------------------------------------------------------
HSENT = 0x5A5A


def _k100(lib, which, a, w, bias, out, hmask, h_saved, T, p, train, rng):
    lib.call("ganffn_ffn_k100_hook", which, ptr(a), ptr(w), ptr(bias), ptr(out), ptr(hmask), ptr(h_saved), T, p, SITE, ptr(rng), ADD,
             train, stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("T", GC.K100_T)
def test_k100_pattern_words_and_the_two_forms_of_the_dgrad_mask(lib, T):
    """which 0 with hmask: out against fp64, and the pattern bits of rows < T are pattern_words(out) (bits of rows >= T in
    the last row tile are unspecified).  which 1 from that hmask and from h_saved = out: the SAME bits, both (a w) * (out >
    0) / (1 - p) against fp64; again under bit 25 of the debug mode word.  T = 1100: 18 token tiles on a persistent grid of
    16 workgroups per panel, the last tile with 12 rows; T = 1, 33: the second wave of the tile lies wholly past T (the row
    tile of its pattern words is clamped)"""
    E, F, p, train = 100, 2048, 0.2, 1
    x, w1, b1, _ = GC.inputs(T, F, E)
    xd, wd, bd, rng = x.cuda(), w1.cuda(), b1.cuda(), _rng()
    tag, fails = "T %d" % T, []
    nwords = (T + 31) // 32 * F * 2
    out = _sent(T * F + GUARD)
    hmask = torch.full((nwords + 2 * GUARD,), HSENT, dtype=torch.int16, device="cuda")
    _k100(lib, 0, xd, wd, bd, out, hmask, None, T, p, train, rng)
    _expect(fails, _untouched(out[T * F:]) and bool((hmask[nwords:] == HSENT).all()), "guards of out and hmask", tag)
    h = out[:T * F].view(T, F)
    _check_epi1(fails, "k100 linear1", tag, h, x, w1, b1, p, train, E)
    words = hmask[:nwords].cpu().numpy().view(np.uint16)
    hc = h.cpu()
    _expect(fails, torch.equal(GC.pattern_rows(words, T, F), hc > 0), "pattern bits of rows < T", tag)
    full = (T // 32) * F * 2                                 # the words of row tiles wholly inside T: every bit specified
    _expect(fails, np.array_equal(words[:full], GC.pattern_words(hc)[:full]), "pattern words of the full row tiles", tag)
    plain = _sent(T * F + GUARD)                             # the activation does not depend on whether the pattern is kept
    _k100(lib, 0, xd, wd, bd, plain, None, None, T, p, train, rng)
    _expect(fails, _same_bits(plain, out), "out with and without hmask", tag)

    a, w2 = GC.k100_dgrad_inputs(T)
    ad, w2d = a.cuda(), w2.T.contiguous().cuda()             # [100 x 2048]
    r64 = (a.double() @ w2.double().T) * (hc > 0).double() / (1 - p)
    r32 = (a @ w2.T) * (hc > 0).float() / (1 - p)
    bound = _bound(E, r32, r64)
    from gan_ffn_amd import _lib
    first = None
    try:
        for bits in (0, 1 << 25):
            _lib.load().ganffn_debug_set_ffn_mode(bits)
            d_bits, d_saved = _sent(T * F + GUARD), _sent(T * F + GUARD)
            _k100(lib, 1, ad, w2d, None, d_bits, hmask, None, T, p, train, rng)
            _k100(lib, 1, ad, w2d, None, d_saved, None, h, T, p, train, rng)
            t2 = tag + " mode word %#x" % bits
            _expect(fails, _same_bits(d_bits, d_saved), "dgrad: pattern form == saved-activation form", t2)
            _bounded(fails, "k100 dgrad (pattern)", rel_err(d_bits[:T * F].view(T, F), r64), bound, t2)
            _bounded(fails, "k100 dgrad (saved)", rel_err(d_saved[:T * F].view(T, F), r64), bound, t2)
            _expect(fails, _untouched(d_bits[T * F:]) and _untouched(d_saved[T * F:]), "guard", t2)
            if first is None:
                first = d_bits
            else:
                _expect(fails, _same_bits(first, d_bits), "bit 25 changes no bit", t2)
    finally:
        _lib.load().ganffn_debug_set_ffn_mode(0)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------
# f. path independence
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("N,K", [(132, 132), (64, 68), (36, 516)])
def test_a_rows_bits_do_not_depend_on_the_epilogue_form_that_stores_it(lib, epi, N, K):
    """eval, p = 0.  Rows 64..96 of an M = 97 problem — row 96 lies in a wave tile cut by M, which the per-element epilogue
    stores — placed at rows 0..32 of an M = 64 problem, where the straight-line full-tile epilogue stores every one of
    them: the same bits.  And along N: the columns past the last full 32 of a ragged N, moved to the front of an N = 64
    problem"""
    x, w, bias, _ = GC.inputs(97, N, K)
    rng = _rng()

    def run(xx, ww, bb):
        M, Nn = xx.shape[0], ww.shape[0]
        Cb = _sent(M * Nn + GUARD)
        _hook(lib, 0, epi, xx.cuda(), ww.contiguous().cuda(), bb.contiguous().cuda(), None, Cb, 0, M, Nn, K, 0.0, 0, 1, rng)
        assert _untouched(Cb[M * Nn:])
        return Cb[:M * Nn].view(M, Nn)
    edge = run(x, w, bias)
    assert bool(torch.isfinite(edge).all())
    x64 = torch.cat([x[64:97], x[:31]])
    full = run(x64, w, bias)
    assert _same_bits(edge[64:97], full[:33])
    tail = N - N % 32
    if N % 32:                                              # columns tail..N-1: an edge tile here, a full tile there
        g = torch.Generator().manual_seed(N + K)
        w64 = torch.cat([w[tail:], torch.randn(64 - (N - tail), K, generator=g) / 10])
        b64 = torch.cat([bias[tail:], torch.zeros(64 - (N - tail))])
        moved = run(x[:64], w64, b64)
        assert _same_bits(edge[:64, tail:], moved[:, :N - tail])
