"""The data-movement kernels of csrc/drnn_head.hip and csrc/elementwise.hip alone: ganffn_seq_reverse (plain and
accumulating), ganffn_drnn_join_fwd / _bwd, ganffn_mask_pos_inplace, ganffn_add3, ganffn_rng_advance and ganffn_zero_floats.

These kernels move, mask or add, so the references are exact and every comparison is BIT EQUALITY with the fp32 evaluation
of the reference on the CPU — with one statement about the dropout scale: the kernels multiply by a precomputed fp32
1 / (1 - p) (csrc/common.h make_drop), they do not divide.  The join is therefore held to two things: the bits of
x * fl(1 / (1 - p)), and at most 1 ulp from the reference's x / (1 - p) (at p = 0.2 the factor is exactly 1.25, at p = 0 and
in eval mode it is 1 and both forms coincide).  The adjointness of the join pair is checked in fp64 to 1e-6 relative.

Shapes: S * B % 4 != 0 (a Philox 4-row group cut by the end of the batch), De % 4 != 0, lengths 0, 1, S and interior ones in
every batch position; outputs start as a NaN bit pattern, so a row nobody writes shows.  Lengths outside 0 <= len <= S are
the caller's contract (include/ganffn.h) and are not passed.

Largest deviation on an MI355X when the module was added: every bit comparison held; the join is 1 ulp from x / (1 - p) at
p = 0.2 (0 otherwise), and its adjointness residual is at most 2.4e-8 relative (the 1e-6 allows for nothing but the fp64 sums).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_epi_cases as GC
from engine_oracle import SITE_JOIN_B, SITE_JOIN_F
from oracle import philox
from test_hip_ops import lib, ptr, stream  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

SEED, OFF, ADD = GC.SEED, GC.OFF, GC.ADD
SENT = 0x7FC0BEEF
GUARD = 256
WORST = {"join ulp from x / (1 - p)": 0, "join adjointness (relative)": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nsequence kernel checks, largest deviation: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _sent(n):
    return torch.full((int(n),), SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _lens_variants(S, B):
    """length vectors that put 0, 1, S, S - 1 and S // 2 into the batch, every value at least once over the variants"""
    cand = sorted({0, 1, S, max(S - 1, 0), S // 2})
    return [[cand[(b + r) % len(cand)] for b in range(B)] for r in range(0, len(cand), B)]


def _reverse(x, lens):
    """out[s, b] = s < len_b ? x[len_b - 1 - s, b] : 0"""
    out = torch.zeros_like(x)
    for b, n in enumerate(lens):
        if n > 0:
            out[:n, b] = x[:n, b].flip(0)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# ganffn_seq_reverse
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,D", [(1, 1, 4), (7, 3, 8), (33, 5, 100), (94, 2, 512)])
def test_seq_reverse(lib, S, B, D):
    g = torch.Generator().manual_seed(S * 131 + B * 17 + D)
    x, out0 = torch.randn(S, B, D, generator=g), torch.randn(S, B, D, generator=g)
    xd = x.cuda()
    n = S * B * D
    for lens in _lens_variants(S, B):
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        ref = _reverse(x, lens)
        # plain, into NaN: the reversed prefix, exact zeros behind it
        buf = _sent(n + GUARD)
        lib.call("ganffn_seq_reverse", ptr(xd), ptr(ld), ptr(buf), S, B, D, 0, stream())
        torch.cuda.synchronize()
        got = buf[:n].view(S, B, D)
        assert _same_bits(got, ref) and _untouched(buf[n:]), lens
        for b, m in enumerate(lens):
            assert bool((_bits(got[m:, b]) == 0).all()), (lens, b)
        # accumulating: out0 + reversed in fp32
        acc = torch.cat([out0.reshape(-1).cuda(), _sent(GUARD)])
        lib.call("ganffn_seq_reverse", ptr(xd), ptr(ld), ptr(acc), S, B, D, 1, stream())
        torch.cuda.synchronize()
        assert _same_bits(acc[:n].view(S, B, D), out0 + ref) and _untouched(acc[n:]), lens
        # twice: the valid prefix, zeros in the padding
        twice = _sent(n + GUARD)
        lib.call("ganffn_seq_reverse", ptr(got), ptr(ld), ptr(twice), S, B, D, 0, stream())
        torch.cuda.synchronize()
        keep = (torch.arange(S).view(S, 1) < torch.tensor(lens).view(1, B)).view(S, B, 1)
        assert _same_bits(twice[:n].view(S, B, D), torch.where(keep, x, torch.zeros(()))) and _untouched(twice[n:]), lens


# ------------------------------------------------------------------------------------------------------------------------
# ganffn_drnn_join_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """largest distance in units in the last place between two finite fp32 tensors of equal signs (0 for +-0 against +-0)"""
    ia, ib = _bits(a.cpu()).long(), _bits(b.cpu()).long()
    d = (ia - ib).abs()
    d[(a.cpu() == 0) & (b.cpu() == 0)] = 0
    return int(d.max()) if d.numel() else 0


@pytest.mark.parametrize("train,p", GC.MODES, ids=GC.MODE_IDS)
@pytest.mark.parametrize("S,B,De", [(1, 1, 4), (5, 3, 6), (7, 3, 100), (33, 5, 100)])
def test_drnn_join_fwd_bwd(lib, S, B, De, train, p):
    """emotions = cat(e_f * kf, reverse(e_b) * kb) / (1 - p), both masks indexed by the forward-time row s * B + b; the
    backward gives d_e_f and d_e_b (in the reverse direction's own order, rows >= len exact zeros)"""
    g = torch.Generator().manual_seed(S * 1009 + B * 31 + De)
    e_f, e_b, d_em = torch.randn(S, B, De, generator=g), torch.randn(S, B, De, generator=g), torch.randn(S, B, 2 * De, generator=g)
    T = S * B
    on = bool(train and p > 0)
    kf = torch.from_numpy(philox.keep_mask(T, De, p if on else 0.0, SITE_JOIN_F, SEED, OFF + ADD)).view(S, B, De)
    kb = torch.from_numpy(philox.keep_mask(T, De, p if on else 0.0, SITE_JOIN_B, SEED, OFF + ADD)).view(S, B, De)
    if on:
        assert not torch.equal(kf, kb) or T * De < 8
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if on else 1.0      # what the kernels multiply by
    div = (1 - p) if on else 1.0                                                             # what the reference divides by
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    efd, ebd, demd = e_f.cuda(), e_b.cuda(), d_em.cuda()
    for lens in _lens_variants(S, B):
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        valid = (torch.arange(S).view(S, 1) < torch.tensor(lens).view(1, B)).view(S, B, 1)
        rev = _reverse(e_b, lens)
        em = _sent(T * 2 * De + GUARD)
        lib.call("ganffn_drnn_join_fwd", ptr(efd), ptr(ebd), ptr(ld), ptr(em), S, B, De, p, SITE_JOIN_F, SITE_JOIN_B, ptr(rng),
                 ADD, train, stream())
        torch.cuda.synchronize()
        assert _untouched(em[T * 2 * De:]), lens
        got = em[:T * 2 * De].view(S, B, 2 * De).cpu()
        assert bool(torch.isfinite(got).all()), lens
        assert torch.equal(got, torch.cat([e_f * kf * scale, rev * kb * scale], dim=2)), lens
        ref_div = torch.cat([e_f * kf / div, rev * kb / div], dim=2)
        u = _ulps(got, ref_div)
        WORST["join ulp from x / (1 - p)"] = max(WORST["join ulp from x / (1 - p)"], u)
        assert u <= 1, (lens, u)
        if on:     # the zero pattern is the contract's, at forward-time rows: dropped wherever a mask drops
            assert bool((got[..., :De][~kf] == 0).all()) and bool((got[..., De:][~kb] == 0).all()), lens
        assert bool((_bits(got[..., De:])[(~valid).expand(S, B, De)] == 0).all()), lens      # the padded half: +0

        d_f, d_b = _sent(T * De + GUARD), _sent(T * De + GUARD)
        lib.call("ganffn_drnn_join_bwd", ptr(demd), ptr(ld), ptr(d_f), ptr(d_b), S, B, De, p, SITE_JOIN_F, SITE_JOIN_B, ptr(rng),
                 ADD, train, stream())
        torch.cuda.synchronize()
        assert _untouched(d_f[T * De:]) and _untouched(d_b[T * De:]), lens
        gf, gb = d_f[:T * De].view(S, B, De).cpu(), d_b[:T * De].view(S, B, De).cpu()
        assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(gb).all()), lens       # every row written
        assert torch.equal(gf, d_em[..., :De] * kf * scale), lens
        # d_e_b[len - 1 - s, b] = (d_em[s, b, De:] * kb[s, b]) * scale: the reversal of the masked, scaled gradient
        assert torch.equal(gb, _reverse(d_em[..., De:] * kb * scale, lens)), lens
        assert _ulps(gf, d_em[..., :De] * kf / div) <= 1 and _ulps(gb, _reverse(d_em[..., De:] * kb / div, lens)) <= 1, lens
        assert bool((_bits(gb)[(~valid).expand(S, B, De)] == 0).all()), lens                  # rows >= len: +0
        # adjointness in fp64: <join_fwd(e_f, e_b), d> == <e_f, d_e_f> + <e_b, d_e_b>
        lhs = float((got.double() * d_em.double()).sum())
        rhs = float((e_f.double() * gf.double()).sum() + (e_b.double() * gb.double()).sum())
        size = float((got.double() * d_em.double()).abs().sum()) or 1.0
        WORST["join adjointness (relative)"] = max(WORST["join adjointness (relative)"], abs(lhs - rhs) / size)
        assert abs(lhs - rhs) <= 1e-6 * size, (lens, lhs, rhs)


# ------------------------------------------------------------------------------------------------------------------------
# ganffn_mask_pos_inplace, ganffn_add3
# ------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 255, 256, 257, 100003]


@pytest.mark.parametrize("mscale", [1.0, 1.25])
@pytest.mark.parametrize("n", SIZES)
def test_mask_pos_inplace(lib, n, mscale):
    """d[i] = aux[i] > 0 ? d[i] * mscale : 0 with IEEE's predicate: +0, -0 and negative values mask, FLT_MIN and a
    subnormal pass; a masked element is +0"""
    g = torch.Generator().manual_seed(n)
    d = torch.randn(n, generator=g)
    aux = GC.saved_activation(1, n).view(-1) if n > 1 else torch.tensor([GC.SUBNORMAL])
    buf = torch.cat([d.cuda(), _sent(GUARD)])
    auxd = aux.cuda()
    lib.call("ganffn_mask_pos_inplace", ptr(buf), ptr(auxd), mscale, n, stream())
    torch.cuda.synchronize()
    ref = torch.where(aux > 0, d * mscale, torch.zeros(()))
    assert _same_bits(buf[:n], ref) and _untouched(buf[n:])
    assert torch.equal(auxd.cpu().view(torch.int32), aux.view(torch.int32))
    if n > 16:
        passed = (aux > 0) & (aux <= GC.FLT_MIN)
        assert int(passed.sum()) > 1 and bool((buf[:n].cpu()[passed] == d[passed] * mscale).all())


@pytest.mark.parametrize("n", SIZES)
def test_add3(lib, n):
    g = torch.Generator().manual_seed(n + 7)
    a, b, c = (torch.randn(n, generator=g) * s for s in (1.0, 1e-3, 1e3))
    ad, bd, cd = a.cuda(), b.cuda(), c.cuda()
    out = _sent(n + GUARD)
    lib.call("ganffn_add3", ptr(ad), ptr(bd), ptr(cd), ptr(out), n, stream())
    torch.cuda.synchronize()
    assert _same_bits(out[:n], (a + b) + c) and _untouched(out[n:])
    assert torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b) and torch.equal(cd.cpu(), c)


# ------------------------------------------------------------------------------------------------------------------------
# ganffn_rng_advance
# ------------------------------------------------------------------------------------------------------------------------
def _i64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def _state(rng):
    torch.cuda.synchronize()
    return [int(v) for v in rng.cpu().numpy().view(np.uint64)]


def test_rng_advance(lib):
    seed = 0x9234567890ABCDEF
    rng = torch.tensor([_i64(seed), (1 << 32) - 1], dtype=torch.int64, device="cuda")
    lib.call("ganffn_rng_advance", ptr(rng), 1, stream())
    assert _state(rng) == [seed, 1 << 32]                                  # the carry into the high word
    rng = torch.tensor([_i64(seed), -1], dtype=torch.int64, device="cuda")
    lib.call("ganffn_rng_advance", ptr(rng), 2, stream())
    assert _state(rng) == [seed, 1]                                        # 2^64 - 1 + 2 wraps to 1
    rng = torch.tensor([_i64(seed), 5], dtype=torch.int64, device="cuda")
    lib.call("ganffn_rng_advance", ptr(rng), (1 << 40) + 3, stream())
    lib.call("ganffn_rng_advance", ptr(rng), 9, stream())
    assert _state(rng) == [seed, 5 + (1 << 40) + 3 + 9]                    # two advances compose


@pytest.mark.parametrize("off,delta", [(5, 7), ((1 << 32) - 1, 1), ((1 << 32) - 8, 40)])
def test_dropout_after_an_advance_draws_the_mask_of_the_advanced_offset(lib, off, delta):
    R, Cn, p, site, seed = 13, 100, 0.2, 18, SEED
    rng = torch.tensor([seed, off], dtype=torch.int64, device="cuda")
    lib.call("ganffn_rng_advance", ptr(rng), delta, stream())
    x, y = torch.ones(R, Cn, device="cuda"), _sent(R * Cn + GUARD)
    lib.call("ganffn_dropout", ptr(x), ptr(y), R, Cn, p, site, ptr(rng), ADD, stream())
    assert _state(rng) == [seed, off + delta]
    got = y[:R * Cn].view(R, Cn).cpu().numpy()
    assert ((got != 0) == philox.keep_mask(R, Cn, p, site, seed, off + delta + ADD)).all() and _untouched(y[R * Cn:])
    assert not ((got != 0) == philox.keep_mask(R, Cn, p, site, seed, off + ADD)).all()      # (the masks do differ)


# ------------------------------------------------------------------------------------------------------------------------
# ganffn_zero_floats
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [4, 5], ids=["aligned16", "offset4"])
@pytest.mark.parametrize("n", [1, 3, 4, 257])
def test_zero_floats(lib, n, lead):
    buf = _sent(lead + n + GUARD)
    assert buf.data_ptr() % 16 == 0
    target = buf[lead:]
    assert target.data_ptr() % 16 == (0 if lead == 4 else 4)
    lib.call("ganffn_zero_floats", ptr(target), n, stream())
    torch.cuda.synchronize()
    assert bool((_bits(buf[lead:lead + n]) == 0).all())
    assert _untouched(buf[:lead]) and _untouched(buf[lead + n:])
