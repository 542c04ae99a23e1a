"""ganffn_attention_fwd_mask / _bwd_mask with GANFFN_ATTN_CAUSAL: self-attention in which query i attends to keys j <= i (and,
with lengths, j < key_len[b]), on every kernel the dispatch reaches, against the fp64 causal oracle with the same Philox mask
(tests/causal_oracle.py).  Bounds: the project's own for these kernels (tests/test_hip_ops.py::test_attention_fwd_bwd,
tests/test_hip_attention_key_len.py) — a mask only removes terms from the same sums.  The shapes cross every tile edge of both
kernel families: 16 / 17, 32 / 33, 48 / 49, 64 / 65."""
import ctypes as C

import pytest
import torch

from oracle import ganffn_oracle as O
from causal_oracle import causal_attention, causal_lse

pytestmark = pytest.mark.gpu

SEED, OFF, ADD, LAYER = 777, 11, 4, 2
SITE = O.SITE_LAYER0 + 4 * LAYER
CAUSAL = 1        # GANFFN_ATTN_CAUSAL

CASES = {
    # 16-row kernels, head_dim 10
    "hd10_1": (1, 2, 20, 2, None),
    "hd10_16": (16, 2, 20, 2, None),
    "hd10_17": (17, 4, 20, 2, [17, 16, 1, 5]),
    "hd10_33": (33, 3, 20, 2, [33, 32, 17]),
    "hd10_94_10heads": (94, 2, 100, 10, [94, 48]),
    "hd10_110": (110, 2, 20, 2, None),
    "hd10_400_problems": (17, 200, 20, 2, [1 + b % 17 for b in range(200)]),      # the path without keep words
    # four query tiles: workgroups cut in two (with lengths: hd10_94_10heads), and whole at B H >= 512
    "hd10_50": (50, 2, 20, 2, None),
    "hd10_520_problems": (50, 52, 100, 10, None),
    "hd10_520_problems_ragged": (50, 52, 100, 10, [50, 1] + [1 + (7 * b) % 50 for b in range(50)]),
    # 16-row, head_dim 30
    "hd30_17": (17, 3, 60, 2, None),
    "hd30_33": (33, 2, 60, 2, [33, 20]),
    "hd30_50": (50, 2, 60, 2, None),
    "hd30_50_ragged": (50, 2, 60, 2, [50, 33]),
    "hd30_512_problems": (50, 128, 120, 4, None),
    "hd30_512_problems_ragged": (50, 128, 120, 4, [50, 1] + [1 + (7 * b) % 50 for b in range(126)]),
    # 16-row, head_dim 64 / 60 (S <= 48)
    "hd64_40": (40, 2, 128, 2, [40, 17]),
    "hd60_48": (48, 2, 120, 2, None),
    # 32-row, head_dim 64 / 60
    "hd64_49": (49, 3, 128, 2, [49, 33, 32]),
    "hd60_65": (65, 2, 120, 2, None),
    "hd64_94": (94, 2, 512, 8, [94, 1]),
    # run-time head_dim
    "hd4_33": (33, 2, 8, 2, None),
    "hd32_65": (65, 2, 128, 4, [65, 64]),
    "hd6_7": (7, 3, 18, 3, [7, 1, 4]),
}
# one or two shapes per kernel family for the tests that run several launches per case
WITH_FUTURE = [c for c in CASES if CASES[c][0] > 1]      # a single utterance has no future to hide
FAMILIES = ["hd10_17", "hd10_94_10heads", "hd30_33", "hd64_40", "hd60_48", "hd64_49", "hd60_65", "hd4_33", "hd32_65"]


@pytest.fixture(scope="module")
def lib():
    from gan_ffn_amd import _lib
    return _lib


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def writes_lse(E, H, S):
    hd = E // H
    return hd in (10, 30) or (hd in (60, 64) and S <= 48)        # the 16-row kernels (csrc/attention16.hip: attn16_supported)


def inputs(S, B, E, H):
    g = torch.Generator().manual_seed(S * 131 + B * 17 + E)
    return torch.randn(S, B, 3 * E, generator=g) * 1.5, torch.randn(S, B, E, generator=g)


def run(lib, qkv, do, lengths, H, p, keep_words, flags=CAUSAL, entry="mask", check=True):
    """the _mask pair (or, entry="len", the _len pair) on the device -> (o, lse, d_qkv), every output starting as NaN.
    lengths=None: a NULL key_len pointer.  check=False: return the two return codes as well instead of raising."""
    S, B, E = do.shape
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    qd, dod = qkv.cuda().contiguous(), do.cuda().contiguous()
    kl = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    keep = torch.zeros(int(lib.load().ganffn_attention_keep_words(B, H)), dtype=torch.int32, device="cuda") if keep_words else None
    od = torch.full((S, B, E), float("nan"), device="cuda")
    lse = torch.full((B * H, S), float("nan"), device="cuda")
    dq = torch.full((S, B, 3 * E), float("nan"), device="cuda")
    fl = () if entry == "len" else (C.c_uint32(flags),)
    tail = (S, B, E, H, C.c_float(p), C.c_uint32(SITE), ptr(rng), C.c_uint64(ADD), stream())
    fwd = (ptr(qd), ptr(od), ptr(lse), ptr(keep), ptr(kl)) + fl + tail
    if check:
        lib.call("ganffn_attention_fwd_" + entry, *fwd)
        o_in = od
    else:
        rc_f = getattr(lib.load(), "ganffn_attention_fwd_" + entry)(*fwd)
        msg_f = lib.load().ganffn_last_error()
        o_in = torch.zeros_like(od)           # a refused forward left no output for the backward to read
        lse_in = torch.zeros_like(lse)
    bwd = (ptr(qd), ptr(o_in), ptr(lse if check else lse_in), ptr(dod), ptr(keep), ptr(kl)) + fl + (ptr(dq),) + tail
    if check:
        lib.call("ganffn_attention_bwd_" + entry, *bwd)
    else:
        rc_b = getattr(lib.load(), "ganffn_attention_bwd_" + entry)(*bwd)
        msg_b = lib.load().ganffn_last_error()
    torch.cuda.synchronize()
    if check:
        return od, lse, dq
    return od, lse, dq, (rc_f, msg_f, rc_b, msg_b)


def oracle(qkv, do, lengths, B, H, p):
    q = qkv.detach().clone().double().requires_grad_(True)
    saved = O.ENC_DROPOUT
    O.ENC_DROPOUT = p
    try:
        with causal_attention(lengths):
            o_ref = O.attention(q, B, H, LAYER, O.Rng(SEED, OFF + ADD, train=p > 0))
    finally:
        O.ENC_DROPOUT = saved
    (o_ref * do.double()).sum().backward()
    return o_ref.detach(), q.grad


def edges(S):
    """query rows t to cut the future at: the first rows, both sides of every 16- and 32-row tile edge inside S, the last rows"""
    ts = {0, 1, S // 2, S - 2, S - 1}
    for e in (16, 32, 48, 64, 80, 96):
        ts |= {e - 1, e}
    return sorted(t for t in ts if 0 <= t < S - 1) or [0]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_causal_fwd_bwd(lib, case, p):
    """tests 1 and 2: against the fp64 causal oracle; keep words or Philox recompute give the same bits"""
    S, B, E, H, lengths = CASES[case]
    qkv, do = inputs(S, B, E, H)
    o_ref, dq_ref = oracle(qkv, do, lengths, B, H, p)
    od, lse, dq = run(lib, qkv, do, lengths, H, p, keep_words=False)
    od2, lse2, dq2 = run(lib, qkv, do, lengths, H, p, keep_words=True)
    assert torch.equal(od, od2) and torch.equal(dq, dq2)          # keep words or Philox calls: the same bits
    err = {"o": rel_err(od, o_ref), "dq": rel_err(dq, dq_ref)}
    if writes_lse(E, H, S):
        assert torch.equal(lse, lse2)
        err["lse"] = rel_err(lse, causal_lse(qkv, B, H, lengths))
    print(case, p, err)
    assert not bool(torch.isnan(od).any()) and not bool(torch.isnan(dq).any())
    assert err["o"] < 2e-5
    assert err["dq"] < 5e-5
    if "lse" in err:
        assert err["lse"] < 2e-5
    # the k and v parts of d_qkv at padded rows are written, as exact zeros
    for b, n in enumerate(lengths or []):
        assert bool((dq[n:, b, E:] == 0).all()), (b, n)


@pytest.mark.parametrize("case", FAMILIES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_flags_zero_gives_the_bits_of_the_len_pair(lib, case, p):
    """test 3: with and without lengths, keep words or not"""
    S, B, E, H, lengths = CASES[case]
    lengths = lengths or [max(1, S - 3 * b) for b in range(B)]
    qkv, do = inputs(S, B, E, H)
    for kw in (False, True):
        for lens in (lengths, None):
            a = run(lib, qkv, do, lens, H, p, keep_words=kw, entry="len")
            b_ = run(lib, qkv, do, lens, H, p, keep_words=kw, flags=0)
            assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2]), (kw, lens)
            if writes_lse(E, H, S):
                assert torch.equal(a[1], b_[1]), (kw, lens)


@pytest.mark.parametrize("case", WITH_FUTURE)
def test_the_future_changes_no_bit(lib, case):
    """test 4: q, k and v at rows > t replaced by large finite noise — o and lse at rows <= t keep every bit"""
    S, B, E, H, lengths = CASES[case]
    qkv, do = inputs(S, B, E, H)
    g = torch.Generator().manual_seed(99)
    for p in (0.0, 0.1):
        base = run(lib, qkv, do, lengths, H, p, keep_words=False)
        for t in edges(S):
            other = qkv.clone()
            other[t + 1:] = torch.randn(S - t - 1, B, 3 * E, generator=g) * 40.0 + 3.0
            a = run(lib, other, do, lengths, H, p, keep_words=False)
            assert torch.equal(a[0][:t + 1], base[0][:t + 1]), (p, t)
            assert not torch.equal(a[0][t + 1:], base[0][t + 1:]), (p, t)          # the replaced rows themselves do change
            if writes_lse(E, H, S):
                assert torch.equal(a[1][:, :t + 1], base[1][:, :t + 1]), (p, t)


@pytest.mark.parametrize("case", WITH_FUTURE)
def test_the_backward_does_not_leak_into_the_future(lib, case):
    """test 5: with d_o zero at rows > t, all of d_qkv at rows > t is exactly zero — and through the _len call (bidirectional)
    the same inputs give non-zero k and v gradients there"""
    S, B, E, H, lengths = CASES[case]
    qkv, do = inputs(S, B, E, H)
    for p, kw in ((0.0, False), (0.1, False), (0.1, True)):
        for t in edges(S)[::2]:
            cut = do.clone()
            cut[t + 1:] = 0.0
            dq = run(lib, qkv, cut, lengths, H, p, keep_words=kw)[2]
            assert bool((dq[t + 1:] == 0).all()), (p, kw, t)
            assert bool((dq[:t + 1, :, E:] != 0).any()), (p, kw, t)
            if not kw:
                bi = run(lib, qkv, cut, lengths, H, p, keep_words=False, entry="len")[2]
                n0 = S if lengths is None else lengths[0]
                if t + 1 < n0:                                      # dialogue 0 has real keys past t: they received gradient
                    assert bool((bi[t + 1:n0, 0, E:] != 0).any()), (p, t)


@pytest.mark.parametrize("case", ["hd10_17", "hd64_40", "hd64_49", "hd6_7"])
def test_an_unknown_flag_bit_is_refused_and_nothing_is_written(lib, case):
    """test 6"""
    S, B, E, H, lengths = CASES[case]
    qkv, do = inputs(S, B, E, H)
    for flags in (2, 3, 0x80000000):
        od, lse, dq, (rc_f, msg_f, rc_b, msg_b) = run(lib, qkv, do, lengths, H, 0.1, keep_words=True, flags=flags, check=False)
        assert rc_f != 0 and rc_b != 0
        assert b"flag" in msg_f and b"flag" in msg_b
        assert bool(torch.isnan(od).all()) and bool(torch.isnan(lse).all()) and bool(torch.isnan(dq).all())
