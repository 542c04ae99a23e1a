"""ganffn_attention_fwd_len / _bwd_len: self-attention in which dialogue b attends over its first key_len[b] keys only, on
every kernel the dispatch reaches, against the fp64 oracle with the same Philox mask (tests/key_len_oracle.py).  Bounds: the
project's own for these kernels (tests/test_hip_ops.py::test_attention_fwd_bwd) — masking only removes terms from the same
sums."""
import ctypes as C

import pytest
import torch

from oracle import ganffn_oracle as O
from key_len_oracle import masked_attention, masked_lse

pytestmark = pytest.mark.gpu

SEED, OFF, ADD, LAYER = 777, 11, 4, 2
SITE = O.SITE_LAYER0 + 4 * LAYER

CASES = {
    # 16-row kernels, head_dim 10
    "hd10_17": (17, 4, 20, 2, [17, 16, 1, 5]),
    "hd10_33": (33, 3, 20, 2, [33, 32, 17]),
    "hd10_110": (110, 2, 20, 2, [110, 97]),
    "hd10_94_10heads": (94, 2, 100, 10, [94, 48]),
    "hd10_400_problems": (17, 200, 20, 2, [1 + b % 17 for b in range(200)]),      # the path without keep words
    # four query tiles at B H >= 512: whole workgroups (fewer problems are cut in two: hd10_94_10heads, hd30_50)
    "hd10_520_problems": (50, 52, 100, 10, [50, 1] + [1 + (7 * b) % 50 for b in range(50)]),
    # 16-row, head_dim 30
    "hd30_17": (17, 3, 60, 2, [17, 1, 16]),
    "hd30_33": (33, 2, 60, 2, [33, 20]),
    "hd30_50": (50, 2, 60, 2, [50, 33]),
    "hd30_512_problems": (50, 128, 120, 4, [50, 1] + [1 + (7 * b) % 50 for b in range(126)]),
    # 16-row, head_dim 64 / 60 (S <= 48)
    "hd64_40": (40, 2, 128, 2, [40, 17]),
    "hd60_48": (48, 2, 120, 2, [48, 33]),
    # 32-row, head_dim 64 / 60
    "hd64_49": (49, 3, 128, 2, [49, 33, 32]),
    "hd60_65": (65, 2, 120, 2, [65, 64]),
    "hd64_94": (94, 2, 512, 8, [94, 1]),
    # run-time head_dim
    "hd4_33": (33, 2, 8, 2, [33, 32]),
    "hd32_65": (65, 2, 128, 4, [65, 64]),
    "hd6_7": (7, 3, 18, 3, [7, 1, 4]),
}
# two shapes per kernel family for the full-length bit equality
FULL = ["hd10_17", "hd10_94_10heads", "hd30_17", "hd30_33", "hd64_40", "hd60_48", "hd64_49", "hd60_65", "hd4_33", "hd32_65"]


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


def run_len(lib, qkv, do, lengths, H, p, keep_words, key_len="given"):
    """the _len pair on the device -> (o, lse, d_qkv), every output starting as NaN.  key_len=None: a NULL pointer."""
    S, B, E = do.shape
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    qd, dod = qkv.cuda().contiguous(), do.cuda().contiguous()
    kl = None if key_len is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    keep = torch.zeros(int(lib.load().ganffn_attention_keep_words(B, H)), dtype=torch.int32, device="cuda") if keep_words else None
    od = torch.full((S, B, E), float("nan"), device="cuda")
    lse = torch.full((B * H, S), float("nan"), device="cuda")
    dq = torch.full((S, B, 3 * E), float("nan"), device="cuda")
    lib.call("ganffn_attention_fwd_len", ptr(qd), ptr(od), ptr(lse), ptr(keep), ptr(kl), S, B, E, H, C.c_float(p), C.c_uint32(SITE),
             ptr(rng), C.c_uint64(ADD), stream())
    lib.call("ganffn_attention_bwd_len", ptr(qd), ptr(od), ptr(lse), ptr(dod), ptr(keep), ptr(kl), ptr(dq), S, B, E, H, C.c_float(p),
             C.c_uint32(SITE), ptr(rng), C.c_uint64(ADD), stream())
    torch.cuda.synchronize()
    return od, lse, dq


def oracle(qkv, do, lengths, B, H, p):
    q = qkv.detach().clone().double().requires_grad_(True)
    saved = O.ENC_DROPOUT
    O.ENC_DROPOUT = p
    try:
        with masked_attention(lengths):
            o_ref = O.attention(q, B, H, LAYER, O.Rng(SEED, OFF + ADD, train=p > 0))
    finally:
        O.ENC_DROPOUT = saved
    (o_ref * do.double()).sum().backward()
    return o_ref.detach(), q.grad


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_key_len_fwd_bwd(lib, case, p):
    S, B, E, H, lengths = CASES[case]
    qkv, do = inputs(S, B, E, H)
    o_ref, dq_ref = oracle(qkv, do, lengths, B, H, p)
    od, lse, dq = run_len(lib, qkv, do, lengths, H, p, keep_words=False)
    od2, lse2, dq2 = run_len(lib, qkv, do, lengths, H, p, keep_words=True)
    assert torch.equal(od, od2) and torch.equal(dq, dq2)          # keep words or Philox calls: the same bits
    err = {"o": rel_err(od, o_ref), "dq": rel_err(dq, dq_ref)}
    if writes_lse(E, H, S):
        assert torch.equal(lse, lse2)
        err["lse"] = rel_err(lse, masked_lse(qkv, B, H, lengths))
    print(case, p, err)
    assert err["o"] < 2e-5
    assert err["dq"] < 5e-5
    if "lse" in err:
        assert err["lse"] < 2e-5
    # the k and v parts of d_qkv at padded rows are written, as exact zeros
    for b, n in enumerate(lengths):
        assert bool((dq[n:, b, E:] == 0).all()), (b, n)


@pytest.mark.parametrize("case", FULL)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_full_lengths_give_the_bits_of_the_plain_pair(lib, case, p):
    S, B, E, H, _ = CASES[case]
    qkv, do = inputs(S, B, E, H)
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device="cuda")
    qd, dod = qkv.cuda().contiguous(), do.cuda().contiguous()
    od = torch.full((S, B, E), float("nan"), device="cuda")
    lse = torch.full((B * H, S), float("nan"), device="cuda")
    dq = torch.full((S, B, 3 * E), float("nan"), device="cuda")
    lib.call("ganffn_attention_fwd", ptr(qd), ptr(od), ptr(lse), S, B, E, H, C.c_float(p), C.c_uint32(SITE), ptr(rng),
             C.c_uint64(ADD), stream())
    lib.call("ganffn_attention_bwd", ptr(qd), ptr(od), ptr(lse), ptr(dod), ptr(dq), S, B, E, H, C.c_float(p), C.c_uint32(SITE),
             ptr(rng), C.c_uint64(ADD), stream())
    for kw in (False, True):
        for key_len in ("given", None):                         # lengths == S, and a NULL pointer
            o2, lse2, dq2 = run_len(lib, qkv, do, [S] * B, H, p, keep_words=kw, key_len=key_len)
            assert torch.equal(o2, od) and torch.equal(dq2, dq), (kw, key_len)
            if writes_lse(E, H, S):
                assert torch.equal(lse2, lse), (kw, key_len)


@pytest.mark.parametrize("case", list(CASES))
def test_values_at_padded_rows_change_no_bit(lib, case):
    S, B, E, H, lengths = CASES[case]
    qkv, do = inputs(S, B, E, H)
    other = qkv.clone()
    g = torch.Generator().manual_seed(99)
    for b, n in enumerate(lengths):
        other[n:, b, E:] = torch.randn(S - n, 2 * E, generator=g) * 40.0 + 3.0        # k and v of the padded rows
    assert not torch.equal(other, qkv)
    for p in (0.0, 0.1):
        for kw in (False, True):                                # the Philox-recomputing backward and the saved-keep-words one
            a = run_len(lib, qkv, do, lengths, H, p, keep_words=kw)
            b_ = run_len(lib, other, do, lengths, H, p, keep_words=kw)
            assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2]), (p, kw)
            if writes_lse(E, H, S):
                assert torch.equal(a[1], b_[1]), (p, kw)
            for b, n in enumerate(lengths):
                assert bool((b_[2][n:, b, E:] == 0).all()), (b, n, kw)


@pytest.mark.parametrize("case", ["hd10_17", "hd60_48", "hd64_49", "hd6_7"])
def test_out_of_range_lengths_are_clamped(lib, case):
    S, B, E, H, _ = CASES[case]
    qkv, do = inputs(S, B, E, H)
    for bad, good in ((0, 1), (S + 5, S), (-3, 1)):
        for p, kw in ((0.1, False), (0.1, True), (0.0, False)):
            a = run_len(lib, qkv, do, [bad] * B, H, p, keep_words=kw)
            b_ = run_len(lib, qkv, do, [good] * B, H, p, keep_words=kw)
            assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2]), (bad, good, p, kw)
            assert not bool(torch.isnan(a[0]).any()) and not bool(torch.isnan(a[2]).any())
            if writes_lse(E, H, S):
                assert torch.equal(a[1], b_[1]) and not bool(torch.isnan(a[1]).any()), (bad, good, p, kw)
