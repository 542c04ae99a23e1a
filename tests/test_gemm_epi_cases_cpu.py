"""What tests/test_hip_gemm_epilogues.py rests on, checked without a GPU (tests/gemm_epi_cases.py): the pattern-word layout
round-trips, the fp32 evaluation of each reference stays inside the bound the GPU module uses (so the bound is not tighter
than fp32 arithmetic itself), and the ReLU-kink band it excludes is a negligible share of every epi-1 case."""
import numpy as np
import pytest
import torch

import gemm_epi_cases as GC


@pytest.mark.parametrize("M,N", [(1, 4), (31, 8), (32, 4), (33, 36), (97, 100), (130, 12)])
def test_pattern_words_round_trip_on_ragged_rows(M, N):
    g = torch.Generator().manual_seed(M * 131 + N)
    h = torch.randn(M, N, generator=g)
    h[0, 0], h[M - 1, N - 1] = 0.0, GC.SUBNORMAL
    words = GC.pattern_words(h)
    assert words.dtype == np.uint16 and words.shape == ((M + 31) // 32 * N * 2,)
    assert torch.equal(GC.pattern_rows(words, M, N), h > 0)
    # the layout itself, element by element: row m of column n is bit i of word [(m // 32 * N + n) * 2 + hh],
    # hh = (m // 4) & 1, i = (m & 3) + 4 * ((m % 32) // 8)
    for m in sorted({0, M // 2, M - 1}):
        for n in (0, N - 1):
            hh, i = (m // 4) & 1, (m & 3) + 4 * ((m % 32) // 8)
            assert bool((int(words[((m // 32) * N + n) * 2 + hh]) >> i) & 1) == bool(h[m, n] > 0)
    # rows past M carry no bit
    only = GC.pattern_words(torch.ones(M, N))
    assert int(np.unpackbits(only.view(np.uint8)).sum()) == M * N


def test_saved_activation_carries_every_special_value():
    a = GC.saved_activation(97, 132).view(-1)
    bits = a.view(torch.int32)
    assert int((bits == 0).sum()) > 0 and int((bits == -(1 << 31)).sum()) > 0               # +0.0 and -0.0
    assert int((a == GC.FLT_MIN).sum()) > 0 and int((a < 0).sum()) > 0
    sub = (a > 0) & (a < GC.FLT_MIN)
    assert int(sub.sum()) > 0                                                                # the subnormal, positive by IEEE
    # every special value lands both in wave tiles wholly inside a [97 x 132] matrix and in the edge tiles
    A = GC.saved_activation(97, 132)
    for region in (A[:96, :128], A[96:, :], A[:, 128:]):
        rb = region.contiguous().view(torch.int32)
        assert int((rb == 0).sum()) and int((rb == -(1 << 31)).sum()) and int(((region > 0) & (region < GC.FLT_MIN)).sum())


@pytest.mark.parametrize("shape", sorted(set(GC.SHAPES)), ids=lambda s: "x".join(map(str, s)))
def test_fp32_references_stay_inside_the_gpu_bound(shape):
    M, N, K = shape
    x, w, bias, aux = GC.inputs(M, N, K)
    floor = GC.floor_bound(K)
    e0 = GC.rel_err(GC.ref_epi0(x, w, bias, aux, dtype=torch.float32), GC.ref_epi0(x, w, bias, aux))
    assert e0 <= floor, e0
    act = GC.saved_activation(M, N)
    for train, p in GC.MODES:
        y64, pre = GC.ref_epi1(x, w, bias, p, train)
        y32, _ = GC.ref_epi1(x, w, bias, p, train, dtype=torch.float32)
        assert GC.rel_err(y32, y64, pre.abs() > GC.KINK) <= floor
        assert GC.rel_err(GC.ref_epi3(x, w, act, p, train, dtype=torch.float32), GC.ref_epi3(x, w, act, p, train)) <= floor


@pytest.mark.parametrize("case", GC.SPLIT_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-max%d" % c[1])
def test_fp32_split_reference_stays_inside_the_gpu_bound(case):
    M, N, K = case[0]
    x, w, bias, aux = GC.inputs(M, N, K)
    assert GC.rel_err(GC.ref_epi0(x, w, bias, aux, dtype=torch.float32), GC.ref_epi0(x, w, bias, aux)) <= GC.floor_bound(K)


KINK_SHAPES = GC.EPI1_SHAPES + [(T, 2048, 100) for T in GC.K100_T]


@pytest.mark.parametrize("shape", KINK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_relu_kink_band_is_a_negligible_share_of_every_epi1_case(shape):
    """at most 1e-4 of the elements have |pre-activation| <= 1e-5 (the exclusion of test_ffn_linear1_fwd_epilogue)"""
    M, N, K = shape
    x, w, bias, _ = GC.inputs(M, N, K)
    _, pre = GC.ref_epi1(x, w, bias, 0.0, 0)
    share = float((pre.abs() <= GC.KINK).double().mean())
    print("kink share %s: %.3g" % (shape, share))
    assert share <= 1e-4
