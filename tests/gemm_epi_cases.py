"""The cases of tests/test_hip_gemm_epilogues.py, shared with tests/test_gemm_epi_cases_cpu.py: the shape tables, the seeded
inputs, the fp64 / fp32 references of the three epilogues ganffn_gemm_hook offers, and the 1-bit ReLU / dropout pattern in
the layout the kernels use (csrc/common.h EpiArgs::mask_out).

Every weight is generated as [N x K]; mode 1 (C = A W, W [K x N]) is handed its transpose, so one reference serves both."""
import functools
import math

import numpy as np
import torch

from oracle import philox

SEED, OFF, ADD = (5 << 32) + 20261019, 3, 11          # rng {seed > 2^32, offset 3}, rng_offset_add 11
SITE = 18
MODES = [(1, 0.2), (1, 0.0), (0, 0.2)]                # (train, p)
MODE_IDS = ["train-p0.2", "train-p0", "eval-p0.2"]
KINK = 1e-5                                           # |pre-activation| <= KINK: the sign of a ReLU input is rounding's

# (M, N, K).  M: 1 one row; 33 M % 64 in 1..32 (a wave wholly past M); 64 exactly full; 97 M % 64 = 33; 130 M % 4 != 0 with a
# Philox 4-row group cut by M.  N: 36, 100, 132 ragged, 64 full, 4 (mode 0 only below a wave tile).  K: 4, 68, 128 on the
# K <= 128 instantiation (68: K % 16 != 0), 132, 516 on the long-K one.
SHAPES = [(1, 64, 4), (33, 36, 68), (64, 64, 128), (97, 132, 132), (130, 100, 516), (97, 4, 68), (130, 132, 128), (33, 100, 132),
          (64, 36, 516), (97, 64, 4), (1, 132, 132), (130, 64, 68), (64, 100, 132)]
# the smallest shape the weight-resident kernel takes (K = 100, N >= 1024): M = 70 is two token tiles, the second with 6 rows.
# With the tables above that is every family of gemm_plan (csrc/gemm.hip) under the three epilogues in both operand modes:
# K = 128 is the last K of the short-K class, K = 132 the first of the generic one
WRES_SHAPE = (70, 1024, 100)
SHAPES = SHAPES + [WRES_SHAPE]
EPI0_CASES = [(0, s) for s in SHAPES] + [(1, s) for s in SHAPES if s[1] != 4]
# K = 100: N >= 1024 runs on the weight-resident kernel, N < 1024 on the generic K <= 128 instantiation; the last two: the
# shapes of the d_model-512 stack's linear1 / a long K
EPI1_SHAPES = SHAPES + [(161, 2048, 100), (161, 132, 100), (65, 2048, 512), (97, 512, 2048)]
EPI3_CASES = EPI0_CASES
# (M, N, K), max_slabs, the slab count of today's rule (asserted only as >= 2 / == 1 by the GPU test)
SPLIT_CASES = [((97, 132, 516), 8, 2), ((33, 36, 2048), 8, 8), ((130, 100, 1800), 8, 6), ((130, 100, 1800), 4, 4),
               ((64, 64, 508), 8, 1)]
K100_T = [1, 33, 97, 1100]                            # ganffn_ffn_k100_hook: 1100 = 18 token tiles, the last with 12 rows

FLT_MIN, SUBNORMAL = 1.1754943508222875e-38, 1e-40
SPECIALS = [0.0, -0.0, -1.5, FLT_MIN, SUBNORMAL]


def floor_bound(K):
    """the project's GEMM tolerance (tests/test_hip_ops.py test_gemm_nt) for a reduction of length K"""
    return 2e-6 * max(1.0, math.sqrt(K))


def rel_err(a, b, where=None):
    """tests/test_hip_ops.py rel_err (largest absolute error over largest absolute reference value), optionally over the
    elements `where` only"""
    a, b = a.double().cpu(), b.double().cpu()
    d = (a - b).abs()
    if where is not None:
        d = d * where
    return float(d.max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def inputs(M, N, K):
    """x [M x K] ~ randn, w [N x K] ~ randn / 10, bias [N] ~ randn / 10, aux [M x N] ~ randn (the fused residual of epi 0)"""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)          # (test_gemm_nt's seed rule)
    x, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / 10, torch.randn(N, generator=g) / 10
    return x, w, bias, torch.randn(M, N, generator=g)


@functools.lru_cache(maxsize=None)
def saved_activation(M, N):
    """the `aux` of epi 3: randn with +0, -0, a negative value, FLT_MIN and a subnormal at every third element in turn"""
    g = torch.Generator().manual_seed(104729 * M + N)
    a = torch.randn(M * N, generator=g)
    at = torch.arange(0, M * N, 3)
    a[at] = torch.tensor(SPECIALS, dtype=torch.float32)[torch.arange(at.numel()) % len(SPECIALS)]
    assert float(a[at[4 % at.numel()]]) != 0.0 or at.numel() <= 4          # the host keeps the subnormal
    return a.view(M, N)


def keep_mask(M, N, p, train, site=SITE):
    if not (train and p > 0):
        return torch.ones(M, N, dtype=torch.bool)
    return torch.from_numpy(philox.keep_mask(M, N, p, site, SEED, OFF + ADD))


def ref_epi0(x, w, bias=None, aux=None, dtype=torch.float64):
    """A W^T + bias (+ aux)"""
    y = x.to(dtype) @ w.to(dtype).T
    if bias is not None:
        y = y + bias.to(dtype)
    if aux is not None:
        y = y + aux.to(dtype)
    return y


def ref_epi1(x, w, bias, p, train, dtype=torch.float64, site=SITE):
    """relu(A W^T + bias) * keep / (1 - p) -> (value, pre-activation)"""
    pre = x.to(dtype) @ w.to(dtype).T + bias.to(dtype)
    y = torch.relu(pre)
    if train and p > 0:
        y = y * keep_mask(*pre.shape, p, train, site).to(dtype) / (1 - p)
    return y, pre


def ref_epi3(x, w, aux, p, train, dtype=torch.float64):
    """(A W^T) * (aux > 0) * (1 / (1 - p) if train and p > 0 else 1); the predicate is IEEE's on the fp32 aux"""
    y = (x.to(dtype) @ w.to(dtype).T) * (aux > 0).to(dtype)
    return y / (1 - p) if train and p > 0 else y


_ROW_OF_BIT = np.array([(i & 3) + 8 * (i >> 2) for i in range(16)])


def pattern_words(h):
    """the uint16 pattern words of an [M x N] activation: word [(rt * N + col) * 2 + hh], bit i <-> h[row, col] > 0 at
    row = rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh; bits of rows >= M are 0 here (the kernels leave them unspecified)"""
    pos = (torch.as_tensor(h) > 0).cpu().numpy()
    M, N = pos.shape
    RT = (M + 31) // 32
    pad = np.zeros((RT * 32, N), dtype=bool)
    pad[:M] = pos
    pad = pad.reshape(RT, 32, N)
    words = np.zeros((RT, N, 2), dtype=np.uint16)
    for hh in range(2):
        for i in range(16):
            words[:, :, hh] |= pad[:, _ROW_OF_BIT[i] + 4 * hh, :].astype(np.uint16) << np.uint16(i)
    return words.reshape(-1)


def pattern_rows(words, M, N):
    """inverse of pattern_words: bool [M x N] (rows < M only)"""
    RT = (M + 31) // 32
    words = np.asarray(words).astype(np.uint16).reshape(RT, N, 2)
    out = np.zeros((RT, 32, N), dtype=bool)
    for hh in range(2):
        for i in range(16):
            out[:, _ROW_OF_BIT[i] + 4 * hh, :] = (words[:, :, hh] >> np.uint16(i)) & np.uint16(1) != 0
    return torch.from_numpy(out.reshape(RT * 32, N)[:M].copy())


@functools.lru_cache(maxsize=None)
def k100_dgrad_inputs(T):
    """ganffn_ffn_k100_hook which = 1: a [T x 100] ~ randn and w [2048 x 100] ~ randn / 10 (handed over as its transpose)"""
    g = torch.Generator().manual_seed(15485863 + T)
    return torch.randn(T, 100, generator=g), torch.randn(2048, 100, generator=g) / 10
