"""The BCE cases of tests/test_hip_bce_adam.py, shared with tests/test_bce_inputs_cpu.py: sizes, targets, seeded inputs."""
import numpy as np
import torch

BCE_N = [1, 5, 1023, 1024, 1025, 6016]                     # both sides of the 1024-thread stride of the one-workgroup mean
BCE_PERIODS = [(0, 0), (6, 3), (6, 0), (6, 6), (7, 2)]     # (period, split); most n are no multiple of the period
BCE_TARGETS = [(1.0, 0.0), (0.9, 0.1)]
DENORMAL = float(np.float32(2.0 ** -149))
PLANTED = [0.0, 1.0, DENORMAL, 1.0 - 2.0 ** -24, 0.5, 1e-12]
CLAMP = 1e-12
# absolute term of the elementwise dprob check: an fp32 intermediate below the normal range ((p - y) scale / n with a denormal
# p and y = 0) carries an absolute error of up to 2^-150 = 7e-46, or is flushed to 0, and is then divided by at least 1e-12
UNDERFLOW = 1e-33


def f32(v):
    """the fp32 value the kernel receives for a float argument, as a Python float"""
    return float(np.float32(v))


def bce_probs(n):
    """seeded uniform probabilities; where n allows, the planted edge values (n = 5: the first four, one seeded value stays)"""
    g = torch.Generator().manual_seed(4000 + n)
    p = torch.rand(n, generator=g)
    seeded = torch.ones(n, dtype=torch.bool)
    if n >= 6:
        where = [0, 1, n // 3, n // 2, n - 2, n - 1]
    else:
        where = list(range(max(n - 1, 0)))[:4]
    for i, v in zip(where, PLANTED):
        p[i] = v
        seeded[i] = False
    return p, seeded


def bce_targets(n, period, split, ta, tb):
    i = torch.arange(n)
    first = (i % period) < split if period > 0 else torch.ones(n, dtype=torch.bool)
    return torch.where(first, torch.tensor(f32(ta), dtype=torch.float64), torch.tensor(f32(tb), dtype=torch.float64))
