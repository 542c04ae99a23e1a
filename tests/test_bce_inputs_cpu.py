"""The inputs and bounds of tests/test_hip_bce_adam.py's BCE cases, checked without a GPU: where the planted values sit, that
no seeded probability falls at the 1e-12 clamp of the backward, and that the kernel's expressions evaluated in fp32 on the
CPU hold the bounds the GPU test sets (so a miss on the GPU is the kernel's, not fp32's)."""
import itertools

import torch
import torch.nn.functional as F

from bce_cases import BCE_N, BCE_PERIODS, BCE_TARGETS, CLAMP, PLANTED, UNDERFLOW, bce_probs, bce_targets, f32


def test_no_seeded_probability_sits_at_the_backward_clamp():
    for n in BCE_N:
        p, seeded = bce_probs(n)
        q = p.double() * (1 - p.double())
        band = (q - CLAMP).abs() <= 1e-6 * CLAMP
        assert int((band & seeded).sum()) == 0
        assert int((~seeded).sum()) == (6 if n >= 6 else max(min(n - 1, 4), 0))
        assert bool(((p >= 0) & (p <= 1)).all())
    p, _ = bce_probs(1023)
    assert sorted(p[[0, 1, 341, 511, 1021, 1022]].tolist()) == sorted(f32(v) for v in PLANTED)
    assert 0.0 < float(p[341]) < 1e-44 and float(p[1021]) < 1.0 == float(p[1])


def test_periodic_targets():
    assert bce_targets(8, 0, 0, 1.0, 0.0).tolist() == [1.0] * 8
    assert bce_targets(8, 6, 3, 1.0, 0.0).tolist() == [1, 1, 1, 0, 0, 0, 1, 1]
    assert bce_targets(7, 6, 0, 1.0, 0.0).tolist() == [0.0] * 7
    assert bce_targets(7, 6, 6, 1.0, 0.0).tolist() == [1.0] * 7
    assert bce_targets(9, 7, 2, 0.9, 0.1).tolist() == [f32(0.9)] * 2 + [f32(0.1)] * 5 + [f32(0.9)] * 2


def test_fp32_arithmetic_holds_the_bounds_of_the_gpu_test():
    """loss = scale * mean(-(y max(log p, -100) + (1 - y) max(log(1 - p), -100))), dprob = scale / n * (p - y) / max(p (1 - p),
    1e-12), in fp32 op by op as the kernels write them, against the fp64 torch reference: 1e-5 on the loss, 1e-5 on every
    element of dprob — the planted 1e-12 included"""
    for n, (period, split), (ta, tb), scale in itertools.product(BCE_N, BCE_PERIODS, BCE_TARGETS, (1.0, 0.5)):
        p, _ = bce_probs(n)
        y = bce_targets(n, period, split, ta, tb)
        p64 = p.double().requires_grad_(True)
        ref = F.binary_cross_entropy(p64, y) * scale
        (gref,) = torch.autograd.grad(ref, p64)
        y32, one = y.float(), torch.tensor(1.0)
        terms = -(y32 * torch.log(p).clamp_min(-100.0) + (one - y32) * torch.log(one - p).clamp_min(-100.0))
        loss32 = terms.sum() * torch.tensor(scale) / torch.tensor(float(n))
        assert abs(float(loss32) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
        d32 = torch.tensor(scale) / torch.tensor(float(n)) * (p - y32) / (p * (one - p)).clamp_min(torch.tensor(1e-12))
        assert bool(((d32.double() - gref).abs() <= 1e-5 * gref.abs() + UNDERFLOW).all())
