"""The cases of tests/test_hip_heads.py, shared with tests/test_head_oracle_cpu.py: the shape tables and the seeded inputs."""
import torch

from head_oracle import DISC, GEN, GRAD_KEYS

# (T, E, D1, D2) of tests/test_hip_heads.py (its comments say which path each takes)
GEN_SHAPES = [(14, 100, 512, 100), (1, 100, 512, 100), (5, 100, 512, 100), (69, 100, 512, 100), (67, 100, 1024, 100),
              (1, 100, 1024, 100), (65, 512, 1024, 100), (37, 600, 1024, 100), (37, 300, 512, 100), (33, 4, 4, 4),
              (70, 68, 132, 36), (9, 128, 60, 200)]
DISC_FUSED_SHAPES = [(T, 100, 64, 16) for T in (1, 3, 4, 5, 15, 16, 17, 63, 330, 1029)]
DISC_UNFUSED_SHAPES = [(5, 100, 64, 32), (257, 64, 16, 4), (70, 512, 64, 16), (33, 100, 128, 16), (16389, 4, 4, 4)]
# the dx product of the discriminator head (EPI_GELU_BWD, K = D1) past the short-K class (D1 = 132) and on the weight-resident
# kernel (D1 = 100, E = 1024: two token tiles, the second with 6 rows) — csrc/gemm.hip gemm_plan.  (Not part of WIDTHS: the
# recorded size tables are over the widths above.)
DISC_PLAN_SHAPES = [(33, 100, 132, 16), (70, 1024, 100, 16)]
WIDTHS = sorted({s[1:] for s in GEN_SHAPES + DISC_FUSED_SHAPES + DISC_UNFUSED_SHAPES})


def head_inputs(kind, T, E, D1, D2, seed=0):
    """seeded (x, w1, b1, w2, b2, w3, b3), d_out and non-zero initial gradient buffers {"w1": .., ..}; fp32, on the host.
    Weights at 1 / sqrt(fan-in), so that every pre-activation is of order 1 at every width."""
    g = torch.Generator().manual_seed(1000003 * kind + 7919 * T + 31 * E + 7 * D1 + D2 + 104729 * seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(T, E)
    w1, b1 = r(D1, E) / E ** 0.5, r(D1) * 0.3
    w2, b2 = r(D2, D1) / D1 ** 0.5, r(D2) * 0.3
    w3, b3 = (r(1, D2) / D2 ** 0.5, r(1) * 0.3) if kind == DISC else (None, None)
    d_out = r(T, D2 if kind == GEN else 1)
    tensors = (x, w1, b1, w2, b2, w3, b3)
    g0 = {k: r(*t.shape) * 0.5 for k, t in zip(GRAD_KEYS, tensors[1:]) if t is not None}
    return tensors, d_out, g0
