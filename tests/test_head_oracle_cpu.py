"""tests/head_oracle.py against stock torch, and its dropout pattern against the Philox contract (no GPU)."""
import pytest
import torch

import head_cases as HC
import head_oracle as HO
from oracle import ganffn_oracle as O
from oracle import philox


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _stock(kind, tensors, d_out):
    """the reference's head (model.py:1223-1228 / 1322-1326) from nn.Linear, nn.GELU() and torch.sigmoid in fp64, eval mode"""
    x, w1, b1, w2, b2, w3, b3 = tensors
    act = torch.nn.GELU()

    def linear(w, b):
        m = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            m.weight.copy_(w.double())
            m.bias.copy_(b.double())
        return m

    fc1, fc2 = linear(w1, b1), linear(w2, b2)
    xs = x.double().clone().requires_grad_(True)
    t = act(fc2(act(fc1(act(xs)))))
    G = {"w1": fc1.weight, "b1": fc1.bias, "w2": fc2.weight, "b2": fc2.bias}
    if kind == HO.DISC:
        fc3 = linear(w3, b3)
        t = torch.sigmoid(fc3(t))
        G.update(w3=fc3.weight, b3=fc3.bias)
    (t * d_out.double()).sum().backward()
    grads = {k: v.grad for k, v in G.items()}
    grads["x"] = xs.grad
    return t.detach(), grads


@pytest.mark.parametrize("E,D1,D2", HC.WIDTHS)
@pytest.mark.parametrize("kind", [HO.GEN, HO.DISC])
def test_head_oracle_without_dropout_is_stock_torch(kind, E, D1, D2):
    """forward and every gradient to 1e-12 of the largest reference value, at every width the GPU tests use; p = 0.2 with
    train off and p = 0 with train on are both the dropout-free head"""
    T = 7
    tensors, d_out, _ = HC.head_inputs(kind, T, E, D1, D2)
    ref, gref = _stock(kind, tensors, d_out)
    for p, rng in ((0.2, None), (0.2, O.Rng(5, 1, False)), (0.0, O.Rng(5, 1, True))):
        out, g = HO.head_run(kind, tensors, d_out, p, rng)
        assert out.shape == ref.shape
        assert _rel(out, ref) < 1e-12
        assert sorted(g) == sorted(gref)
        for k in gref:
            assert _rel(g[k], gref[k]) < 1e-12, k


@pytest.mark.parametrize("T", [5, 70])
def test_head_oracle_dropout_pattern_is_the_philox_contract(T):
    """T no multiple of 4 (a Philox call covers 4 rows): a generator's output is 0 exactly where the SITE_HEAD2 mask drops and
    its input gradient exactly where SITE_HEAD0 drops; a discriminator's probability is 0.5 exactly where SITE_HEAD3 drops"""
    p, seed, off = 0.2, (9 << 32) + 77, 14
    rng = O.Rng(seed, off, True)
    E, D1, D2 = 100, 64, 16
    tensors, d_out, _ = HC.head_inputs(HO.GEN, T, E, D1, D2)
    out, g = HO.head_run(HO.GEN, tensors, d_out, p, rng)
    keep2 = torch.from_numpy(philox.keep_mask(T, D2, p, O.SITE_HEAD2, seed, off))
    keep0 = torch.from_numpy(philox.keep_mask(T, E, p, O.SITE_HEAD0, seed, off))
    assert 0 < int((~keep2).sum()) < keep2.numel()
    assert torch.equal(out == 0, ~keep2)
    assert torch.equal(g["x"] == 0, ~keep0)
    tensors, d_out, _ = HC.head_inputs(HO.DISC, T, E, D1, D2)
    prob, g = HO.head_run(HO.DISC, tensors, d_out, p, rng)
    keep3 = torch.from_numpy(philox.keep_mask(T, 1, p, O.SITE_HEAD3, seed, off))
    assert T < 70 or 0 < int((~keep3).sum())
    assert torch.equal(prob == 0.5, ~keep3)
    # the kept values carry the 1 / (1 - p) scale: with every mask forced to keep, the oracle is the p = 0 head times the scales
    # of its sites — checked where it is cheap to state: a discriminator's fc3 bias gradient is sum_t d_out * prob * (1 - prob) * m3
    m3 = keep3.double() / (1 - p)
    assert _rel(g["b3"], (d_out.double() * prob * (1 - prob) * m3).sum(0)) < 1e-12
