"""The fp64 restatement of GanEngine's masked sub-steps (tests/gan_mask_oracle.py) on the CPU: at full lengths it is
tests/engine_oracle.py's disc_substep / gen_substep, its loss is stock torch.nn.BCELoss over the valid positions, and its loss
gradient is autograd's.  No GPU needed."""
import numpy as np
import pytest
import torch

import engine_oracle as EO
import formula as F_
import gan_mask_oracle as GM
from key_len_oracle import valid_rows
from util import DIN, DISC, GEN, NETS, formula_sd

S, B, SEED, BASE = 6, 3, 4242, 96


def _net(cls_name, p_pe=0.2, p_enc=0.1, p_head=0.2):
    kind, _, _, H, _, _ = NETS[cls_name]
    return EO.Net(kind, formula_sd(cls_name), H, p_pe, p_enc, p_head)


def _x(m):
    return torch.from_numpy(F_.formula_input("gm." + m, S, B, DIN[m], pad_from=S - 2)).double()


def _same(a, b, what, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300), (what, np.abs(a - b).max())


def _probs(Bt, seed):
    """probabilities with exact 0 and 1 among them, inside and outside the valid region of lengths [S, 2, 1, ...]"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(S, Bt, generator=g, dtype=torch.float64) * 0.98 + 0.01
    p[0, 0], p[1, 0], p[0, 1] = 0.0, 1.0, 1.0          # valid rows of dialogues 0 and 1
    p[S - 1, 1], p[S - 2, 2] = 0.0, 1.0                # padded rows of dialogues 1 and 2
    return p


@pytest.mark.parametrize("lens", [[S, 2, 1], [S, S, S], [0, 99, 3]])
def test_masked_bce_is_stock_bceloss_over_the_valid_positions(lens):
    p = _probs(B, 1)
    y = (torch.arange(S * B).view(S, B) % 2).double()
    y[0, 0], y[1, 0] = 1.0, 0.0                        # against p = 0 and p = 1: a clamped log(0) = -100 each
    valid = valid_rows(S, GM.clamp_lengths(lens, S))
    want = torch.nn.BCELoss()(p[valid], y[valid])
    got = GM.masked_bce(p, y, lens)
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
    assert float(want) > 5.0                           # the -100 clamp took part: a term of 100 among <= 18 valid positions
    # the discriminator's form: [real | fake] with the lengths twice = the mean of the two halves' masked means
    p2 = torch.cat((p, _probs(B, 2)), dim=1)
    both = GM.masked_bce(p2, GM.disc_targets(S, B), list(lens) + list(lens))
    halves = (GM.masked_bce(p2[:, :B], 1.0, lens) + GM.masked_bce(p2[:, B:], 0.0, lens)) / 2.0
    assert abs(float(both) - float(halves)) <= 1e-12 * abs(float(halves))


def test_masked_bce_grad_is_autograds_and_zero_on_padding():
    lens = [S, 2, 1]
    g = torch.Generator().manual_seed(3)
    p = (torch.rand(S, B, 1, generator=g, dtype=torch.float64) * 0.98 + 0.01).requires_grad_(True)
    (3.0 * GM.masked_bce(p, 1.0, lens)).backward()
    got = GM.masked_bce_grad(p.detach(), 1.0, lens, scale=3.0)
    _same(got, p.grad, "dprob")
    pad = ~valid_rows(S, lens)
    assert bool((got[..., 0][pad] == 0).all()) and bool((got[..., 0][~pad] != 0).all())


@pytest.mark.parametrize("who,partner,i", [("visual", "acoustic", 0), ("text", "visual", 8)])
def test_masked_disc_substep_at_full_lengths_is_the_unmasked_one(who, partner, i):
    xr, xp = _x(who), _x(partner)
    want = EO.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i)
    got = GM.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i, [S] * B)
    assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    _same(got["fake"], want["fake"], "fake")
    _same(got["prob"], want["prob"], "prob")
    assert set(got["grads"]) == set(want["grads"])
    for k in want["grads"]:
        _same(got["grads"][k], want["grads"][k], k)
    # and ragged lengths give another step
    rag = GM.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i, [S, 2, 1])
    assert abs(rag["loss"] - want["loss"]) > 1e-6 * abs(want["loss"])


@pytest.mark.parametrize("who,partner,i", [("text", "acoustic", 7), ("visual", "text", 9)])
def test_masked_gen_substep_at_full_lengths_is_the_unmasked_one(who, partner, i):
    x = _x(who)
    want = EO.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i)
    got = GM.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i, [S] * B)
    assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    _same(got["out"], want["out"], "out")
    for k in want["grads"]:
        _same(got["grads"][k], want["grads"][k], k)
    rag = GM.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i, [S, 2, 1])
    assert abs(rag["loss"] - want["loss"]) > 1e-6 * abs(want["loss"])
