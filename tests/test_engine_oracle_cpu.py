"""The fp64 restatement of the step runner's train-mode sub-steps (tests/engine_oracle.py) against the oracle: with dropout
off it is the oracle's own train_disc / train_gen (which run D(real) and D(fake) as two passes), and with dropout on it
draws, for the real and the fake half of the [real | fake] batch, exactly the rows of the 2B-dialogue Philox layout.
No GPU needed."""
import numpy as np
import pytest
import torch

import engine_oracle as EO
import formula as F_
from oracle import ganffn_oracle as O
from test_hip_modules import oracle_head
from util import DIN, DISC, GEN, NETS, formula_sd

S, B, SEED, BASE = 6, 3, 4242, 96


def _net(cls_name, p_pe, p_enc, p_head):
    kind, _, _, H, _, _ = NETS[cls_name]
    return EO.Net(kind, formula_sd(cls_name), H, p_pe, p_enc, p_head)


def _x(tag, m):
    return torch.from_numpy(F_.formula_input("eo." + tag, S, B, DIN[m], pad_from=S - 2)).double()


def _close(a, b, what, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= rtol * scale, (what, np.abs(a - b).max(), scale)


@pytest.mark.parametrize("who,partner", [("visual", "text"), ("acoustic", "visual")])
def test_disc_substep_without_dropout_is_the_oracles_train_disc(who, partner):
    D, G = _net(DISC[who], 0.0, 0.0, 0.0), _net(GEN[partner], 0.0, 0.0, 0.0)
    xr, xp = _x(who, who), _x(partner, partner)
    got = EO.disc_substep(D, G, xr, xp, SEED, BASE, 5)
    od = O.OracleNet("disc", formula_sd(DISC[who]), D.H, 0.0, torch.float64)
    og = O.OracleNet("gen", formula_sd(GEN[partner]), G.H, 0.0, torch.float64)
    opt = O.Adam(od.parameters(), 0.0)                 # lr 0: the step leaves the parameters and their gradients alone
    valid, fake = torch.ones(S, B, 1, dtype=torch.float64), torch.zeros(S, B, 1, dtype=torch.float64)
    want = O.train_disc(od, xr, og, xp, opt, valid, fake, None)
    assert abs(got["loss"] - want) <= 1e-13 * abs(want), (got["loss"], want)
    assert set(got["grads"]) == {k for k, v in od.P.items() if v.grad is not None}
    assert ("object.weight" in got["grads"]) == (who == "visual")
    for k, g in got["grads"].items():
        _close(g, od.P[k].grad, k)


@pytest.mark.parametrize("who,partner", [("text", "acoustic"), ("visual", "acoustic")])
def test_gen_substep_without_dropout_is_the_oracles_train_gen(who, partner):
    G, D = _net(GEN[who], 0.0, 0.0, 0.0), _net(DISC[partner], 0.0, 0.0, 0.0)
    x = _x(who, who)
    got = EO.gen_substep(G, D, x, SEED, BASE, 7)
    og = O.OracleNet("gen", formula_sd(GEN[who]), G.H, 0.0, torch.float64)
    od = O.OracleNet("disc", formula_sd(DISC[partner]), D.H, 0.0, torch.float64)
    opt = O.Adam(og.parameters(), 0.0)
    want = O.train_gen(og, x, od, opt, torch.ones(S, B, 1, dtype=torch.float64), None, None)
    assert abs(got["loss"] - want) <= 1e-13 * abs(want), (got["loss"], want)
    assert set(got["grads"]) == {k for k, v in og.P.items() if v.grad is not None}
    for k, g in got["grads"].items():
        _close(g, og.P[k].grad, k)


@pytest.mark.parametrize("who,partner,i", [("visual", "acoustic", 0), ("text", "visual", 8)])
def test_disc_substep_draws_the_rows_of_the_2B_layout(who, partner, i):
    """dropout on: the real half of D's one pass uses rows (s, 0..B-1) and the fake half rows (s, B..2B-1) of the masks of
    a 2B-dialogue batch at offsets b + 4i + 2 (encoder) and b + 4i + 3 (head) — checked against the oracle run on each
    half alone with `Rng(full_batch=2B, select=...)`, which slices philox.keep_mask / attn_keep_mask of that layout"""
    D, G = _net(DISC[who], 0.2, 0.1, 0.2), _net(GEN[partner], 0.2, 0.1, 0.2)
    xr, xp = _x(who, who), _x(partner, partner)
    got = EO.disc_substep(D, G, xr, xp, SEED, BASE, i)
    P = {k: v.detach() for k, v in D.P.items()}
    real = xr @ P["object.weight"].T + P["object.bias"] if "object.weight" in P else xr
    a = BASE + 4 * i
    halves = []
    for x, sel in ((real, range(B)), (got["fake"], range(B, 2 * B))):
        h = O.encoder_stack(x, P, D.H, O.Rng(SEED, a + 2, True, full_batch=2 * B, select=sel))
        on = O.OracleNet("disc", {}, D.H)
        on.P = P
        halves.append(oracle_head(on, "disc", h, O.Rng(SEED, a + 3, True, full_batch=2 * B, select=sel)))
    _close(got["prob"][:, :B], halves[0], "real half")
    _close(got["prob"][:, B:], halves[1], "fake half")
    # the masks matter: the same pass without dropout, or with the halves' masks swapped, gives other probabilities
    D0 = _net(DISC[who], 0.0, 0.0, 0.0)
    p0 = EO.disc_substep(D0, G, xr, xp, SEED, BASE, i, fake=got["fake"])["prob"]
    assert (got["prob"] - p0).abs().max() > 1e-3
    assert (got["prob"][:, :B] - halves[1]).abs().max() > 1e-3


def test_gen_substep_draws_the_generator_offsets_and_a_frozen_eval_discriminator():
    """dropout on: the generator's masks at b + 4i (encoder) and b + 4i + 1 (head) over the B layout; the frozen
    discriminator draws none"""
    i = 3
    G, D = _net(GEN["text"], 0.2, 0.1, 0.2), _net(DISC["visual"], 0.2, 0.1, 0.2)
    x = _x("text", "text")
    got = EO.gen_substep(G, D, x, SEED, BASE, i)
    P = {k: v.detach() for k, v in G.P.items()}
    on = O.OracleNet("gen", {}, G.H)
    on.P = P
    out = oracle_head(on, "gen", O.encoder_stack(x, P, G.H, O.Rng(SEED, BASE + 4 * i, True)), O.Rng(SEED, BASE + 4 * i + 1, True))
    _close(got["out"], out, "generator output")
    prob = O.discriminator_forward(out, {k: v.detach() for k, v in D.P.items()}, D.H, 0.2, None)
    want = float(O.bce_mean(prob, torch.ones_like(prob)))
    assert abs(got["loss"] - want) <= 1e-13 * abs(want)


def test_adam_restatement_is_the_oracles_adam():
    """EO.adam (numpy, one step from given moments) against O.Adam over three steps, bias corrections included"""
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(50)
    p = torch.tensor(p0, requires_grad=True)
    opt = O.Adam([p], 1.1e-4, (0.5, 0.6))
    q, m, v = p0.copy(), np.zeros(50), np.zeros(50)
    for t in range(1, 4):
        g = rng.standard_normal(50) * 10.0 ** (-t)
        p.grad = torch.tensor(g)
        opt.step()
        q, m, v = EO.adam(q, g, m, v, t, 1.1e-4, 0.5, 0.6)
        _close(q, p.detach().numpy(), "adam t=%d" % t, 1e-15)
