"""The fp64 restatement of GanEngine's causal sub-steps (tests/gan_causal_oracle.py) on the CPU: at S = 1, where the causal mask
removes nothing, it is tests/engine_oracle.py's disc_substep / gen_substep; a generator's output at rows < t does not depend on
input rows >= t while the bidirectional discriminator's answer at row 0 does; and with full lengths the lengths form is the form
without lengths.  No GPU needed."""
import numpy as np
import pytest
import torch

import engine_oracle as EO
import formula as F_
import gan_causal_oracle as GC
from util import DIN, DISC, GEN, NETS, formula_sd

S, B, SEED, BASE = 6, 3, 4242, 96


def _net(cls_name, p_pe=0.2, p_enc=0.1, p_head=0.2):
    kind, _, _, H, _, _ = NETS[cls_name]
    return EO.Net(kind, formula_sd(cls_name), H, p_pe, p_enc, p_head)


def _x(m, S_=S):
    return torch.from_numpy(F_.formula_input("gc." + m, S_, B, DIN[m], pad_from=S_)).double()


def _same(a, b, what, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300), (what, np.abs(a - b).max())


def _same_step(got, want, out):
    assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    for k in out:
        _same(got[k], want[k], k)
    assert set(got["grads"]) == set(want["grads"])
    for k in want["grads"]:
        _same(got["grads"][k], want["grads"][k], k)


@pytest.mark.parametrize("who,partner,i", [("visual", "acoustic", 0), ("text", "visual", 8)])
def test_causal_disc_substep_at_one_utterance_is_the_bidirectional_one(who, partner, i):
    xr, xp = _x(who, 1), _x(partner, 1)
    want = EO.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i)
    _same_step(GC.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i), want, ("fake", "prob"))
    _same_step(GC.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i, [1] * B), want, ("fake", "prob"))
    # and at more than one utterance the causal generators make it another step
    xr, xp = _x(who), _x(partner)
    plain = EO.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i)
    causal = GC.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i)
    assert float((causal["fake"] - plain["fake"]).abs().max()) > 1e-3 * float(plain["fake"].abs().max())


@pytest.mark.parametrize("who,partner,i", [("text", "acoustic", 7), ("visual", "text", 9)])
def test_causal_gen_substep_at_one_utterance_is_the_bidirectional_one(who, partner, i):
    x = _x(who, 1)
    want = EO.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i)
    _same_step(GC.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i), want, ("out",))
    _same_step(GC.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i, [1] * B), want, ("out",))
    x = _x(who)
    plain = EO.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i)
    causal = GC.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i)
    assert float((causal["out"] - plain["out"]).abs().max()) > 1e-3 * float(plain["out"].abs().max())
    assert abs(causal["loss"] - plain["loss"]) > 1e-9 * abs(plain["loss"])


@pytest.mark.parametrize("lens", [None, [S, 2, 4]], ids=["no lengths", "ragged"])
def test_generators_never_look_ahead_and_discriminators_do(lens):
    who, partner, t = "text", "acoustic", 3
    x = _x(who)
    later = x.clone()
    later[t:] += torch.from_numpy(F_.formula_input("gc.later", S - t, B, DIN[who], pad_from=S)).double() + 0.5
    # the fake of a discriminator sub-step (eval mode) and the output of a generator sub-step (train mode)
    a, b = (GC.generator_eval(_net(GEN[who]), v, SEED, BASE, 4, lens) for v in (x, later))
    assert torch.equal(a[:t], b[:t]) and not torch.equal(a[t], b[t])
    D = DISC[partner]
    ga, gb = (GC.gen_substep(_net(GEN[who]), _net(D), v, SEED, BASE, 5, lens) for v in (x, later))
    assert torch.equal(ga["out"][:t], gb["out"][:t]) and not torch.equal(ga["out"][t], gb["out"][t])
    # the discriminator that judges those rows is bidirectional: its probabilities at row 0 move with the later rows (dialogue 0
    # has every utterance in both cases; the largest move over the row, since the head's last dropout site zeroes some logits),
    # over the fake half and over the real half alike
    xr = _x(partner)
    da, db = (GC.disc_substep(_net(D), _net(GEN[who]), r, v, SEED, BASE, 4, lens)
              for r, v in ((xr, x), (xr, later)))
    assert torch.equal(da["fake"][:t], db["fake"][:t])
    assert float((da["prob"][0, B:] - db["prob"][0, B:]).abs().max()) > 1e-9     # row 0 of the fake half
    later_r = xr.clone()
    later_r[t:] += 0.5
    dc = GC.disc_substep(_net(D), _net(GEN[who]), later_r, x, SEED, BASE, 4, lens)
    assert float((da["prob"][0, :B] - dc["prob"][0, :B]).abs().max()) > 1e-9     # row 0 of the real half


@pytest.mark.parametrize("who,partner,i", [("visual", "acoustic", 0), ("acoustic", "text", 6)])
def test_full_lengths_are_the_form_without_lengths_disc(who, partner, i):
    xr, xp = _x(who), _x(partner)
    want = GC.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i)
    _same_step(GC.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i, [S] * B), want, ("fake", "prob"))
    rag = GC.disc_substep(_net(DISC[who]), _net(GEN[partner]), xr, xp, SEED, BASE, i, [S, 2, 1])
    assert abs(rag["loss"] - want["loss"]) > 1e-6 * abs(want["loss"])


@pytest.mark.parametrize("who,partner,i", [("text", "acoustic", 7), ("visual", "text", 9)])
def test_full_lengths_are_the_form_without_lengths_gen(who, partner, i):
    x = _x(who)
    want = GC.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i)
    _same_step(GC.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i, [S + 3] * B), want, ("out",))
    rag = GC.gen_substep(_net(GEN[who]), _net(DISC[partner]), x, SEED, BASE, i, [S, 2, 1])
    assert abs(rag["loss"] - want["loss"]) > 1e-6 * abs(want["loss"])
