"""No encoder, head, LSTM or DialogueRNN call writes past the size its size function reports.

Every buffer a call writes (outputs, saved, workspace, K/V cache, gradients) is a tensor of exactly the reported size plus 256
guard floats of a fixed bit pattern; the call is handed the front part, and after each call every guard is compared with the
pattern.  The guard is a bounds check inside the test's own allocations: an overrun shorter than the guard shows here without
anything outside a tensor being touched.  The call lists are in workspace_bounds_cases.py.

The sizes are the smallest at which the layouts can go wrong: T = 3 rows (every round-to-4 of a layout rounds) and T = 15 (three
dialogues), two layers (a layer set above another, the cross-layer reach of the rowchain backward), at d_model 100 (rowchain,
n100 and tn100 kernels, unreduced weight gradients) and at 64 (the generic path).  The LSTM's (layer and stack calls of the
three entry-point families): S = 1 (the first step is the last: no recurrent weight gradient), one and three dialogues, 33 (two
dialogue tiles) behind the batch and packed entry points, an input wider and narrower than H (the partial slabs are sized for
the larger), 1 layer (no between-layer region) and 3 (both of the alternating gradient buffers), eval and train with p = 0.5,
packed lengths (1, 5, 3) and a ragged vector with dialogues of length 1.  The DialogueRNN's (forward and backward through
ops.drnn_fwd_raw / drnn_bwd_raw, about 60 regions that depend on attention type, listener, parties and B): S = 1, one and three
dialogues with a padded tail, 33 behind the batch entry points, one and two directions, eval and train with p = 0.5, widths
(12, 8, 4) (emotion chain) and (8, 8, 132) (the per-step emotion cell with D_e > 2 D_g, whose pre-activations and direct-path
gradient take regions sized for the wider cell), every attention type with and without the listener (general2 at S = 3, B = 1:
9 tanh scores rounded to 12; concat at D_a = 4), and 1, 2 and 16 parties (16 with the listener: 34 products in one launch);
saved and workspace start as the NaN pattern, so e, dU and every gradient must come out finite."""
import pytest
import torch

import workspace_bounds_cases as WB

pytestmark = pytest.mark.gpu


def _check_guards(seen):
    def visit(label, buffers):
        torch.cuda.synchronize()
        for name, t in buffers.items():
            assert WB.guard_intact(t), "%s: wrote past the end of %s (%d floats)" % (label, name, t.numel() - WB.GUARD)
        seen.append(label)
    return visit


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("S,B", WB.SHAPES, ids=["%dx%d" % sb for sb in WB.SHAPES])
@pytest.mark.parametrize("E,H,F", WB.WIDTHS, ids=["E%d" % w[0] for w in WB.WIDTHS])
def test_encoder_calls_stay_inside_their_buffers(E, H, F, S, B, train):
    seen = []
    WB.run_encoder_case(WB.encoder_case(E, H, F, S, B, train), _check_guards(seen))
    want = ["fwd unsaved", "fwd saved", "bwd [1,2)", "bwd [0,1)", "bwd [0,2)", "bwd no grads [0,2)"]
    want += ["bwd_parts"] if E == 100 else []
    want += ["fwd_pair"]
    want += ["stream step", "stream extend"] if not train else []
    assert seen == want


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("family,S,B", WB.LSTM_CALLS, ids=["%s-%dx%d" % (f or "plain", s, b) for f, s, b in WB.LSTM_CALLS])
def test_lstm_calls_stay_inside_their_buffers(family, S, B, train):
    """layer and stack calls of every family (csrc/lstm.hip), at both width orders and at 1 and 3 layers; train: p = 0.5"""
    seen = []
    for In, H in WB.LSTM_WIDTHS:
        for n_layers in WB.LSTM_LAYERS:
            WB.run_lstm_case(WB.lstm_case(family, S, B, In, H, n_layers, train), _check_guards(seen))
    assert seen == ["layer fwd", "layer bwd", "stack fwd", "stack bwd"] * (len(WB.LSTM_WIDTHS) * len(WB.LSTM_LAYERS))


@pytest.mark.parametrize("case", WB.DRNN_CASES, ids=[WB.drnn_case_id(c) for c in WB.DRNN_CASES])
def test_drnn_calls_stay_inside_their_buffers(case):
    """forward and backward of every entry-point family (csrc/dialogue_rnn.hip), on buffers of exactly ops.drnn_floats"""
    seen = []
    WB.run_drnn_case(case, _check_guards(seen))
    assert seen == ["fwd", "bwd"]


def test_drnn_cases_cover_every_family_attention_and_party_count():
    from gan_ffn_amd import ops
    cases = WB.DRNN_CASES
    family = lambda c: ops.drnn_family(c[1], c[7], c[5], c[6])
    for width in WB.DRNN_WIDTHS:
        assert {family(c) for c in cases if c[4] == width} == {"", "listener", "att", "party", "batch"}, width
    assert {(c[5], c[6]) for c in cases} == {(a, l) for a in ("general", "simple", "dot", "general2", "concat") for l in (False, True)}
    assert {c[7] for c in cases} == {1, 2, 16} and {(c[0], c[1]) for c in cases} == {(1, 1), (3, 1), (5, 3), (5, 33)}
    assert {c[2] for c in cases} == {1, 2} and {c[3] for c in cases} == {False, True}
    assert (3, 1) in {(c[0], c[1]) for c in cases if c[5] == "general2"}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", list(WB.HEADS))
def test_head_calls_stay_inside_their_buffers(name, train):
    seen = []
    WB.run_head_case(name, train, _check_guards(seen))
    assert seen == ["head fwd", "head bwd"]
