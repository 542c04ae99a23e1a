"""No encoder, head or LSTM call writes past the size its size function reports.

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
packed lengths (1, 5, 3) and a ragged vector with dialogues of length 1."""
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


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", list(WB.HEADS))
def test_head_calls_stay_inside_their_buffers(name, train):
    seen = []
    WB.run_head_case(name, train, _check_guards(seen))
    assert seen == ["head fwd", "head bwd"]
