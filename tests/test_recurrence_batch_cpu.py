"""Batches above 32 dialogues (every reference trainer's --batch-size: train_IEMOCAP_DialogueRNN.py:580, train_MELD.py:114) without a
GPU: the C ABI of the wide dialogue axis (ganffn_drnn_batch_*, ganffn_lstm_batch_*, ganffn_lstm_stack_batch_*: exported, bound,
sized — the existing sizes at B <= 32, growing with B as the layout comments say —, B = 0 and B = GANFFN_MAX_DIALOGUES + 1 reported as
errors, the existing entry points still refusing 33), the step runners' max_dialogues argument, and the project's CPU restatement
against the reference fixture tests/golden/recurrence_batch.npz (make_golden_batch.py: the reference's BiModel and MELDLSTMModel at 33
to 256 dialogues) at the tolerances tests/test_drnn_parties_cpu.py and tests/test_meld_step_cpu.py use for the same quantities."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import formula as F_
import make_golden_batch as MB
from test_dialogue_rnn_cpu import DIMS
from util import check_summary, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SYMBOLS = ["ganffn_drnn_batch_saved_floats", "ganffn_drnn_batch_workspace_floats", "ganffn_drnn_batch_fwd", "ganffn_drnn_batch_bwd",
                 "ganffn_lstm_batch_saved_floats", "ganffn_lstm_batch_workspace_floats", "ganffn_lstm_batch_layer_fwd",
                 "ganffn_lstm_batch_layer_bwd", "ganffn_lstm_stack_batch_saved_floats", "ganffn_lstm_stack_batch_workspace_floats",
                 "ganffn_lstm_stack_batch_fwd", "ganffn_lstm_stack_batch_bwd", "ganffn_drnn_skinny_batch"]
ATTS = [("general", 0), ("simple", 0), ("dot", 0), ("general2", 0), ("concat", 100)]


def header_max_dialogues():
    src = open(os.path.join(ROOT, "include", "ganffn.h")).read()
    return int(re.search(r"#define\s+GANFFN_MAX_DIALOGUES\s+(\d+)", src).group(1))


BMAX = header_max_dialogues()


def _drnn_cfg(att, S, B):
    from gan_ffn_amd import _lib
    return _lib.DrnnCfg(S, B, 100, 100 if att == "dot" else 500, 100, 0.1, 1)


def _drnn_sizes(fam, cfg, a, listener, P):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    return (getattr(lib, "ganffn_drnn_%s_saved_floats" % fam)(C.byref(cfg), C.byref(a), listener, P),
            getattr(lib, "ganffn_drnn_%s_workspace_floats" % fam)(C.byref(cfg), C.byref(a), listener, P))


def test_library_exports_the_batch_entry_points_with_bindings():
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    for s in BATCH_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    for s in ("fwd", "bwd", "saved_floats", "workspace_floats"):           # the _party_ argument lists
        assert _lib.SIGNATURES["ganffn_drnn_batch_" + s] == _lib.SIGNATURES["ganffn_drnn_party_" + s]
        assert _lib.SIGNATURES["ganffn_lstm_stack_batch_" + s] == _lib.SIGNATURES["ganffn_lstm_stack_" + s]
    for new, old in (("batch_saved_floats", "saved_floats"), ("batch_workspace_floats", "workspace_floats"),
                     ("batch_layer_fwd", "layer_fwd"), ("batch_layer_bwd", "layer_bwd")):
        assert _lib.SIGNATURES["ganffn_lstm_" + new] == _lib.SIGNATURES["ganffn_lstm_" + old]
    assert ops.MAX_DIALOGUES == BMAX == 256


@pytest.mark.parametrize("listener", [0, 1])
@pytest.mark.parametrize("att,da", ATTS)
def test_drnn_batch_sizes_equal_the_existing_ones_up_to_32_dialogues(att, da, listener):
    from gan_ffn_amd import _lib
    a = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], da)
    for B in (1, 30, 32):
        for P in (2, 9):
            cfg = _drnn_cfg(att, 94, B)
            want = _drnn_sizes("party", cfg, a, listener, P)
            assert want[0] > 0 and want[1] > 0
            assert _drnn_sizes("batch", cfg, a, listener, P) == want


@pytest.mark.parametrize("listener", [0, 1])
@pytest.mark.parametrize("att,da", ATTS)
def test_drnn_batch_sizes_grow_as_the_layouts_say(att, da, listener):
    """every region of the saved block and of the workspace but the transposed weights is linear in B at a fixed S (multiples of
    4 floats for B % 4 == 0: no padding): size(B) = size(32) + (B - 32) / 32 * (size(32) - weights)"""
    from gan_ffn_amd import _lib
    a = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], da)
    S, P = 33, 9
    H = 100 if att == "dot" else 500
    wt = (4 + (2 if listener else 0)) * H * 3 * H             # WT (+ WTl): the only regions that do not depend on B
    s32, w32 = _drnn_sizes("batch", _drnn_cfg(att, S, 32), a, listener, P)
    prev = (s32, w32)
    for B in (64, 100, 128, 256):
        s, w = _drnn_sizes("batch", _drnn_cfg(att, S, B), a, listener, P)
        assert s * 32 == s32 * B, (B, s, s32)
        assert (w - wt) * 32 == (w32 - wt) * B, (B, w, w32)
        assert s > prev[0] and w > prev[1]
        prev = (s, w)
    for B in (33, 255):                                          # odd counts: accepted, between their neighbours
        s, w = _drnn_sizes("batch", _drnn_cfg(att, S, B), a, listener, P)
        lo, hi = _drnn_sizes("batch", _drnn_cfg(att, S, B - 1), a, listener, P), _drnn_sizes("batch", _drnn_cfg(att, S, B + 1), a, listener, P)
        assert lo[0] < s < hi[0] and lo[1] < w < hi[1]


@pytest.mark.parametrize("B", [0, -3, BMAX + 1, 4096])
def test_dialogue_counts_outside_the_limit_are_reported_not_crashed(B):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    a = _lib.DrnnAtt(0, 0)
    cfg = _lib.DrnnCfg(7, B, 100, 500, 100, 0.1, 0)
    for listener in (0, 1):
        assert lib.ganffn_drnn_batch_saved_floats(C.byref(cfg), C.byref(a), listener, 2) < 0
        assert b"B=%d" % B in lib.ganffn_last_error()
        assert lib.ganffn_drnn_batch_workspace_floats(C.byref(cfg), C.byref(a), listener, 2) < 0
    with pytest.raises(_lib.GanffnError, match="B=%d" % B):
        _lib.call("ganffn_drnn_batch_fwd", C.byref(cfg), C.byref(a), 2, 2, *([None] * 11), C.c_uint64(0), None)
    with pytest.raises(_lib.GanffnError, match="B=%d" % B):
        _lib.call("ganffn_drnn_batch_bwd", C.byref(cfg), C.byref(a), 2, 2, *([None] * 15), C.c_uint64(0), None)
    lc = _lib.LstmCfg(7, B, 600, 300)
    assert lib.ganffn_lstm_batch_saved_floats(C.byref(lc)) < 0 and b"B=%d" % B in lib.ganffn_last_error()
    assert lib.ganffn_lstm_batch_workspace_floats(C.byref(lc)) < 0
    with pytest.raises(_lib.GanffnError, match="B=%d" % B):
        _lib.call("ganffn_lstm_batch_layer_fwd", C.byref(lc), *([None] * 9))
    with pytest.raises(_lib.GanffnError, match="B=%d" % B):
        _lib.call("ganffn_lstm_batch_layer_bwd", C.byref(lc), *([None] * 13))
    sc = _lib.LstmStackCfg(7, B, 600, 300, 4, 0.5, 1)
    assert lib.ganffn_lstm_stack_batch_saved_floats(C.byref(sc)) < 0 and b"B=%d" % B in lib.ganffn_last_error()
    assert lib.ganffn_lstm_stack_batch_workspace_floats(C.byref(sc)) < 0
    with pytest.raises(_lib.GanffnError, match="B=%d" % B):
        _lib.call("ganffn_lstm_stack_batch_fwd", C.byref(sc), *([None] * 9), C.c_uint64(0), None)
    with pytest.raises(_lib.GanffnError, match="B=%d" % B):
        _lib.call("ganffn_lstm_stack_batch_bwd", C.byref(sc), *([None] * 13), C.c_uint64(0), None)


def test_existing_entry_points_still_refuse_33_dialogues():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    a = _lib.DrnnAtt(0, 0)
    cfg = _lib.DrnnCfg(7, 33, 100, 500, 100, 0.1, 0)
    assert lib.ganffn_drnn_saved_floats(C.byref(cfg)) < 0 and b"B=33" in lib.ganffn_last_error()
    assert lib.ganffn_drnn_listener_workspace_floats(C.byref(cfg)) < 0
    assert lib.ganffn_drnn_att_saved_floats(C.byref(cfg), C.byref(a), 0) < 0
    assert lib.ganffn_drnn_party_saved_floats(C.byref(cfg), C.byref(a), 1, 9) < 0 and b"B=33" in lib.ganffn_last_error()
    with pytest.raises(_lib.GanffnError, match="B=33"):
        _lib.call("ganffn_drnn_party_fwd", C.byref(cfg), C.byref(a), 2, 2, *([None] * 11), C.c_uint64(0), None)
    assert lib.ganffn_lstm_saved_floats(C.byref(_lib.LstmCfg(7, 33, 600, 300))) < 0 and b"B=33" in lib.ganffn_last_error()
    assert lib.ganffn_lstm_stack_workspace_floats(C.byref(_lib.LstmStackCfg(7, 33, 600, 300, 4, 0.5, 1))) < 0
    with pytest.raises(_lib.GanffnError, match="M=33"):
        _lib.call("ganffn_drnn_skinny", 0, 1, None, None, None, 33, 16, 16, None)
    # ... and the batch ones take them
    assert lib.ganffn_drnn_batch_saved_floats(C.byref(cfg), C.byref(a), 0, 2) > 0


def test_lstm_batch_sizes_equal_the_existing_ones_and_grow_with_the_tokens():
    """saved: gates [2][T x 4H] | c [2][T x H] = 10 T H per layer (+ 2 x [T x 2H] per layer boundary in the stack): linear in B"""
    from gan_ffn_amd import _lib
    lib = _lib.load()
    S, In, H, L = 33, 600, 300, 4
    for B in (1, 7, 32):
        lc, sc = _lib.LstmCfg(S, B, In, H), _lib.LstmStackCfg(S, B, In, H, L, 0.5, 1)
        assert lib.ganffn_lstm_batch_saved_floats(C.byref(lc)) == lib.ganffn_lstm_saved_floats(C.byref(lc)) > 0
        assert lib.ganffn_lstm_batch_workspace_floats(C.byref(lc)) == lib.ganffn_lstm_workspace_floats(C.byref(lc)) > 0
        assert lib.ganffn_lstm_stack_batch_saved_floats(C.byref(sc)) == lib.ganffn_lstm_stack_saved_floats(C.byref(sc)) > 0
        assert lib.ganffn_lstm_stack_batch_workspace_floats(C.byref(sc)) == lib.ganffn_lstm_stack_workspace_floats(C.byref(sc)) > 0
    prev = 0
    for B in (33, 64, 100, 256):
        lc, sc = _lib.LstmCfg(S, B, In, H), _lib.LstmStackCfg(S, B, In, H, L, 0.5, 1)
        T = S * B
        assert lib.ganffn_lstm_batch_saved_floats(C.byref(lc)) == 10 * T * H
        assert lib.ganffn_lstm_stack_batch_saved_floats(C.byref(sc)) == L * 10 * T * H + (L - 1) * 2 * T * 2 * H
        w, ws = lib.ganffn_lstm_batch_workspace_floats(C.byref(lc)), lib.ganffn_lstm_stack_batch_workspace_floats(C.byref(sc))
        assert w >= 2 * T * 4 * H + 2 * B * 4 * H            # forward: xg [2][T x 4H] | G [2][B x 4H]
        assert ws >= w + 2 * T * 2 * H > prev                # + the two [T x 2H] gradient buffers of the backward
        prev = ws


def test_step_runners_take_a_dialogue_capacity():
    import inspect
    from gan_ffn_amd import artifacts as A, engine as E
    for cls in (E.DrnnEngine, E.MeldEngine):
        assert inspect.signature(cls.__init__).parameters["max_dialogues"].default == 32
    for n in (31, 0, BMAX + 1, 1000):
        with pytest.raises(ValueError, match="max_dialogues"):
            E._check_max_dialogues("MeldEngine", n)
    assert [E._check_max_dialogues("DrnnEngine", n) for n in (32, 64, BMAX)] == [32, 64, BMAX]
    assert "max_dialogues=max(32, batch_size)" in inspect.getsource(A.run_meld_training)


# ---- the reference fixture against the CPU restatement ------------------------------------------------------------------
def batch_model(name):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(1)
    m = DR.BiModel(**DIMS, **MB.DRNN_MODELS[name]).eval()
    sd = F_.formula_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def check_drnn_case(m, tag, dev, rtol=5e-5, grtol=5e-4, du_rtol=None):
    """BiModel `m` on the batch of DRNN_CASES[tag] against drnn/<tag>/* (tests/test_drnn_parties_cpu.check_big's bounds: every
    stored sample, no outliers; the l2 of every tensor)"""
    from gan_ffn_amd import model as M
    g = golden("recurrence_batch")
    U, qmask, umask, label = MB.drnn_inputs(tag)
    assert U.shape[:2] == MB.DRNN_CASES[tag][1:3] and qmask.shape[2] == MB.DRNN_CASES[tag][3]
    Ut = torch.from_numpy(U).to(dev).requires_grad_(True)
    um = torch.from_numpy(umask).to(dev)
    lp = m(Ut, torch.from_numpy(qmask).to(dev), um)[0]
    loss = M.MaskedNLLLoss(torch.tensor(MB.CLASS_W, device=dev))(lp.transpose(0, 1).contiguous().view(-1, lp.size(2)),
                                                                torch.from_numpy(label).to(dev).view(-1), um)
    loss.backward()
    pre = "drnn/%s/" % tag
    ref_loss = float(g[pre + "loss"])
    print("%s: loss %.7f (reference %.7f)" % (tag, float(loss.detach()), ref_loss))
    assert abs(float(loss.detach()) - ref_loss) <= 2e-5 * abs(ref_loss)
    r = {"log_prob": check_summary(g, pre + "log_prob", lp, rtol=rtol, atol=1e-6, what="log_prob", strict=True),
         "dU": check_summary(g, pre + "dU", Ut.grad, rtol=du_rtol or grtol, atol=1e-9, what="dU", strict=True)}
    assert abs(float(lp.detach().abs().max()) - float(g[pre + "log_prob/maxabs"])) <= rtol * float(g[pre + "log_prob/maxabs"])
    n, worst = 0, (0.0, "")
    for k, p in m.named_parameters():
        if p.grad is None:
            assert pre + "grad/" + k + "/maxabs" not in g.files, k
            continue
        d = check_summary(g, pre + "grad/" + k, p.grad, rtol=grtol, atol=1e-9, what="grad " + k, strict=True, l2_rtol=2e-3)
        worst = max(worst, (d, k))
        n += 1
    print("%s: log_prob %.2e dU %.2e worst gradient %.2e of scale (%s), %d gradient tensors" % (tag, r["log_prob"], r["dU"], *worst, n))
    assert n >= 24


@pytest.mark.parametrize("tag", list(MB.DRNN_CASES))
def test_torch_restatement_matches_reference_fixture(tag):
    check_drnn_case(batch_model(MB.DRNN_CASES[tag][0]), tag, "cpu")


def meld_dist(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def check_meld_case(g, tag, res, final, rt_lp=5e-5):
    """res: per step (loss, log_prob (S, B, C)); final: name -> parameter after MB.N_STEPS Adam steps.  The bounds of
    tests/test_meld_step_cpu.check_case: loss 2e-5 relative, log_prob 5e-5 of scale at every step, final parameters within
    2 lr N_STEPS (an Adam update is at most ~lr whatever the gradient)."""
    pre = "meld/%s/" % tag
    for i, (loss, lp) in enumerate(res):
        ref = float(g[pre + "loss"][i])
        assert abs(loss - ref) <= 2e-5 * abs(ref), (tag, i, loss, ref)
        check_summary(g, pre + "log_prob%d" % i, lp, rtol=rt_lp, atol=0.0, what="%s step %d log_prob" % (tag, i), strict=True)
    dp = 0.0
    for k, p in final.items():
        d = float(np.abs(MB.sample(p).astype(np.float64) - g[pre + "param/" + k]).max())
        assert d <= 2 * MB.LR * MB.N_STEPS, (tag, k, d)
        dp = max(dp, d)
    print("%s: worst final-parameter distance %.2e" % (tag, dp))
    return dp


@pytest.mark.parametrize("tag", list(MB.MELD_CASES))
def test_mirror_under_stock_loss_and_adam_reproduces_the_reference_fixture(tag):
    from gan_ffn_amd import model as M
    from test_meld_step_cpu import mirror
    g = golden("recurrence_batch")
    S, B, Cn = MB.MELD_CASES[tag]
    m = mirror(Cn)
    opt = torch.optim.Adam(m.parameters(), lr=MB.LR, weight_decay=MB.L2)
    U, umask, label = MB.meld_inputs(tag)
    Ut, um, lab = torch.from_numpy(U), torch.from_numpy(umask), torch.from_numpy(label)
    res = []
    for i in range(MB.N_STEPS):
        opt.zero_grad()
        lp = m(Ut, None, um)[0]
        loss = M.MaskedNLLLoss()(lp.transpose(0, 1).contiguous().view(-1, Cn), lab.view(-1), um)
        loss.backward()
        res.append((loss.item(), lp.detach().numpy().copy()))
        opt.step()
    check_meld_case(g, tag, res, {k: p.detach().numpy() for k, p in m.named_parameters()})


def test_fixture_inputs_are_ragged_as_documented():
    for S, B in ((20, 33), (33, 256), (12, 33)):
        L = MB.lengths(S, B)
        assert L[0] == S and L[2] == 1 and min(L) == 1 and max(L) == S and len(set(L)) > 5
    U, qmask, umask, label = MB.drnn_inputs("concat_listener_s33b100p9")
    assert qmask.shape == (33, 100, 9) and (qmask.sum(2) == umask.T).all() and qmask[:, :, 8].sum() == 0
    assert (U[1:, 2] == 0).all() and (label[umask == 0] == 0).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "recurrence_batch.npz")) < 1000000
