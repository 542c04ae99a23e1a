"""The streamed causal MELD classifier on the GPU: the LSTM step alone (ganffn_stream_lstm_step, csrc/lstm_stream.hip) and the
native extend against the fp64 restatement over the state as include/ganffn.h lays it out (tests/meld_stream_oracle.py);
MELDLSTMModel(causal=True).stream() sessions, step and extend, against the fp64 oracle run on each dialogue ALONE
(meld_causal_oracle.forward) and against the model's own full causal forward; the session after a MeldEngine train step.
Bounds, the project's own: 2e-5 of each output's maximum for one recurrence step built from the skinny products (E_TOL,
tests/test_hip_drnn_stream.py), OUT_TOL = 1e-4 of scale for log_prob (the module path, tests/test_hip_meld_causal.py)."""
import copy

import pytest
import torch

import meld_stream_oracle as MSO
import stream_oracle as SO
from test_hip_attention_causal import rel_err
from test_hip_key_len_engines import OUT_TOL, _close
from test_hip_stream import CAP, POS, ROW_SLOTS, bits, i32

pytestmark = pytest.mark.gpu

E_TOL = 2e-5
MAX_LEN = 110
F32 = dict(device="cuda", dtype=torch.float32)
SMALL, MELD = (16, 8, 8), (600, 300, 300)


# ================================================================================================================
# 1: the step kernel alone
# ================================================================================================================
# (In, H, L), capacity: the trained shape; small; L = 1 (no inter-layer product); 4H = 144, no multiple of the 16-column product
# tile; 40 rows (the skinny kernels' tiled path above 32 rows)
STEP_CASES = [((600, 300, 4), CAP), ((16, 8, 4), CAP), ((12, 20, 1), CAP), ((8, 36, 2), CAP), ((16, 8, 4), 40)]


def _layout(cap):
    """(positions per slot, the slot of every row): test_hip_stream's for 8 slots, repeated in blocks of 8 with the blocks' order
    reversed for more"""
    pos = [POS[s % CAP] for s in range(cap)]
    blocks = list(range(cap // CAP))[::-1]
    return pos, [CAP * blk + s for blk in blocks for s in ROW_SLOTS]


def _lstm(dims, seed=11):
    In, H, L = dims
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(In, H, num_layers=L, bidirectional=False)
    with torch.no_grad():                       # livelier recurrent weights than the default init (tests/test_hip_drnn_stream.py)
        for p in lstm.parameters():
            p.mul_(1.5)
    return lstm.eval()


_CASES = {}


def _step_case(dims, cap):
    """the LSTM (fp32 on the GPU, its fp64 copy for the oracle), the state the oracle builds from random utterances up to every
    slot's position (rounded to fp32, NaN where a step must not read), and one new row per slot; built once per case"""
    if (dims, cap) in _CASES:
        return _CASES[(dims, cap)]
    lstm = _lstm(dims)
    l64 = copy.deepcopy(lstm).double()
    pos, row_slots = _layout(cap)
    st = MSO.LstmState(l64, cap, MAX_LEN)
    g = torch.Generator().manual_seed(dims[1] * 7 + cap)
    for t in range(max(pos)):
        slots = [s for s in range(cap) if pos[s] > t]
        st.step(torch.rand(len(slots), dims[0], generator=g, dtype=torch.float64) - 0.3, slots, [t] * cap)
    st.Hs, st.Cs, st.E = st.Hs.float().double(), st.Cs.float().double(), st.E.float().double()
    st.poison(pos)
    x = torch.rand(cap, dims[0], generator=g) - 0.3
    _CASES[(dims, cap)] = (lstm.cuda(), st, x, pos, row_slots)
    return _CASES[(dims, cap)]


def _cfg(st):
    from gan_ffn_amd import ops
    return ops.lstm_stream_cfg(st.capacity, st.max_len, st.In, st.H, st.L)


def _launch_step(lstm_d, st, state_d, x_d, slots, pos, off=0, count=None):
    from gan_ffn_amd import ops
    cfg, n = _cfg(st), len(slots)
    _, n_ws = ops.lstm_stream_sizes(cfg, n)
    ws = torch.full((n_ws,), float("nan"), **F32)
    e_out = torch.full((n, st.H), float("nan"), **F32)
    slot_d, pos_d = i32(slots), i32(pos)
    count_d = i32(count) if count is not None else None
    ops.lstm_stream_step_raw(cfg, n, slot_d, pos_d, x_d, ops.lstm_stream_ptrs(lstm_d), state_d, e_out, ws, off, count_d)
    torch.cuda.synchronize()
    return e_out


def _views(st, flat):
    """(Hs, Cs, E) views of a flat state in the header's layout"""
    h, c, e, _ = st.offsets()
    return (flat[h:h + st.Hs.numel()].view(st.Hs.shape), flat[c:c + st.Cs.numel()].view(st.Cs.shape),
            flat[e:e + st.E.numel()].view(st.E.shape))


@pytest.mark.parametrize("dims,cap", STEP_CASES, ids=["%dx%dx%d_cap%d" % (d + (c,)) for d, c in STEP_CASES])
def test_step_kernel(dims, cap):
    lstm_d, st, x, pos, row_slots = _step_case(dims, cap)
    L = st.L
    before = st.flat()
    state_d, x_d = before.cuda(), x.cuda()
    e_out = _launch_step(lstm_d, st, state_d, x_d, row_slots, pos)              # row i belongs to slot row_slots[i]
    assert bool(torch.isfinite(e_out).all()), "a state word that must not be read reached the output"
    ref = st.clone()
    want_e = ref.step(x.double(), row_slots, pos)
    after = state_d.cpu()
    Hs, Cs, E = _views(st, after)
    e_new = torch.stack([E[s, pos[s]] for s in row_slots])
    errs = dict(e_out=rel_err(e_out, want_e), Hs=rel_err(Hs, ref.Hs), Cs=rel_err(Cs, ref.Cs),
                E=rel_err(e_new, torch.stack([ref.E[s, pos[s]] for s in row_slots])))
    print("lstm stream step %s cap %d: %s (bound %g)" % (dims, cap, ", ".join("%s %.3g" % kv for kv in errs.items()), E_TOL))
    assert bool(torch.isfinite(Hs).all()) and bool(torch.isfinite(Cs).all()) and bool(torch.isfinite(e_new).all())
    assert all(v < E_TOL for v in errs.values()), errs
    assert torch.equal(bits(e_new), bits(e_out.cpu()))          # e_out is the new E row
    assert torch.equal(bits(torch.stack([Hs[s, L - 1] for s in row_slots])), bits(e_out.cpu()))       # and the last layer's h
    # every other state word keeps its bits
    want = before.clone()
    Hw, Cw, Ew = _views(st, want)
    Hw.copy_(Hs)
    Cw.copy_(Cs)                                                # (every slot has a row)
    for s in row_slots:
        Ew[s, pos[s]] = E[s, pos[s]]
    assert torch.equal(bits(after), bits(want))
    # the bits of a row do not depend on the other rows: three of them, in another order, from an untouched copy of the state
    sub = [6, 0, 3]
    state2 = before.cuda()
    e2 = _launch_step(lstm_d, st, state2, x_d[sub].contiguous(), [row_slots[i] for i in sub], pos)
    assert torch.equal(bits(e2), bits(e_out[sub]))
    H2, C2, E2 = _views(st, state2.cpu())
    for i in sub:
        s = row_slots[i]
        assert torch.equal(bits(H2[s]), bits(Hs[s])) and torch.equal(bits(C2[s]), bits(Cs[s]))
        assert torch.equal(bits(E2[s, pos[s]]), bits(E[s, pos[s]]))
    want2 = before.clone()
    Hw, Cw, Ew = _views(st, want2)
    for i in sub:
        s = row_slots[i]
        Hw[s], Cw[s], Ew[s, pos[s]] = Hs[s], Cs[s], E[s, pos[s]]
    assert torch.equal(bits(state2.cpu()), bits(want2))         # and the slots without a row are untouched


def test_step_kernel_skipped_rows():
    """a slot at max_len, a negative position, slots -1 and capacity and a count-masked row beside one live row: zero rows, the
    state untouched but for the live row's words"""
    lstm_d, st, x, _, _ = _step_case((16, 8, 4), CAP)
    before = st.flat()
    pos = list(POS)
    pos[2], pos[4] = MAX_LEN, -1
    #        full  cap  live  -1  negative  masked by count
    slots = [2, CAP, 5, -1, 4, 0]
    count = [1, 1, 1, 1, 1, 0]
    state_d = before.cuda()
    e = _launch_step(lstm_d, st, state_d, x[:6].cuda().contiguous(), slots, pos, 0, count)
    assert bool((e[[0, 1, 3, 4, 5]] == 0).all())
    ref = st.clone()
    want_e = ref.step(x[2:3].double(), [5], pos)
    assert rel_err(e[2:3], want_e) < E_TOL
    after = state_d.cpu()
    Hs, Cs, E = _views(st, after)
    want = before.clone()
    Hw, Cw, Ew = _views(st, want)
    Hw[5], Cw[5], Ew[5, pos[5]] = Hs[5], Cs[5], E[5, pos[5]]
    assert torch.equal(bits(after), bits(want))
    assert rel_err(Hs[5], ref.Hs[5]) < E_TOL and rel_err(Cs[5], ref.Cs[5]) < E_TOL


# ================================================================================================================
# 2: the extend kernel
# ================================================================================================================
COUNTS = [4, 1, 0, 3, 2, 4, 1, 1]         # per row; row i belongs to slot ROW_SLOTS[i]


@pytest.mark.parametrize("dims", [(16, 8, 4), (600, 300, 4)], ids=["16x8x4", "600x300x4"])
def test_extend_kernel_is_m_steps_bit_for_bit(dims):
    """m = 4; the row at position 108 (slot 6, count 4) loses its last two steps"""
    from gan_ffn_amd import ops
    lstm_d, st, _, pos, row_slots = _step_case(dims, CAP)
    m, n = 4, CAP
    assert pos[row_slots[5]] == 108 and COUNTS[5] == 4
    before = st.flat()
    x = (torch.rand(m, n, dims[0], generator=torch.Generator().manual_seed(3)) - 0.3).cuda()
    cfg = _cfg(st)
    _, n_ws = ops.lstm_stream_sizes(cfg, n)
    ws = torch.full((n_ws,), float("nan"), **F32)
    slot_d, pos_d, count_d = i32(row_slots), i32(pos), i32(COUNTS)
    state_a = before.cuda()
    e_a = torch.full((m, n, st.H), float("nan"), **F32)
    ops.lstm_stream_extend_raw(cfg, n, m, slot_d, count_d, pos_d, x, ops.lstm_stream_ptrs(lstm_d), state_a, e_a, ws)
    torch.cuda.synchronize()
    state_b = before.cuda()
    e_b = torch.stack([_launch_step(lstm_d, st, state_b, x[j].contiguous(), row_slots, pos, j, COUNTS) for j in range(m)])
    assert torch.equal(bits(state_a), bits(state_b)) and torch.equal(bits(e_a), bits(e_b))
    live = [[j < COUNTS[i] and pos[row_slots[i]] + j < MAX_LEN for i in range(n)] for j in range(m)]
    assert sum(map(sum, live)) == 14
    for j in range(m):
        for i in range(n):
            assert bool(torch.isfinite(e_a[j, i]).all()) and (live[j][i] or bool((e_a[j, i] == 0).all())), (j, i)
            assert not live[j][i] or bool((e_a[j, i] != 0).any()), (j, i)


# ================================================================================================================
# 3: sessions
# ================================================================================================================
LENS = [33, 1, 20, 7, 12]
JOIN = [(0, 0, 33), (1, 1, 1), (2, 3, 20), (3, 5, 7), (4, 8, 12)]          # (slot, the step it joins at, utterances)


def _model(dims, seed=2, packed=False):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    m = DR.MELDLSTMModel(*dims, n_classes=7, dropout=0.5, packed=packed, causal=True)
    with torch.no_grad():                               # transform is initialised small: scores away from tanh's linear range
        m.matchatt.transform.weight.mul_(20.0 if dims == SMALL else 4.0)
        if dims == SMALL:                               # livelier than the default init, so that a late row depends visibly on
            for p in m.lstm.parameters():               # the early utterances (the discrimination check of the session test)
                p.mul_(4.0)
            m.smax_fc.weight.mul_(3.0)
    return m.cuda().eval()


def _inputs(lens, D_m, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, D_m, generator=g) - 0.5).cuda() for n in lens]


def _run_session(sess, dialogues, inp, rotate=True):
    got = {}
    for ev in SO.schedule(dialogues, rotate=rotate):
        if ev[0] == "reset":
            sess.reset(ev[1])
            continue
        _, rows, slots = ev
        lp = sess.step(torch.stack([inp[d][u] for d, u in rows]), slots)
        assert tuple(lp.shape) == (len(rows), 7)
        for i, key in enumerate(rows):
            got[key] = lp[i].clone()
    torch.cuda.synchronize()
    return got


def _same_bits(a, b, keys=None):
    for k in (keys if keys is not None else a):
        assert torch.equal(bits(a[k]), bits(b[k])), k


def _oracle_log_prob(model, inp):
    m64 = copy.deepcopy(model).cpu().double().eval()
    return [MSO.alone(m64, x.cpu()) for x in inp]


def _module_log_prob(model, inp):
    """the model's own full causal forward on the padded batch -> [log_prob (n, 7)]"""
    lens = [x.shape[0] for x in inp]
    S, B = max(lens), len(lens)
    text, umask = torch.zeros(S, B, inp[0].shape[1], device="cuda"), torch.zeros(B, S, device="cuda")
    for d, n in enumerate(lens):
        text[:n, d] = inp[d]
        umask[d, :n] = 1.0
    with torch.no_grad():
        lp = model(text, None, umask)[0]
    return [lp[:n, d] for d, n in enumerate(lens)]


def _session_case(dims):
    model = _model(dims)
    inp = _inputs(LENS, dims[0], 41)
    sess = model.stream(capacity=5)
    base = _run_session(sess, JOIN, inp)
    return dict(model=model, inp=inp, sess=sess, base=base, dims=dims)


@pytest.fixture(scope="module")
def session_case():
    return _session_case(SMALL)


@pytest.mark.parametrize("dims", [SMALL, MELD], ids=["16x8x8", "600x300x300"])
def test_session_matches_the_oracle_and_the_full_forward_per_dialogue(dims, session_case):
    c = session_case if dims == SMALL else _session_case(dims)
    assert {len(e[1]) for e in SO.schedule(JOIN) if e[0] == "step"} >= {1, 2, 3, 4}        # positions differ within a call
    want = _oracle_log_prob(c["model"], c["inp"])
    full = _module_log_prob(c["model"], c["inp"])
    if dims == SMALL:           # (discrimination: the bound sees the history — other early utterances move the late rows far past it)
        moved = c["inp"][0].clone()
        moved[:5] += 0.3
        far = _oracle_log_prob(c["model"], [moved])[0]
        assert float((far[10:] - want[0][10:]).abs().max()) > 10 * OUT_TOL * float(want[0].abs().max())
    for d, n in enumerate(LENS):
        have = torch.stack([c["base"][(d, u)] for u in range(n)])
        _close(have, want[d], OUT_TOL, "%s session log_prob vs oracle, dialogue %d (%d utterances)" % (dims, d, n))
        _close(have, full[d], OUT_TOL, "%s session log_prob vs full causal forward, dialogue %d" % (dims, d))
    assert c["sess"].positions.tolist() == LENS and c["sess"]._host_pos == LENS


def test_session_replay_after_reset_gives_the_same_bits(session_case):
    c = session_case
    c["sess"].reset()
    assert c["sess"].positions.tolist() == [0] * 5
    _same_bits(_run_session(c["sess"], JOIN, c["inp"]), c["base"])


def test_session_row_order_changes_no_bit(session_case):
    c = session_case
    assert any(e[2] != sorted(e[2]) for e in SO.schedule(JOIN) if e[0] == "step")       # the base run did permute rows
    _same_bits(_run_session(c["model"].stream(capacity=5), JOIN, c["inp"], rotate=False), c["base"])


def test_session_other_slots_change_no_bit(session_case):
    c = session_case
    other = _inputs(LENS, SMALL[0], 97)
    got = _run_session(c["model"].stream(capacity=5), JOIN, [c["inp"][0]] + other[1:])
    _same_bits(got, c["base"], [(0, u) for u in range(LENS[0])])
    assert not torch.equal(got[(2, 0)], c["base"][(2, 0)])


def test_session_of_a_packed_twin_streams_the_same_bits(session_case):
    c = session_case
    twin = _model(SMALL, packed=True)
    twin.load_state_dict(c["model"].state_dict())
    assert twin.packed and not c["model"].packed
    _same_bits(_run_session(twin.stream(capacity=5), JOIN, c["inp"]), c["base"])


def test_session_one_slot_to_the_last_position_then_full(session_case):
    model = session_case["model"]
    sess = model.stream(capacity=2)
    x = _inputs([MAX_LEN], SMALL[0], 5)[0]
    for t in range(MAX_LEN):
        lp = sess.step(x[t:t + 1], [1])
    last = lp.clone()
    assert sess.positions.tolist() == [0, MAX_LEN] and bool(torch.isfinite(last).all())
    full = _module_log_prob(model, [x])[0]
    _close(last[0], full[-1], OUT_TOL, "session log_prob at position 109 vs full causal forward")
    state = bits(sess.state).clone()
    with pytest.raises(ValueError, match="full"):                # the 111th step: nothing launched
        sess.step(x[:1], [1])
    torch.cuda.synchronize()
    assert sess.positions.tolist() == [0, MAX_LEN] and sess._host_pos == [0, MAX_LEN] and torch.equal(bits(sess.state), state)
    assert torch.equal(lp, last)
    with pytest.raises(ValueError, match="text must be"):
        sess.step(x[:1, :12], [0])
    assert sess._host_pos == [0, MAX_LEN]


# ================================================================================================================
# 4: extend
# ================================================================================================================
ELENS, PRE = [9, 1, 6], [7, 1, 4]


def _padded(inp, pre, m, fill=0.0):
    x = torch.full((m, len(pre), inp[0].shape[1]), fill, device="cuda")
    for i, c in enumerate(pre):
        x[:c, i] = inp[i][:c]
    return x


def _run_extend(sess, inp, fill=0.0):
    """extend (7, 3) with lengths [7, 1, 4], then steps to the dialogues' ends -> {(dialogue, t): log_prob row}"""
    lp = sess.extend(_padded(inp, PRE, 7, fill), PRE)
    assert tuple(lp.shape) == (7, 3, 7)
    got = {(d, t): lp[t, d].clone() for d in range(3) for t in range(PRE[d])}
    for k in range(max(n - p for n, p in zip(ELENS, PRE))):
        rows = [d for d in range(3) if PRE[d] + k < ELENS[d]]
        out = sess.step(torch.stack([inp[d][PRE[d] + k] for d in rows]), rows)
        for i, d in enumerate(rows):
            got[(d, PRE[d] + k)] = out[i].clone()
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def extend_case(session_case):
    model = session_case["model"]
    inp = _inputs(ELENS, SMALL[0], 43)
    sess = model.stream(capacity=3)
    base = _run_extend(sess, inp)
    return dict(model=model, inp=inp, sess=sess, base=base)


def test_extend_then_steps_matches_steps_and_the_oracle(extend_case):
    c = extend_case
    assert c["sess"].positions.tolist() == ELENS and c["sess"]._host_pos == ELENS
    steps = _run_session(c["model"].stream(capacity=3), [(d, 0, n) for d, n in enumerate(ELENS)], c["inp"])
    want = _oracle_log_prob(c["model"], c["inp"])
    for d, n in enumerate(ELENS):
        have = torch.stack([c["base"][(d, u)] for u in range(n)])
        _close(have, torch.stack([steps[(d, u)] for u in range(n)]), OUT_TOL, "extend + steps vs steps, dialogue %d" % d)
        _close(have, want[d], OUT_TOL, "extend + steps vs oracle, dialogue %d" % d)


def test_extend_rows_past_a_length_change_no_bit(extend_case):
    c = extend_case
    sess, ref = c["model"].stream(capacity=3), c["model"].stream(capacity=3)
    ref.extend(_padded(c["inp"], PRE, 7), PRE)
    lp = sess.extend(_padded(c["inp"], PRE, 7, fill=3.25), PRE).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lp).all())
    for d in range(3):
        for t in range(PRE[d]):
            assert torch.equal(bits(lp[t, d]), bits(c["base"][(d, t)])), (d, t)
    H, L = sess.D_e, sess.L
    E, E0 = sess.e_hist.view(3, MAX_LEN, H), ref.e_hist.view(3, MAX_LEN, H)
    for d in range(3):                                       # the state below the new positions
        assert torch.equal(bits(E[d, :PRE[d]]), bits(E0[d, :PRE[d]]))
    n_hc = 2 * 3 * L * H                                     # Hs and Cs: every slot was stepped
    assert torch.equal(bits(sess.state[:n_hc]), bits(ref.state[:n_hc]))
    _same_bits(_run_extend(c["model"].stream(capacity=3), c["inp"], fill=-1.5), c["base"])


def test_extend_refusals_move_no_position_and_launch_nothing(extend_case):
    c = extend_case
    sess = c["model"].stream(capacity=3, max_len=9)
    x = _padded(c["inp"], PRE, 7)
    sess.extend(x, PRE)

    def state():
        torch.cuda.synchronize()
        return sess.positions.tolist(), list(sess._host_pos), int(bits(sess.state).to(torch.int64).sum())

    before = state()
    assert before[0] == PRE
    short = x[:3]
    for lengths, match in (([3, 1, 1], "slot 0 holds 7 of max_len=9 utterances: 2 more fit, not 3"),
                           ([1, 1], "lengths"),
                           ([1, 0, 1], r"outside \[1, m=3\]")):
        with pytest.raises(ValueError, match=match):
            sess.extend(short, lengths)
        assert state() == before, match
    lp = sess.extend(short, [2, 2, 1])                       # still usable
    assert sess.positions.tolist() == [9, 3, 5] and bool(torch.isfinite(lp[0]).all())


# ================================================================================================================
# 5: after training
# ================================================================================================================
def test_session_after_a_train_step_reads_the_new_weights_and_leaves_the_engine_alone():
    """one MeldEngine train step on the model, then reset() + extend of a dialogue: the rows are the model's full forward with
    the weights as they are NOW (the engine moved the parameters into its slab; the session reads them at call time).  The
    engine's next step has the bits of a twin engine's that never saw a session."""
    from gan_ffn_amd import engine as E, ops
    from test_hip_meld_causal import SEED, batch
    S, B = 9, 3
    b = batch(S, B, SMALL[0], [9, 4, 1])
    x = _inputs([12], SMALL[0], 7)[0]

    def run(with_session):
        from gan_ffn_amd import dialogue_rnn as DR
        torch.manual_seed(23)
        net = DR.MELDLSTMModel(*SMALL, n_classes=7, dropout=0.6, causal=True).cuda().train()
        ops.manual_seed(SEED)
        eng = E.MeldEngine(net, lr=1e-2, weight_decay=1e-4)
        rows = {}
        if with_session:
            sess = net.stream(capacity=2)
            rows["stale"] = sess.extend(x.unsqueeze(1), [12], [1]).clone()
        loss1, _ = eng.step(b, train=True)
        if with_session:
            sess.reset()
            rows["fresh"] = sess.extend(x.unsqueeze(1), [12], [1]).clone()
            assert sess.positions.tolist() == [0, 12]
            was = net.training
            net.eval()
            rows["full"] = _module_log_prob(net, [x])[0]
            net.train(was)
        loss2, lp2 = eng.step(b, train=True)
        torch.cuda.synchronize()
        return eng.slab.clone(), loss1.clone(), loss2.clone(), lp2.clone(), rows

    plain = run(False)
    seen = run(True)
    rows = seen[4]
    _close(rows["fresh"][:, 0], rows["full"], OUT_TOL, "session after a train step vs the model's full forward")
    moved = float((rows["stale"] - rows["fresh"]).abs().max())
    print("one train step at lr 1e-2 moved the streamed rows by %.3g" % moved)
    assert moved > 10 * OUT_TOL * float(rows["full"].abs().max())          # (the step did move what the session computes)
    for a, c in zip(plain[:4], seen[:4]):
        assert torch.equal(bits(a), bits(c))
