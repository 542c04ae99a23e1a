"""The streamed DialogueRNN head on the GPU: the recurrence step alone (ganffn_drnn_stream_step, csrc/drnn_stream.hip) and the
single-query general2 attention alone (ganffn_general2_stream_attention) against the fp64 restatement over the state as
include/ganffn.h lays it out (tests/drnn_stream_oracle.py); GAN_FFN_DialogueRNN(causal=True).stream() sessions, step and extend,
against the fp64 oracle run on each dialogue ALONE (the causal generators through causal_attention, then
drnn_causal_oracle.uni_head) and against the net's own full causal forward.
Bounds, the project's own: 2e-5 of each output's maximum for the recurrence forward (tests/test_hip_drnn_kernel.py, e_tol), 5e-6
for the causal general2 forward (tests/test_hip_drnn_causal.py), OUT_TOL = 1e-4 of scale for log_prob (the module path)."""
import copy

import pytest
import torch

from oracle import ganffn_oracle as O
from causal_oracle import causal_attention
import drnn_causal_oracle as DCO
import drnn_stream_oracle as DSO
import stream_oracle as SO
from test_hip_attention_causal import rel_err
from test_hip_drnn_causal import _net
from test_hip_key_len_engines import OUT_TOL, _close
from test_hip_stream import CAP, KEYS, POS, ROW_SLOTS, WIDTHS, bits, i32

pytestmark = pytest.mark.gpu

E_TOL = 2e-5
G2_TOL = 5e-6
MAX_LEN = 110
F32 = dict(device="cuda", dtype=torch.float32)


# ================================================================================================================
# 1: the step kernel alone
# ================================================================================================================
STEP_CASES = [((100, 500, 100), a, 2, False) for a in ("general", "simple", "general2", "concat")] + \
             [((100, 100, 100), "dot", 2, False),
              ((100, 500, 100), "general", 2, True), ((100, 500, 100), "concat", 2, True),
              ((12, 20, 8), "general", 1, False), ((12, 20, 8), "general", 16, False),
              ((8, 16, 36), "general", 9, True),
              ((100, 512, 132), "general", 2, False)]


def _cell(dims, att, listener, seed=11):
    from gan_ffn_amd import dialogue_rnn as DR
    Dm, H, He = dims
    torch.manual_seed(seed)
    cell = DR.DialogueRNNCell(Dm, H, H, He, listener_state=listener, context_attention=att, D_a=100, dropout=0.1)
    with torch.no_grad():                       # livelier recurrent weights than the default init (tests/test_hip_drnn_kernel.py)
        for p in cell.parameters():
            p.mul_(1.5)
        if att == "general2":                   # transform is initialised at std 0.01: scores away from tanh's linear range
            cell.attention.transform.weight.mul_(20.0)
    return cell.eval()


def _step_case(dims, att, parties, listener):
    """the cell (fp32 on the GPU, its fp64 copy for the oracle), the state the oracle builds from random utterances and speakers up
    to every slot's position (rounded to fp32, NaN at and above), and one new row per slot"""
    cell = _cell(dims, att, listener)
    c64 = copy.deepcopy(cell).double()
    st = DSO.HeadState(c64, CAP, MAX_LEN, parties)
    g = torch.Generator().manual_seed(dims[1] * 7 + parties)
    for t in range(max(POS)):
        slots = [s for s in range(CAP) if POS[s] > t]
        U = torch.rand(len(slots), dims[0], generator=g, dtype=torch.float64) - 0.3
        spk = torch.randint(0, parties, (len(slots),), generator=g).tolist()
        st.step(U, spk, slots, [t] * CAP)
    st.G, st.Q, st.E = st.G.float().double(), st.Q.float().double(), st.E.float().double()
    st.poison(POS)
    U = (torch.rand(CAP, dims[0], generator=g) - 0.3)
    spk = torch.randint(0, parties, (CAP,), generator=g).tolist()
    return cell.cuda(), st, U, spk


def _launch_step(cell_d, st, state_d, U_d, spk, slots, pos, off=0, count=None):
    from gan_ffn_amd import ops
    c = st.cell
    att = DSO.att_type(c)
    cfg = ops.drnn_stream_cfg(st.capacity, st.max_len, st.parties, c.D_m, c.D_g, c.D_e, c.listener_state, att,
                              c.attention.transform.weight.shape[0] if att == "concat" else 0)
    n = len(slots)
    _, n_ws = ops.drnn_stream_sizes(cfg, n)
    ws = torch.full((n_ws,), float("nan"), **F32)
    e_out = torch.full((n, c.D_e), float("nan"), **F32)
    slot_d, pos_d, spk_d = i32(slots), i32(pos), i32(spk)
    count_d = i32(count) if count is not None else None
    ops.drnn_stream_step_raw(cfg, n, slot_d, pos_d, spk_d, U_d, ops.drnn_stream_cell_ptrs(cell_d), state_d, e_out, ws, off, count_d)
    torch.cuda.synchronize()
    return e_out


def _views(st, flat):
    """(G, Q, E) views of a flat state in the header's layout"""
    g, q, e, _ = st.offsets()
    return (flat[g:g + st.G.numel()].view(st.G.shape), flat[q:q + st.Q.numel()].view(st.Q.shape),
            flat[e:e + st.E.numel()].view(st.E.shape))


@pytest.mark.parametrize("dims,att,parties,listener", STEP_CASES,
                         ids=["%dx%dx%d_%s_p%d%s" % (d + (a, p, "_listener" if l else "")) for d, a, p, l in STEP_CASES])
def test_step_kernel(dims, att, parties, listener):
    cell_d, st, U, spk = _step_case(dims, att, parties, listener)
    before = st.flat()
    state_d, U_d = before.cuda(), U.cuda()
    rows_U, rows_spk = U_d, spk                                # row i belongs to slot ROW_SLOTS[i]
    e_out = _launch_step(cell_d, st, state_d, rows_U, rows_spk, ROW_SLOTS, POS)
    assert bool(torch.isfinite(e_out).all()), "a state word at or above a position reached the output"
    ref = st.clone()
    want_e = ref.step(U.double(), spk, ROW_SLOTS, POS)
    after = state_d.cpu()
    G, Q, E = _views(st, after)
    errs = dict(e_out=rel_err(e_out, want_e))
    g_new = torch.stack([G[s, POS[s]] for s in ROW_SLOTS])
    e_new = torch.stack([E[s, POS[s]] for s in ROW_SLOTS])
    errs["G"] = rel_err(g_new, torch.stack([ref.G[s, POS[s]] for s in ROW_SLOTS]))
    errs["E"] = rel_err(e_new, torch.stack([ref.E[s, POS[s]] for s in ROW_SLOTS]))
    errs["Q"] = rel_err(Q, ref.Q)
    print("drnn stream step %s %s p%d%s: %s (bound %g)" % (dims, att, parties, " listener" if listener else "",
                                                          ", ".join("%s %.3g" % kv for kv in errs.items()), E_TOL))
    assert bool(torch.isfinite(g_new).all()) and bool(torch.isfinite(e_new).all()) and bool(torch.isfinite(Q).all())
    assert all(v < E_TOL for v in errs.values()), errs
    assert torch.equal(bits(e_new), bits(e_out.cpu()))          # e_out is the new E row
    # every other state word keeps its bits
    want = before.clone()
    Gw, Qw, Ew = _views(st, want)
    for s in ROW_SLOTS:
        Gw[s, POS[s]], Ew[s, POS[s]] = G[s, POS[s]], E[s, POS[s]]
    Qw.copy_(Q)
    assert torch.equal(bits(after), bits(want))
    # the bits of a row do not depend on the other rows: three of them, in another order, from an untouched copy of the state
    sub = [6, 0, 3]
    state2 = before.cuda()
    e2 = _launch_step(cell_d, st, state2, U_d[sub].contiguous(), [spk[i] for i in sub], [ROW_SLOTS[i] for i in sub], POS)
    assert torch.equal(bits(e2), bits(e_out[sub]))
    G2, Q2, E2 = _views(st, state2.cpu())
    for i in sub:
        s = ROW_SLOTS[i]
        assert torch.equal(bits(G2[s, POS[s]]), bits(G[s, POS[s]])) and torch.equal(bits(Q2[s]), bits(Q[s]))


def test_step_kernel_skipped_rows():
    """a slot at max_len, a negative position, slots -1 and capacity, a speaker equal to parties and a count-masked row beside one
    live row: zero rows, the state untouched but for the live row's words"""
    dims, parties = (12, 20, 8), 2
    cell_d, st, U, spk = _step_case(dims, "general", parties, True)
    before = st.flat()
    pos = list(POS)
    pos[2], pos[4] = MAX_LEN, -1
    #        full  cap  live  -1  negative  spk = parties  masked by count
    slots = [2, CAP, 5, -1, 4, 3, 0]
    spks = [0, 1, spk[2], 0, 1, parties, 1]
    count = [1, 1, 1, 1, 1, 1, 0]
    state_d = before.cuda()
    e = _launch_step(cell_d, st, state_d, U[:7].cuda().contiguous(), spks, slots, pos, 0, count)
    assert bool((e[[0, 1, 3, 4, 5, 6]] == 0).all())
    ref = st.clone()
    want_e = ref.step(U[2:3].double(), [spk[2]], [5], pos)
    assert rel_err(e[2:3], want_e) < E_TOL
    after = state_d.cpu()
    G, Q, E = _views(st, after)
    want = before.clone()
    Gw, Qw, Ew = _views(st, want)
    Gw[5, pos[5]], Ew[5, pos[5]], Qw[5] = G[5, pos[5]], E[5, pos[5]], Q[5]
    assert torch.equal(bits(after), bits(want))
    assert rel_err(Q[5], ref.Q[5]) < E_TOL and rel_err(G[5, pos[5]], ref.G[5, pos[5]]) < E_TOL


# ================================================================================================================
# 2: the second attention of new rows alone
# ================================================================================================================
COUNTS = [4, 1, 0, 3, 2, 4, 1, 1]         # per row; row i belongs to slot ROW_SLOTS[i]


def _g2_launch(x, e_hist, slots, count, pos, m, D, with_alpha=True):
    from gan_ffn_amd import ops
    n = len(slots)
    att = torch.full((m, n, D), float("nan"), **F32)
    alpha = torch.full((m, n, MAX_LEN), float("nan"), **F32) if with_alpha else None
    slot_d, pos_d = i32(slots), i32(pos)
    count_d = i32(count) if count is not None else None
    ops.general2_stream_attention_raw(x, e_hist, slot_d, count_d, pos_d, att, alpha, n, m, CAP, MAX_LEN, D)
    torch.cuda.synchronize()
    return att, alpha


@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("D", [100, 8, 132])
def test_general2_stream_attention(D, m):
    g = torch.Generator().manual_seed(D * 10 + m)
    count = None if m == 1 else COUNTS
    cnt = [1] * CAP if m == 1 else COUNTS
    E = torch.rand(CAP, MAX_LEN, D, generator=g) - 0.5
    for i, s in enumerate(ROW_SLOTS):                       # the state already holds the new rows; NaN above them
        E[s, min(MAX_LEN, POS[s] + cnt[i]):] = float("nan")
    x = (torch.rand(m, CAP, D, generator=g) - 0.5) * (8.0 if D == 8 else 1.5)
    att, alpha = _g2_launch(x.cuda(), E.cuda(), ROW_SLOTS, count, POS, m, D)
    assert bool(torch.isfinite(att).all()) and bool(torch.isfinite(alpha).all()), "a word above pos + j reached the output"
    want_att, want_alpha = torch.zeros(m, CAP, D, dtype=torch.float64), torch.zeros(m, CAP, MAX_LEN, dtype=torch.float64)
    live = 0
    for i, s in enumerate(ROW_SLOTS):
        for j in range(m):
            nk = POS[s] + j + 1
            if j < cnt[i] and nk <= MAX_LEN:
                want_att[j, i], want_alpha[j, i, :nk] = DSO.general2_row(x[j, i].double(), E[s, :nk].double())
                live += 1
            else:                                            # skipped: zero rows
                assert bool((att[j, i] == 0).all()) and bool((alpha[j, i] == 0).all())
    assert live == (8 if m == 1 else 14)                     # (m = 4: the row at position 108 loses its last two of four)
    errs = (rel_err(att, want_att), rel_err(alpha, want_alpha))
    print("general2 stream attention D %d m %d: att %.3g alpha %.3g (bound %g)" % (D, m, errs[0], errs[1], G2_TOL))
    assert errs[0] < G2_TOL and errs[1] < G2_TOL
    assert bool((alpha.cpu()[want_alpha == 0] == 0).all())   # exact zeros past the row's last memory step
    att2, _ = _g2_launch(x.cuda(), E.cuda(), ROW_SLOTS, count, POS, m, D, with_alpha=False)
    assert torch.equal(bits(att2), bits(att))
    # slots outside the capacity and a negative position: zero rows
    pos3 = list(POS)
    pos3[4] = -1
    att3, alpha3 = _g2_launch(x[:, :4].contiguous().cuda(), E.cuda(), [CAP, 5, -1, 4], None if m == 1 else [1, 1, 1, 1], pos3, m, D)
    assert bool((att3[:, [0, 2, 3]] == 0).all()) and bool((alpha3[:, [0, 2, 3]] == 0).all())
    assert bool(torch.isfinite(att3).all())


# ================================================================================================================
# 3: sessions
# ================================================================================================================
LENS = [33, 1, 20, 7, 12]
JOIN = [(0, 0, 33), (1, 1, 1), (2, 3, 20), (3, 5, 7), (4, 8, 12)]          # (slot, the step it joins at, utterances)


def _inputs(lens, parties, seed):
    g = torch.Generator().manual_seed(seed)
    inp = {k: [torch.rand(n, WIDTHS[k], generator=g).cuda() for n in lens] for k in KEYS}
    inp["spk"] = [torch.randint(0, parties, (n,), generator=g).tolist() for n in lens]
    return inp


def _run_session(sess, dialogues, inp, rotate=True):
    got = {}
    for ev in SO.schedule(dialogues, rotate=rotate):
        if ev[0] == "reset":
            sess.reset(ev[1])
            continue
        _, rows, slots = ev
        a, v, t = (torch.stack([inp[k][d][u] for d, u in rows]) for k in KEYS)
        lp = sess.step(a, v, t, [inp["spk"][d][u] for d, u in rows], slots)
        assert tuple(lp.shape) == (len(rows), 6)
        for i, key in enumerate(rows):
            got[key] = lp[i].clone()
    torch.cuda.synchronize()
    return got


def _same_bits(a, b, keys=None):
    for k in (keys if keys is not None else a):
        assert torch.equal(bits(a[k]), bits(b[k])), k


_FUSION = {}


def _oracle_fusion(net, inp, lens, seed):
    """fp64 causal generators on each dialogue alone -> [fusion (n, 100)]; the three nets of this file share their generators
    (same seed, built first), so the stacks are run once per input set"""
    key = (seed, tuple(lens))
    slabs = [getattr(net, k + "_generator").slab.detach().cpu() for k in KEYS]
    if key in _FUSION and all(torch.equal(a, b) for a, b in zip(_FUSION[key][0], slabs)):
        return _FUSION[key][1]
    og = {k: O.OracleNet("gen", {n: v.detach().cpu() for n, v in getattr(net, k + "_generator").state_dict().items()},
                         getattr(net, k + "_generator").nhead, dtype=torch.float64) for k in KEYS}
    out = []
    for d in range(len(lens)):
        with torch.no_grad(), causal_attention():
            out.append(sum(og[k](inp[k][d].cpu().double().unsqueeze(1)) for k in KEYS)[:, 0].detach())
    _FUSION[key] = (slabs, out)
    return out


def _oracle_log_prob(net, inp, lens, parties, seed):
    um = copy.deepcopy(net.bi_model).cpu().double().eval()
    out = []
    for d, fus in enumerate(_oracle_fusion(net, inp, lens, seed)):
        res = DCO.uni_head(um, fus.unsqueeze(1), DSO.one_hot(inp["spk"][d], parties), torch.ones(1, lens[d], dtype=torch.float64))
        out.append(res["log_prob"][:, 0])
    return out


def _module_log_prob(net, inp, lens, parties):
    """the net's own full causal forward on the padded batch -> [log_prob (n, 6)]"""
    S, B = max(lens), len(lens)
    x = {k: torch.zeros(S, B, WIDTHS[k], device="cuda") for k in KEYS}
    qmask, umask = torch.zeros(S, B, parties, device="cuda"), torch.zeros(B, S, device="cuda")
    for d, n in enumerate(lens):
        for k in KEYS:
            x[k][:n, d] = inp[k][d]
        qmask[:n, d] = torch.nn.functional.one_hot(torch.tensor(inp["spk"][d]), parties).float().cuda()
        umask[d, :n] = 1.0
    with torch.no_grad():
        lp = net(x["acoustic"], x["visual"], x["text"], qmask, umask)[0]
    return [lp[:n, d] for d, n in enumerate(lens)]


SESSION_CASES = {"general": (False, "general", 2), "concat_listener": (True, "concat", 2), "parties9": (False, "general", 9)}


def _session_case(name):
    listener, att, parties = SESSION_CASES[name]
    net = _net(listener, att).eval()
    inp = _inputs(LENS, parties, 41)
    sess = net.stream(capacity=5, parties=parties)
    base = _run_session(sess, JOIN, inp)
    return dict(net=net, inp=inp, sess=sess, base=base, parties=parties)


@pytest.fixture(scope="module")
def session_case():
    return _session_case("general")


@pytest.mark.parametrize("name", list(SESSION_CASES))
def test_session_matches_the_oracle_and_the_full_forward_per_dialogue(name, session_case):
    c = session_case if name == "general" else _session_case(name)
    assert {len(e[1]) for e in SO.schedule(JOIN) if e[0] == "step"} >= {1, 2, 3, 4}        # positions differ within a call
    want = _oracle_log_prob(c["net"], c["inp"], LENS, c["parties"], 41)
    full = _module_log_prob(c["net"], c["inp"], LENS, c["parties"])
    if name == "general":       # (discrimination: the bound sees the history — other early utterances move the late rows far past it)
        fus = _oracle_fusion(c["net"], c["inp"], LENS, 41)[0].clone()
        fus[:5] += 0.3
        um = copy.deepcopy(c["net"].bi_model).cpu().double().eval()
        moved = DCO.uni_head(um, fus.unsqueeze(1), DSO.one_hot(c["inp"]["spk"][0], 2), torch.ones(1, LENS[0], dtype=torch.float64))
        assert float((moved["log_prob"][10:, 0] - want[0][10:]).abs().max()) > 10 * OUT_TOL * float(want[0].abs().max())
    for d, n in enumerate(LENS):
        have = torch.stack([c["base"][(d, u)] for u in range(n)])
        _close(have, want[d], OUT_TOL, "%s session log_prob vs oracle, dialogue %d (%d utterances)" % (name, d, n))
        _close(have, full[d], OUT_TOL, "%s session log_prob vs full causal forward, dialogue %d" % (name, d))
    assert c["sess"].positions.tolist() == LENS and c["sess"]._host_pos == LENS


def test_session_replay_after_reset_gives_the_same_bits(session_case):
    c = session_case
    c["sess"].reset()
    assert c["sess"].positions.tolist() == [0] * 5
    _same_bits(_run_session(c["sess"], JOIN, c["inp"]), c["base"])


def test_session_row_order_changes_no_bit(session_case):
    c = session_case
    assert any(e[2] != sorted(e[2]) for e in SO.schedule(JOIN) if e[0] == "step")       # the base run did permute rows
    _same_bits(_run_session(c["net"].stream(capacity=5), JOIN, c["inp"], rotate=False), c["base"])


def test_session_other_slots_change_no_bit(session_case):
    c = session_case
    other = _inputs(LENS, 2, 97)
    mixed = {k: [c["inp"][k][0]] + other[k][1:] for k in KEYS + ("spk",)}
    got = _run_session(c["net"].stream(capacity=5), JOIN, mixed)
    _same_bits(got, c["base"], [(0, u) for u in range(LENS[0])])
    assert not torch.equal(got[(2, 0)], c["base"][(2, 0)])


def test_session_with_mask_padding_streams_the_same_bits(session_case):
    c = session_case
    both = _net(mask_padding=True).eval()
    both.load_state_dict(c["net"].state_dict())
    _same_bits(_run_session(both.stream(capacity=5), JOIN, c["inp"]), c["base"])


def test_session_one_slot_to_the_last_position_then_full(session_case):
    net = session_case["net"]
    sess = net.stream(capacity=2)
    g = torch.Generator().manual_seed(5)
    x = {k: torch.rand(MAX_LEN, WIDTHS[k], generator=g).cuda() for k in KEYS}
    spk = torch.randint(0, 2, (MAX_LEN,), generator=g).tolist()
    for t in range(MAX_LEN):
        lp = sess.step(x["acoustic"][t:t + 1], x["visual"][t:t + 1], x["text"][t:t + 1], [spk[t]], [1])
    last = lp.clone()
    assert sess.positions.tolist() == [0, MAX_LEN] and bool(torch.isfinite(last).all())
    full = _module_log_prob(net, {**{k: [x[k]] for k in KEYS}, "spk": [spk]}, [MAX_LEN], 2)[0]
    _close(last[0], full[-1], OUT_TOL, "session log_prob at position 109 vs full causal forward")
    state = bits(sess.state).clone()
    for bad, match in (((x["acoustic"][:1], x["visual"][:1], x["text"][:1], [0], [1]), "full"),
                       ((x["acoustic"][:1], x["visual"][:1], x["text"][:1], [2], [0]), "speaker 2"),
                       ((x["acoustic"][:1], x["visual"][:1], x["text"][:1], [-1], [0]), "speaker -1"),
                       ((x["acoustic"][:1], x["visual"][:1], x["text"][:1], [0, 1], [0]), "speakers")):
        with pytest.raises(ValueError, match=match):         # the 111th step, a speaker out of range: nothing launched
            sess.step(*bad[:3], bad[3], bad[4])
        torch.cuda.synchronize()
        assert sess.positions.tolist() == [0, MAX_LEN] and sess._host_pos == [0, MAX_LEN] and torch.equal(bits(sess.state), state)
    assert torch.equal(lp, last)


# ================================================================================================================
# 4: extend
# ================================================================================================================
ELENS, PRE = [9, 1, 6], [7, 1, 4]


def _padded(inp, pre, m, fill=0.0, spk_fill=0):
    xs = []
    for k in KEYS:
        x = torch.full((m, len(pre), WIDTHS[k]), fill, device="cuda")
        for i, c in enumerate(pre):
            x[:c, i] = inp[k][i][:c]
        xs.append(x)
    spk = [[inp["spk"][i][j] if j < pre[i] else spk_fill for i in range(len(pre))] for j in range(m)]
    return xs, spk


def _run_extend(sess, inp, fill=0.0, spk_fill=0):
    """extend (7, 3) with lengths [7, 1, 4], then steps to the dialogues' ends -> {(dialogue, t): log_prob row}"""
    xs, spk = _padded(inp, PRE, 7, fill, spk_fill)
    lp = sess.extend(*xs, spk, PRE)
    assert tuple(lp.shape) == (7, 3, 6)
    got = {(d, t): lp[t, d].clone() for d in range(3) for t in range(PRE[d])}
    for k in range(max(n - p for n, p in zip(ELENS, PRE))):
        rows = [d for d in range(3) if PRE[d] + k < ELENS[d]]
        out = sess.step(*(torch.stack([inp[key][d][PRE[d] + k] for d in rows]) for key in KEYS),
                        [inp["spk"][d][PRE[d] + k] for d in rows], rows)
        for i, d in enumerate(rows):
            got[(d, PRE[d] + k)] = out[i].clone()
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def extend_case(session_case):
    net = session_case["net"]
    inp = _inputs(ELENS, 2, 43)
    sess = net.stream(capacity=3)
    base = _run_extend(sess, inp)
    return dict(net=net, inp=inp, sess=sess, base=base)


def test_extend_then_steps_matches_steps_and_the_oracle(extend_case):
    c = extend_case
    assert c["sess"].positions.tolist() == ELENS and c["sess"]._host_pos == ELENS
    steps = _run_session(c["net"].stream(capacity=3), [(d, 0, n) for d, n in enumerate(ELENS)], c["inp"])
    want = _oracle_log_prob(c["net"], c["inp"], ELENS, 2, 43)
    for d, n in enumerate(ELENS):
        have = torch.stack([c["base"][(d, u)] for u in range(n)])
        _close(have, torch.stack([steps[(d, u)] for u in range(n)]), OUT_TOL, "extend + steps vs steps, dialogue %d" % d)
        _close(have, want[d], OUT_TOL, "extend + steps vs oracle, dialogue %d" % d)


def test_extend_rows_past_a_length_change_no_bit(extend_case):
    c = extend_case
    sess = c["net"].stream(capacity=3)
    ref = c["net"].stream(capacity=3)
    xs, spk = _padded(c["inp"], PRE, 7)
    ref.extend(*xs, spk, PRE)
    xs2, spk2 = _padded(c["inp"], PRE, 7, fill=3.25, spk_fill=1)
    lp = sess.extend(*xs2, spk2, PRE).clone()
    torch.cuda.synchronize()
    for d in range(3):
        for t in range(PRE[d]):
            assert torch.equal(bits(lp[t, d]), bits(c["base"][(d, t)])), (d, t)
    H, He = sess.cell.D_g, sess.cell.D_e
    n_g = 3 * MAX_LEN * H
    G, G0 = sess.state[:n_g].view(3, MAX_LEN, H), ref.state[:n_g].view(3, MAX_LEN, H)
    E, E0 = sess.e_hist.view(3, MAX_LEN, He), ref.e_hist.view(3, MAX_LEN, He)
    Q, Q0 = sess.state[n_g:n_g + 3 * 2 * H], ref.state[n_g:n_g + 3 * 2 * H]
    for d in range(3):                                       # the state below the new positions
        assert torch.equal(bits(G[d, :PRE[d]]), bits(G0[d, :PRE[d]])) and torch.equal(bits(E[d, :PRE[d]]), bits(E0[d, :PRE[d]]))
    assert torch.equal(bits(Q), bits(Q0))
    _same_bits(_run_extend(c["net"].stream(capacity=3), c["inp"], fill=-1.5, spk_fill=1), c["base"])


def test_extend_split_over_dialogue_groups_keeps_the_bits(extend_case, monkeypatch):
    from gan_ffn_amd import ops
    c = extend_case
    monkeypatch.setattr(ops, "STREAM_EXTEND_MAX_ROWS", 14)          # m = 7: two dialogues per generator call, n = 3 in two groups
    sess = c["net"].stream(capacity=3)
    got = _run_extend(sess, c["inp"])
    assert len(sess._ext_bufs[(7, 3)].groups) == 2 and len(c["sess"]._ext_bufs[(7, 3)].groups) == 1
    _same_bits(got, c["base"])


def test_extend_refusals_move_no_position_and_launch_nothing(extend_case):
    c = extend_case
    sess = c["net"].stream(capacity=3, max_len=9)
    xs, spk = _padded(c["inp"], PRE, 7)
    sess.extend(*xs, spk, PRE)

    def state():
        torch.cuda.synchronize()
        return (sess.positions.tolist(), list(sess._host_pos), int(bits(sess.state).to(torch.int64).sum()),
                [int(bits(ch).to(torch.int64).sum()) for ch in sess.caches])

    before = state()
    assert before[0] == PRE
    short = [x[:3] for x in xs]
    for args, sp, lengths, match in ((short, spk[:3], [3, 1, 1], "slot 0 holds 7 of max_len=9 utterances: 2 more fit, not 3"),
                                     (short, [[0, 0, 2]] * 3, [1, 1, 1], "speaker 2"),
                                     (short, spk[:2], [1, 1, 1], "speakers"),
                                     (short, spk[:3], [1, 1], "lengths"),
                                     (short, spk[:3], [1, 0, 1], r"outside \[1, m=3\]")):
        with pytest.raises(ValueError, match=match):
            sess.extend(*args, sp, lengths)
        assert state() == before, match
    lp = sess.extend(*short, [[0, 0, 1], [0, 0, 5], [5, 5, 5]], [2, 2, 1])      # speakers past a length are ignored; still usable
    assert sess.positions.tolist() == [9, 3, 5] and bool(torch.isfinite(lp[0]).all())
