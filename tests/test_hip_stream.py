"""Streaming on the GPU: the single-query attention step over a K/V cache alone (ganffn_stream_attention, csrc/stream.hip), the
stack step (ganffn_encoder_stream_step) and GAN_FFN.stream() sessions, against fp64 — the attention step against a direct
restatement over the cache as include/ganffn.h lays it out, the stack and the session against the causal oracle
(tests/causal_oracle.py) run on each dialogue ALONE: a streamed row must be the matching row of the dialogue's full causal forward.
Bounds: the project's own — 2e-5 of the output's maximum for an attention forward (tests/test_hip_attention_causal.py), OUT_TOL =
1e-4 of scale for stack outputs and log_prob (tests/test_hip_key_len_engines.py)."""
import ctypes as C
import math

import pytest
import torch

from oracle import ganffn_oracle as O
from causal_oracle import causal_attention
import stream_oracle as SO
from test_hip_attention_causal import rel_err
from test_hip_dispatch_range import _encoder_inputs, _encoder_params
from test_hip_key_len_engines import OUT_TOL, _close

pytestmark = pytest.mark.gpu

ATTN_TOL = 2e-5
MAX_LEN = 110


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


# ================================================================================================================
# the kernel alone
# ================================================================================================================
CAP = 8
POS = [0, 1, 62, 63, 64, 65, 108, 109]        # per slot: both sides of the 64-key lane boundary, the last legal position
ROW_SLOTS = [5, 2, 7, 0, 3, 6, 1, 4]          # row i of the launch belongs to slot ROW_SLOTS[i]


def _attn_case(E, H):
    """cache [CAP][2][H][MAX_LEN][hd] per the header: random finite values below each slot's pos, NaN at and above; qkv [8, 3E]"""
    hd = E // H
    g = torch.Generator().manual_seed(E * 31 + H)
    cache = torch.randn(CAP, 2, H, MAX_LEN, hd, generator=g) * 1.5
    for s, t in enumerate(POS):
        cache[s, :, :, t:, :] = float("nan")
    qkv = torch.randn(CAP, 3 * E, generator=g) * 1.5
    return cache, qkv


def _attn_ref(cache, qkv, slots, pos, E, H):
    """fp64: row i attends with its q over the cached keys 0 .. t-1 of its slot and its own key"""
    hd = E // H
    o = torch.zeros(len(slots), E, dtype=torch.float64)
    for i, s in enumerate(slots):
        t = pos[s]
        q = qkv[i, :E].double().view(H, hd)
        k = torch.cat([cache[s, 0, :, :t].double(), qkv[i, E:2 * E].double().view(H, 1, hd)], 1)        # [H, t + 1, hd]
        v = torch.cat([cache[s, 1, :, :t].double(), qkv[i, 2 * E:].double().view(H, 1, hd)], 1)
        p = torch.softmax(torch.einsum("hd,hjd->hj", q, k) / math.sqrt(hd), dim=-1)
        o[i] = torch.einsum("hj,hjd->hd", p, v).reshape(E)
    return o


def _attn_launch(lib, cache_d, qkv_rows, slots, pos, E, H, cap=CAP):
    n = len(slots)
    o = torch.full((n, E), float("nan"), device="cuda")
    slot_d, pos_d = i32(slots), i32(pos)          # (named: both must be alive, at addresses of their own, when the call is made)
    lib.call("ganffn_stream_attention", ptr(qkv_rows), ptr(cache_d), ptr(slot_d), ptr(pos_d), ptr(o), n, cap, MAX_LEN, E, H,
             stream())
    torch.cuda.synchronize()
    return o


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("E,H", [(100, 10), (512, 8), (300, 10), (600, 10), (64, 4), (48, 4)],
                         ids=["hd10", "hd64", "hd30", "hd60", "hd16_runtime", "hd12_runtime"])
def test_stream_attention_kernel(E, H):
    from gan_ffn_amd import _lib as lib
    hd = E // H
    cache, qkv = _attn_case(E, H)
    cache_d, qkv_d = cache.cuda(), qkv.cuda()
    o = _attn_launch(lib, cache_d, qkv_d, ROW_SLOTS, POS, E, H)
    assert bool(torch.isfinite(o).all()), "a cache word at or above a position reached the output"
    err = rel_err(o, _attn_ref(cache, qkv, ROW_SLOTS, POS, E, H))
    print("stream attention (E %d, H %d): err / max %.3g (bound %g)" % (E, H, err, ATTN_TOL))
    assert err < ATTN_TOL
    # the cache: position pos of every row's slot now holds the row's K and V bits, every other word is unchanged
    want = cache.clone()
    for i, s in enumerate(ROW_SLOTS):
        want[s, 0, :, POS[s], :] = qkv[i, E:2 * E].view(H, hd)
        want[s, 1, :, POS[s], :] = qkv[i, 2 * E:].view(H, hd)
    assert torch.equal(bits(cache_d.cpu()), bits(want))
    # the bits of a row do not depend on the other rows: three of the slots, in another order, from the untouched cache
    sub = [6, 0, 3]
    cache2 = cache.cuda()
    o2 = _attn_launch(lib, cache2, qkv_d[sub].contiguous(), [ROW_SLOTS[i] for i in sub], POS, E, H)
    assert torch.equal(bits(o2), bits(o[sub]))
    # skipped rows: a full slot (pos = max_len), a negative position, slots outside [0, capacity); one live row beside them
    pos3 = list(POS)
    pos3[2], pos3[4] = MAX_LEN, -1
    slots3 = [2, CAP, 5, -1, 4]
    cache3 = cache.cuda()
    o3 = _attn_launch(lib, cache3, qkv_d[:5].contiguous(), slots3, pos3, E, H)
    assert bool((o3[[0, 1, 3, 4]] == 0).all())
    ref3 = _attn_ref(cache, qkv[2:3], [5], pos3, E, H)
    assert rel_err(o3[2:3], ref3) < ATTN_TOL
    want3 = cache.clone()
    want3[5, 0, :, POS[5], :] = qkv[2, E:2 * E].view(H, hd)
    want3[5, 1, :, POS[5], :] = qkv[2, 2 * E:].view(H, hd)
    assert torch.equal(bits(cache3.cpu()), bits(want3))


# ================================================================================================================
# the stack step
# ================================================================================================================
def _stack_case(E, H, F, L, n_dialogues):
    """seeded slab, a positional table of MAX_LEN rows and one input column per dialogue -> (slab, pe, [x_d [MAX_LEN, E]], P)"""
    slab, x, pe, _ = _encoder_inputs(MAX_LEN, n_dialogues, E, H, F, L)
    return slab, pe, [x[:, d].contiguous() for d in range(n_dialogues)], _encoder_params(slab, pe, E, F, L)


def _stack_oracle(xd, P, H, L, causal=True):
    with torch.no_grad():
        if causal:
            with causal_attention():
                return O.encoder_stack(xd.double().unsqueeze(1), P, H, None, n_layers=L)[:, 0]
        return O.encoder_stack(xd.double().unsqueeze(1), P, H, None, n_layers=L)[:, 0]


def _stream_stack(E, H, F, L, cap, dialogues, slab, pe, xs):
    """drive ganffn_encoder_stream_step through the schedule (the test advances and resets pos) -> {(dialogue, t): row}"""
    from gan_ffn_amd import ops
    cfg = ops.enc_cfg(MAX_LEN, cap, E, H, L, F=F, train=False)
    n_cache, n_ws = ops.stream_sizes(cfg, cap)
    f32 = dict(device="cuda", dtype=torch.float32)
    cache = torch.full((n_cache,), float("nan"), **f32)        # nothing at or above a position may be read
    ws = torch.zeros(n_ws, **f32)
    slab_d, pe_d = slab.cuda(), pe.cuda()
    xs_d = [x.cuda() for x in xs]
    pos = torch.zeros(cap, dtype=torch.int32, device="cuda")
    got = {}
    for ev in SO.schedule(dialogues):
        if ev[0] == "reset":
            pos[ev[1]] = 0
            continue
        _, rows, slots = ev
        n = len(rows)
        x = torch.stack([xs_d[d][t] for d, t in rows])
        out = torch.full((n, E), float("nan"), **f32)
        ops.encoder_stream_step_raw(cfg, n, i32(slots), pos, x, pe_d, slab_d, cache, out, ws)
        pos[slots] += 1
        for i, key in enumerate(rows):
            got[key] = out[i].cpu()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("E,H,F", [(100, 10, 2048), (512, 8, 2048), (64, 4, 128)])
def test_stream_stack_matches_causal_oracle_per_dialogue(E, H, F):
    L, cap = 2, 4
    slab, pe, xs, P = _stack_case(E, H, F, L, len(SO.STAGGERED))
    xs = [x[:n] for x, (_, _, n) in zip(xs, SO.STAGGERED)]
    want = [_stack_oracle(x, P, H, L) for x in xs]
    # the inputs tell the causal function from the bidirectional one at a row that is not a dialogue's last
    bi = _stack_oracle(xs[0], P, H, L, causal=False)
    gap = float((bi - want[0])[:-1].abs().max())
    assert gap > 10 * OUT_TOL * float(want[0].abs().max()), gap
    got = _stream_stack(E, H, F, L, cap, SO.STAGGERED, slab, pe, xs)
    assert {len(e[1]) for e in SO.schedule(SO.STAGGERED) if e[0] == "step"} >= {1, 3}        # thin T for the row-wise kernels
    for d, w in enumerate(want):
        have = torch.stack([got[(d, t)] for t in range(w.shape[0])])
        _close(have, w, OUT_TOL, "stream stack (%d, %d, %d) dialogue %d (%d rows)" % (E, H, F, d, w.shape[0]))


def test_stream_stack_one_slot_to_the_last_position():
    E, H, F, L = 64, 4, 128, 1
    slab, pe, xs, P = _stack_case(E, H, F, L, 1)
    want = _stack_oracle(xs[0], P, H, L)
    got = _stream_stack(E, H, F, L, 1, [(0, 0, MAX_LEN)], slab, pe, xs)
    have = torch.stack([got[(0, t)] for t in range(MAX_LEN)])
    _close(have, want, OUT_TOL, "stream stack, capacity 1, positions 0 .. 109")


# ================================================================================================================
# sessions
# ================================================================================================================
WIDTHS = {"acoustic": 100, "visual": 512, "text": 100}
KEYS = ("acoustic", "visual", "text")


def _inputs(dialogues, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: [torch.rand(n, WIDTHS[k], generator=g).cuda() for _, _, n in dialogues] for k in KEYS}


def _run_session(sess, dialogues, inp, rotate=True):
    """-> {(dialogue, t): log_prob row (a copy)}"""
    got = {}
    for ev in SO.schedule(dialogues, rotate=rotate):
        if ev[0] == "reset":
            sess.reset(ev[1])
            continue
        _, rows, slots = ev
        a, v, t = (torch.stack([inp[k][d][u] for d, u in rows]) for k in KEYS)
        lp = sess.step(a, v, t, slots)
        assert tuple(lp.shape) == (len(rows), 6)
        for i, key in enumerate(rows):
            got[key] = lp[i].clone()
    torch.cuda.synchronize()
    return got


def _same_bits(a, b, keys=None):
    for k in (keys if keys is not None else a):
        assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.fixture(scope="module")
def session_case():
    """real 8-layer generators, a causal classifier, the inputs of the SHORT schedule and the eager session's outputs"""
    from gan_ffn_amd import engine, model
    gens, _ = engine.build_networks(device="cuda", seed=23)
    net = model.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, causal=True).cuda()
    inp = _inputs(SO.SHORT, 41)
    sess = net.stream(capacity=3)
    base = _run_session(sess, SO.SHORT, inp)
    return dict(gens=gens, net=net, inp=inp, sess=sess, base=base)


def test_session_matches_gan_ffn_oracle_per_dialogue(session_case):
    c = session_case
    net = c["net"]
    og = {k: O.OracleNet("gen", {n: v.detach().cpu() for n, v in c["gens"][k].state_dict().items()}, c["gens"][k].nhead,
                         dtype=torch.float64) for k in KEYS}
    fc_w, fc_b = net.fc.weight.detach().cpu().double(), net.fc.bias.detach().cpu().double()
    for d, (_, _, n) in enumerate(SO.SHORT):
        a, v, t = (c["inp"][k][d].cpu().double().unsqueeze(1) for k in KEYS)
        with torch.no_grad():
            with causal_attention():
                want = O.gan_ffn_forward(a, v, t, og, fc_w, fc_b)[:, 0]
            bi = O.gan_ffn_forward(a, v, t, og, fc_w, fc_b)[:, 0]
        if d == 0:      # (discrimination: the bidirectional classifier is elsewhere at a row that is not the last)
            assert float((bi - want)[:-1].abs().max()) > 10 * OUT_TOL * float(want.abs().max())
        have = torch.stack([c["base"][(d, u)] for u in range(n)])
        _close(have, want, OUT_TOL, "session log_prob, dialogue %d (%d utterances)" % (d, n))
    assert c["sess"].positions.tolist() == [9, 1, 5]


def test_session_replay_after_reset_gives_the_same_bits(session_case):
    c = session_case
    c["sess"].reset()
    assert c["sess"].positions.tolist() == [0, 0, 0]
    _same_bits(_run_session(c["sess"], SO.SHORT, c["inp"]), c["base"])


def test_session_with_mask_padding_streams_the_same_values(session_case):
    from gan_ffn_amd import model
    c = session_case
    g = c["gens"]
    both = model.GAN_FFN(g["acoustic"], g["visual"], g["text"], n_classes=6, causal=True, mask_padding=True).cuda()
    both.load_state_dict(c["net"].state_dict())
    _same_bits(_run_session(both.stream(capacity=3), SO.SHORT, c["inp"]), c["base"])


def test_session_row_order_changes_no_bit(session_case):
    c = session_case
    sess = c["net"].stream(capacity=3)
    assert any(e[2] != sorted(e[2]) for e in SO.schedule(SO.SHORT) if e[0] == "step")       # the base run did permute rows
    _same_bits(_run_session(sess, SO.SHORT, c["inp"], rotate=False), c["base"])


def test_session_other_slots_change_no_bit(session_case):
    c = session_case
    other = _inputs(SO.SHORT, 97)
    mixed = {k: [c["inp"][k][0], other[k][1], other[k][2]] for k in KEYS}
    got = _run_session(c["net"].stream(capacity=3), SO.SHORT, mixed)
    _same_bits(got, c["base"], [(0, u) for u in range(SO.SHORT[0][2])])
    assert not torch.equal(got[(2, 0)], c["base"][(2, 0)])


def test_session_graph_gives_the_eager_bits(session_case):
    c = session_case
    sess = c["net"].stream(capacity=3, use_graph=True)
    _same_bits(_run_session(sess, SO.SHORT, c["inp"]), c["base"])
    sess.reset()
    _same_bits(_run_session(sess, SO.SHORT, c["inp"]), c["base"])       # every step a replay now
    assert sess.positions.tolist() == [9, 1, 5]


def test_session_full_slot_raises_and_launches_nothing(session_case):
    c = session_case
    sess = c["net"].stream(capacity=2, max_len=2)
    x = {k: torch.rand(2, WIDTHS[k], device="cuda") for k in KEYS}
    sess.step(x["acoustic"], x["visual"], x["text"])                     # slots = None: both slots
    sess.step(x["acoustic"][:1], x["visual"][:1], x["text"][:1], [1])
    assert sess.positions.tolist() == [1, 2]
    with pytest.raises(ValueError, match="full"):
        sess.step(x["acoustic"], x["visual"], x["text"], [0, 1])
    with pytest.raises(ValueError, match="distinct"):
        sess.step(x["acoustic"], x["visual"], x["text"], [0, 0])
    with pytest.raises(ValueError, match="capacity"):
        sess.step(x["acoustic"][:1], x["visual"][:1], x["text"][:1])
    assert sess.positions.tolist() == [1, 2] and sess._host_pos == [1, 2]
    sess.reset([1])
    sess.step(x["acoustic"], x["visual"], x["text"], torch.tensor([1, 0]))
    assert sess.positions.tolist() == [2, 1]
