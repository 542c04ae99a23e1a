"""Stream prefill on the GPU: the chunk attention kernel over a K/V cache alone (ganffn_stream_attention_chunk, csrc/stream.hip),
the stack call (ganffn_encoder_stream_extend) and StreamSession.extend, against fp64 — the kernel against a direct restatement
over the cache as include/ganffn.h lays it out, the stack and the session against the causal oracle (tests/causal_oracle.py) run
on each dialogue ALONE: however a dialogue is cut into chunks and steps, a row must be the matching row of its full causal forward.
Bounds: the project's own, as tests/test_hip_stream.py has them — ATTN_TOL = 2e-5 of the output's maximum for an attention
forward, OUT_TOL = 1e-4 of scale for stack outputs and log_prob."""
import ctypes as C
import math

import pytest
import torch

from oracle import ganffn_oracle as O
from causal_oracle import causal_attention
import stream_oracle as SO
import stream_extend_oracle as XO
from test_hip_attention_causal import rel_err
from test_hip_key_len_engines import OUT_TOL, _close
from test_hip_stream import ATTN_TOL, MAX_LEN, _attn_ref, _stack_case, _stack_oracle, bits, i32, ptr, stream

pytestmark = pytest.mark.gpu

NAN = float("nan")

# ================================================================================================================
# the kernel alone
# ================================================================================================================
CAP = 8
M = 110
# (pos, count) per chunk: both sides of the 64-key lane boundary in the cached part and in the new part, the last legal
# position, a full slot
CHUNKS = [(0, 1), (0, 110), (63, 2), (1, 64), (64, 46), (109, 1), (30, 17), (0, 65)]
CHUNK_SLOTS = [5, 2, 7, 0, 3, 6, 1, 4]          # column i of the launch belongs to slot CHUNK_SLOTS[i]
POS = [0] * CAP
for (_t, _c), _s in zip(CHUNKS, CHUNK_SLOTS):
    POS[_s] = _t


def _chunk_case(E, H):
    """cache [CAP][2][H][MAX_LEN][hd] per the header: random finite values below each slot's pos, NaN at and above;
    qkv [M, 8, 3E] time-major: random in the rows j < count of each chunk, NaN in the others"""
    hd = E // H
    g = torch.Generator().manual_seed(E * 37 + H)
    cache = torch.randn(CAP, 2, H, MAX_LEN, hd, generator=g) * 1.5
    for s, t in enumerate(POS):
        cache[s, :, :, t:, :] = NAN
    qkv = torch.randn(M, len(CHUNKS), 3 * E, generator=g) * 1.5
    for i, (_, c) in enumerate(CHUNKS):
        qkv[c:, i] = NAN
    return cache, qkv


def _chunk_ref(cache, qkv, slots, counts, pos, E, H):
    """fp64: row j of chunk i attends with its q over the cached keys 0 .. t-1 of its slot and the chunk's keys 0 .. j
    -> {i: [count, E]}"""
    hd = E // H
    out = {}
    for i, (s, c) in enumerate(zip(slots, counts)):
        t = pos[s]
        k = torch.cat([cache[s, 0, :, :t].double(), qkv[:c, i, E:2 * E].double().view(c, H, hd).transpose(0, 1)], 1)     # [H, t + c, hd]
        v = torch.cat([cache[s, 1, :, :t].double(), qkv[:c, i, 2 * E:].double().view(c, H, hd).transpose(0, 1)], 1)
        q = qkv[:c, i, :E].double().view(c, H, hd)
        sc = torch.einsum("jhd,hkd->hjk", q, k) / math.sqrt(hd)
        key = torch.arange(t + c).view(1, 1, -1)
        sc = sc.masked_fill(key > (t + torch.arange(c)).view(1, -1, 1), float("-inf"))
        out[i] = torch.einsum("hjk,hkd->jhd", torch.softmax(sc, dim=-1), v).reshape(c, E)
    return out


def _chunk_launch(lib, cache_d, qkv_d, slots, counts, pos, E, H, m=M):
    n = len(slots)
    o = torch.full((m, n, E), NAN, device="cuda")
    slot_d, count_d, pos_d = i32(slots), i32(counts), i32(pos)       # (named: all must be alive when the call is made)
    lib.call("ganffn_stream_attention_chunk", ptr(qkv_d), ptr(cache_d), ptr(slot_d), ptr(count_d), ptr(pos_d), ptr(o), n, m, CAP,
             MAX_LEN, E, H, stream())
    torch.cuda.synchronize()
    return o


def _cache_after(cache, qkv, slots, counts, pos, E, H):
    """the cache a launch must leave: the chunks' K / V bits at t .. t+c-1, every other word unchanged"""
    hd = E // H
    want = cache.clone()
    for i, (s, c) in enumerate(zip(slots, counts)):
        t = pos[s]
        want[s, 0, :, t:t + c, :] = qkv[:c, i, E:2 * E].view(c, H, hd).transpose(0, 1)
        want[s, 1, :, t:t + c, :] = qkv[:c, i, 2 * E:].view(c, H, hd).transpose(0, 1)
    return want


def _check_chunks(o, ref, counts, label):
    worst = 0.0
    for i, c in enumerate(counts):
        if c > 0:
            assert bool(torch.isfinite(o[:c, i]).all()), "%s: a cache word at or above a position, or a pad row, reached chunk %d" % (label, i)
            worst = max(worst, rel_err(o[:c, i], ref[i]))
        assert bool((o[max(c, 0):, i] == 0).all()), "%s: rows j >= count of chunk %d are not exact zeros" % (label, i)
    print("%s: err / max %.3g (bound %g)" % (label, worst, ATTN_TOL))
    assert worst < ATTN_TOL


WIDTHS_EH = [(100, 10), (512, 8), (300, 10), (600, 10), (64, 4), (48, 4)]
WIDTH_IDS = ["hd10", "hd64", "hd30", "hd60", "hd16_runtime", "hd12_runtime"]


@pytest.mark.parametrize("E,H", WIDTHS_EH, ids=WIDTH_IDS)
def test_stream_attention_chunk_kernel(E, H):
    from gan_ffn_amd import _lib as lib
    cache, qkv = _chunk_case(E, H)
    counts = [c for _, c in CHUNKS]
    cache_d, qkv_d = cache.cuda(), qkv.cuda()
    o = _chunk_launch(lib, cache_d, qkv_d, CHUNK_SLOTS, counts, POS, E, H)
    _check_chunks(o.cpu(), _chunk_ref(cache, qkv, CHUNK_SLOTS, counts, POS, E, H), counts, "chunk attention (E %d, H %d)" % (E, H))
    # the cache: positions t .. t+c-1 of every chunk's slot hold the rows' K and V bits, every other word is unchanged
    want = _cache_after(cache, qkv, CHUNK_SLOTS, counts, POS, E, H)
    assert torch.equal(bits(cache_d.cpu()), bits(want))
    # the bits of a chunk depend neither on the other chunks nor on its column: three of them, in another order, fresh cache
    # (fewer chunks also split each chunk's queries over more workgroups)
    sub = [6, 1, 3]
    cache2 = cache.cuda()
    o2 = _chunk_launch(lib, cache2, qkv_d[:, sub].contiguous(), [CHUNK_SLOTS[i] for i in sub], [counts[i] for i in sub], POS, E, H)
    for k, i in enumerate(sub):
        assert torch.equal(bits(o2[:counts[i], k]), bits(o[:counts[i], i])), i
    # a single-query step at pos + count reads the cache the chunk kernel wrote
    nxt = [i for i, (t, c) in enumerate(CHUNKS) if t + c < MAX_LEN]
    assert len(nxt) == 5
    pos1 = list(POS)
    for (t, c), s in zip(CHUNKS, CHUNK_SLOTS):
        pos1[s] = t + c
    g = torch.Generator().manual_seed(E + 7)
    q1 = torch.randn(len(nxt), 3 * E, generator=g) * 1.5
    slots1 = [CHUNK_SLOTS[i] for i in nxt]
    o1 = torch.full((len(nxt), E), NAN, device="cuda")
    slot_d, pos_d, q1_d = i32(slots1), i32(pos1), q1.cuda()
    lib.call("ganffn_stream_attention", ptr(q1_d), ptr(cache_d), ptr(slot_d), ptr(pos_d), ptr(o1), len(nxt), CAP, MAX_LEN, E, H, stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1).all())
    assert rel_err(o1, _attn_ref(want, q1, slots1, pos1, E, H)) < ATTN_TOL


@pytest.mark.parametrize("E,H", WIDTHS_EH, ids=WIDTH_IDS)
def test_stream_attention_chunk_skip_rule(E, H):
    """slot -1, slot = capacity, a negative position, pos + count = max_len + 1, count = m + 1 and count = 0 beside one live
    chunk: zeros for the skipped ones, the cache untouched but for the live chunk, the live one right"""
    from gan_ffn_amd import _lib as lib
    cache, qkv = _chunk_case(E, H)
    pos = list(POS)              # slot 3 is at 64, slot 1 at 30
    pos[2] = -1
    slots = [-1, CAP, 2, 3, 4, 6, 1]
    counts = [3, 3, 3, 47, M + 1, 0, 17]
    live = 6
    g = torch.Generator().manual_seed(E + 11)
    q = torch.full((M, len(slots), 3 * E), NAN)
    q[:17, live] = torch.randn(17, 3 * E, generator=g) * 1.5
    cache_d = cache.cuda()
    o = _chunk_launch(lib, cache_d, q.cuda(), slots, counts, pos, E, H).cpu()
    for i in range(len(slots)):
        if i != live:
            assert bool((o[:, i] == 0).all()), i
    ref = _chunk_ref(cache, q[:, live:live + 1], [1], [17], pos, E, H)
    _check_chunks(o[:, live:live + 1], ref, [17], "live chunk beside skipped ones (E %d, H %d)" % (E, H))
    want = _cache_after(cache, q[:, live:live + 1], [1], [17], pos, E, H)
    assert torch.equal(bits(cache_d.cpu()), bits(want))


# ================================================================================================================
# the stack
# ================================================================================================================
def _drive_stack(E, H, F, L, cap, events, slab, pe, xs, pad=0.0):
    """drive ganffn_encoder_stream_extend / _step through the events on a NaN-filled cache (the test advances and resets pos)
    -> ({(dialogue, t): row}, cache)"""
    from gan_ffn_amd import ops
    cfg = ops.enc_cfg(MAX_LEN, cap, E, H, L, F=F, train=False)
    n_cache, n_ws = ops.stream_sizes(cfg, cap)
    rows_max = max([max(c for _, _, c in e[1]) * len(e[1]) for e in events if e[0] == "extend"] + [1])
    f32 = dict(device="cuda", dtype=torch.float32)
    cache = torch.full((n_cache,), NAN, **f32)                  # nothing at or above a position may be read
    ws = torch.zeros(n_ws, **f32)
    ws_x = torch.zeros(ops.stream_extend_sizes(cfg, rows_max), **f32)
    slab_d, pe_d = slab.cuda(), pe.cuda()
    xs_d = [x.cuda() for x in xs]
    pos = torch.zeros(cap, dtype=torch.int32, device="cuda")
    got = {}
    for ev in events:
        if ev[0] == "reset":
            pos[ev[1]] = 0
        elif ev[0] == "step":
            _, rows, slots = ev
            x = torch.stack([xs_d[d][t] for d, t in rows])
            out = torch.full((len(rows), E), NAN, **f32)
            ops.encoder_stream_step_raw(cfg, len(rows), i32(slots), pos, x, pe_d, slab_d, cache, out, ws)
            pos[slots] += 1
            for i, key in enumerate(rows):
                got[key] = out[i].cpu()
        else:
            _, chunks, slots = ev
            x, counts = XO.pad_chunks(xs_d, chunks, fill=pad)
            m, n = x.shape[0], x.shape[1]
            out = torch.full((m, n, E), NAN, **f32)
            ops.encoder_stream_extend_raw(cfg, n, m, i32(slots), i32(counts), pos, x, pe_d, slab_d, cache, out, ws_x)
            pos[slots] += torch.tensor(counts, dtype=torch.int32, device="cuda")
            for i, (d, first, c) in enumerate(chunks):
                for j in range(c):
                    got[(d, first + j)] = out[j, i].cpu()
    torch.cuda.synchronize()
    return got, cache


@pytest.mark.parametrize("E,H,F", [(100, 10, 2048), (512, 8, 2048), (64, 4, 128)])
def test_stack_chunks_and_steps_match_causal_oracle_per_dialogue(E, H, F):
    L, cap = 2, 4
    slab, pe, xs, P = _stack_case(E, H, F, L, len(SO.STAGGERED))
    xs = [x[:n] for x, (_, _, n) in zip(xs, SO.STAGGERED)]
    want = [_stack_oracle(x, P, H, L) for x in xs]
    events = XO.mixed_schedule(SO.STAGGERED, XO.STAGGERED_SPLITS, XO.STAGGERED_STARTS)
    assert XO.STAGGERED_SPLITS[0] == [30, 1, 1, 1, 33] and [e for e in events if e[0] == "reset"] == [("reset", [2])]
    first = [e for e in events if e[0] == "extend"][0]
    assert [c for _, _, c in first[1]] == [30, 12]                # two dialogues open with chunks of different lengths
    got, _ = _drive_stack(E, H, F, L, cap, events, slab, pe, xs)
    for d, w in enumerate(want):
        have = torch.stack([got[(d, t)] for t in range(w.shape[0])])
        _close(have, w, OUT_TOL, "extend + step stack (%d, %d, %d) dialogue %d (%d rows)" % (E, H, F, d, w.shape[0]))


@pytest.mark.parametrize("split", [[110], [109, 1]], ids=["extend110", "extend109_step"])
def test_stack_one_slot_to_the_last_position(split):
    E, H, F, L = 64, 4, 128, 1
    slab, pe, xs, P = _stack_case(E, H, F, L, 1)
    want = _stack_oracle(xs[0], P, H, L)
    events = XO.mixed_schedule([(0, 0, MAX_LEN)], [split], [0])
    got, _ = _drive_stack(E, H, F, L, 1, events, slab, pe, xs)
    have = torch.stack([got[(0, t)] for t in range(MAX_LEN)])
    _close(have, want, OUT_TOL, "extend stack, capacity 1, positions 0 .. 109 as %r" % (split,))


def test_stack_padded_rows_change_no_bit():
    E, H, F, L, cap = 100, 10, 2048, 2, 4
    slab, pe, xs, _ = _stack_case(E, H, F, L, 3)
    lens = [21, 3, 9]
    events = [("extend", [(d, 0, n) for d, n in enumerate(lens)], [2, 0, 3])]
    a, cache_a = _drive_stack(E, H, F, L, cap, events, slab, pe, xs, pad=0.0)
    b, cache_b = _drive_stack(E, H, F, L, cap, events, slab, pe, xs, pad=-7.25)
    assert set(a) == set(b) and len(a) == sum(lens)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(bits(cache_a), bits(cache_b))


# ================================================================================================================
# sessions
# ================================================================================================================
WIDTHS = {"acoustic": 100, "visual": 512, "text": 100}
KEYS = ("acoustic", "visual", "text")
LENS = [n for _, _, n in SO.SHORT]             # 9, 1, 5


def _padded(inp, cols, counts, m):
    """time-major padded inputs [m, n, width] of the dialogues `cols`, their first counts[i] utterances"""
    out = []
    for k in KEYS:
        x = torch.zeros(m, len(cols), WIDTHS[k], device="cuda")
        for i, (d, c) in enumerate(zip(cols, counts)):
            x[:c, i] = inp[k][d][:c]
        out.append(x)
    return out


def _run(sess, inp, order=(0, 2)):
    """extend dialogues 0 and 2 by all but their last utterance (columns in `order`), then one step over the three dialogues
    (dialogue 1 has one utterance) -> {(dialogue, t): log_prob row (a copy)}"""
    counts = [LENS[d] - 1 for d in order]
    lp = sess.extend(*_padded(inp, order, counts, 8), counts, slots=list(order))
    assert tuple(lp.shape) == (8, 2, 6)
    got = {(d, t): lp[t, i].clone() for i, d in enumerate(order) for t in range(LENS[d] - 1)}
    last = sess.step(*(torch.stack([inp[k][d][LENS[d] - 1] for d in range(3)]) for k in KEYS))
    for d in range(3):
        got[(d, LENS[d] - 1)] = last[d].clone()
    torch.cuda.synchronize()
    return got


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.fixture(scope="module")
def session_case():
    """2-layer generators at the real widths, a causal classifier, seeded inputs, one session's outputs"""
    from gan_ffn_amd import model as M
    torch.manual_seed(29)
    gens = {k: cls(100, num_layers=2).cuda() for k, cls in zip(KEYS, (M.AcousticGenerator, M.VisualGenerator, M.TextGenerator))}
    net = M.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, causal=True).cuda()
    g = torch.Generator().manual_seed(43)
    inp = {k: [torch.rand(n, WIDTHS[k], generator=g).cuda() for n in LENS] for k in KEYS}
    sess = net.stream(capacity=3)
    base = _run(sess, inp)
    return dict(gens=gens, net=net, inp=inp, sess=sess, base=base)


def test_session_extend_then_step_matches_gan_ffn_oracle_per_dialogue(session_case):
    c = session_case
    net = c["net"]
    og = {k: O.OracleNet("gen", {n: v.detach().cpu() for n, v in c["gens"][k].state_dict().items()}, c["gens"][k].nhead,
                         dtype=torch.float64, n_layers=2) for k in KEYS}
    fc_w, fc_b = net.fc.weight.detach().cpu().double(), net.fc.bias.detach().cpu().double()
    assert len(c["base"]) == sum(LENS)
    for d, n in enumerate(LENS):
        a, v, t = (c["inp"][k][d].cpu().double().unsqueeze(1) for k in KEYS)
        with torch.no_grad(), causal_attention():
            want = O.gan_ffn_forward(a, v, t, og, fc_w, fc_b)[:, 0]
        have = torch.stack([c["base"][(d, u)] for u in range(n)])
        _close(have, want, OUT_TOL, "session extend + step log_prob, dialogue %d (%d utterances)" % (d, n))
    assert c["sess"].positions.tolist() == LENS and c["sess"]._host_pos == LENS


def test_session_replay_after_reset_gives_the_same_bits(session_case):
    c = session_case
    c["sess"].reset()
    assert c["sess"].positions.tolist() == [0, 0, 0]
    _same_bits(_run(c["sess"], c["inp"]), c["base"])          # a used session after reset() + extend ...
    _same_bits(_run(c["net"].stream(capacity=3), c["inp"]), c["base"])          # ... and a fresh one


def test_session_column_order_changes_no_bit(session_case):
    c = session_case
    _same_bits(_run(c["net"].stream(capacity=3), c["inp"], order=(2, 0)), c["base"])


def test_session_split_over_dialogue_groups_equals_the_unsplit_call(session_case, monkeypatch):
    from gan_ffn_amd import ops
    c = session_case
    monkeypatch.setattr(ops, "STREAM_EXTEND_MAX_ROWS", 8)           # m = 8: one dialogue per native call
    sess = c["net"].stream(capacity=3)
    got = _run(sess, c["inp"])
    assert len(sess._ext_bufs[(8, 2)].groups) == 2 and len(c["sess"]._ext_bufs[(8, 2)].groups) == 1
    _same_bits(got, c["base"])


def test_session_refusals_move_no_position_and_launch_nothing(session_case):
    c = session_case
    sess = c["net"].stream(capacity=3, max_len=7)
    x = {k: torch.rand(4, 3, WIDTHS[k], device="cuda") for k in KEYS}
    xs = lambda m=4, n=3: [x[k][:m, :n] for k in KEYS]
    sess.extend(*xs(), [4, 1, 3])
    assert sess.positions.tolist() == [4, 1, 3]

    def state():
        torch.cuda.synchronize()
        return (sess.positions.tolist(), list(sess._host_pos), [int(bits(ch).to(torch.int64).sum()) for ch in sess.caches])

    before = state()
    bad = [
        (xs(), dict(lengths=[4, 1]), "lengths"),
        (xs(), dict(lengths=[4, 0, 3]), r"outside \[1, m=4\]"),
        (xs(), dict(lengths=[5, 1, 3]), r"outside \[1, m=4\]"),
        (xs(n=2), dict(lengths=[1, 1]), "capacity"),
        (xs(n=2), dict(lengths=[1, 1], slots=[1, 1]), "distinct"),
        (xs(n=2), dict(lengths=[1, 1], slots=[0, 3]), "slot 3"),
        (xs(n=2), dict(lengths=[1, 1], slots=[0]), "slots"),
        ([x["acoustic"], x["visual"][:3], x["text"]], dict(lengths=[1, 1, 1]), "inputs must be"),
        ([x["acoustic"][0], x["visual"][0], x["text"][0]], dict(lengths=[1, 1, 1]), "inputs must be"),
        ([x["acoustic"], x["text"], x["text"]], dict(lengths=[1, 1, 1]), "inputs must be"),
        (xs(), dict(lengths=[4, 4, 4]), "slot 0 holds 4 of max_len=7 utterances: 3 more fit, not 4"),
    ]
    for args, kw, match in bad:
        with pytest.raises(ValueError, match=match):
            sess.extend(*args, **kw)
        assert state() == before, match
    with pytest.raises(ValueError, match="6 more fit, not 7"):
        big = [torch.rand(7, 1, WIDTHS[k], device="cuda") for k in KEYS]
        sess.extend(*big, [7], slots=[1])
    with pytest.raises(ValueError, match="max_len"):
        sess.extend(*[torch.rand(11, 1, WIDTHS[k], device="cuda") for k in KEYS], [1], slots=[0])
    assert state() == before
    sess.extend(*[t[:3] for t in xs()], [3, 2, 1], slots=[2, 0, 1])          # still usable: slot 2 to 6, slot 0 to 6, slot 1 to 2
    assert sess.positions.tolist() == [6, 2, 6] and sess._host_pos == [6, 2, 6]
