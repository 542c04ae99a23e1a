"""The stream prefill on the CPU: the fp64 restatement of the chunk call (tests/stream_extend_oracle.py) against the causal oracle
run on each dialogue alone — however a dialogue is cut into chunks and single steps, its rows must be the rows of its full causal
forward — the chunk skip rule, the argument checks of the three new entry points and the signature of StreamSession.extend."""
import ctypes as C
import inspect

import pytest
import torch

from oracle import ganffn_oracle as O
from causal_oracle import causal_attention
import stream_oracle as SO
import stream_extend_oracle as XO
from test_stream_cpu import TOL, _rel

E, H, F, L = 64, 4, 128, 2


@pytest.fixture(scope="module")
def stack_case():
    """seeded parameters, the five STAGGERED dialogues' inputs and their causal-oracle rows (computed once, left unchanged)"""
    P = SO.random_stack_params(E, F, L, seed=5)
    g = torch.Generator().manual_seed(6)
    xs = [torch.rand(n, E, generator=g, dtype=torch.float64) for _, _, n in SO.STAGGERED]
    want = []
    for x in xs:
        with causal_attention():
            want.append(O.encoder_stack(x.unsqueeze(1), P, H, None, n_layers=L)[:, 0])
    return P, xs, want


@pytest.mark.parametrize("split", [[66], [1, 65], [30, 1, 1, 1, 33]], ids=lambda s: "-".join(map(str, s)))
def test_any_split_of_a_dialogue_gives_the_rows_of_the_causal_oracle(stack_case, split):
    P, xs, want = stack_case
    x = xs[0]
    assert x.shape[0] == 66
    st = XO.ExtendStack(P, H, L, capacity=2)
    rows = []
    for first, c in XO.pieces(66, split):
        if c == 1:
            rows.append(st.step(x[first:first + 1], [1]))
            st.advance([1])
        else:
            # m above the count and a NaN pad: rows j >= count are not looked at by anything a valid row depends on
            pad = torch.full((c + 2, 1, E), float("nan"), dtype=torch.float64)
            pad[:c, 0] = x[first:first + c]
            rows.append(st.extend(pad, [1], [c])[:c, 0])
            st.advance_chunks([1], [c], c + 2)
    have = torch.cat(rows)
    assert st.pos == [0, 66]
    assert _rel(have, want[0]) < TOL, _rel(have, want[0])


def test_interleaved_dialogues_in_chunks_and_steps_equal_the_causal_oracle_per_dialogue(stack_case):
    P, xs, want = stack_case
    cap = 4
    st = XO.ExtendStack(P, H, L, cap)
    ev = XO.mixed_schedule(SO.STAGGERED, XO.STAGGERED_SPLITS, XO.STAGGERED_STARTS)
    assert [e for e in ev if e[0] == "reset"] == [("reset", [2])]
    ext = [e for e in ev if e[0] == "extend"]
    assert [c for _, _, c in ext[0][1]] == [30, 12] and all(first == 0 for _, first, _ in ext[0][1])     # two dialogues open together
    assert any(len(e[1]) == 3 for e in ext) and any(e[0] == "step" for e in ev)
    got = {}
    for e in ev:
        if e[0] == "reset":
            st.reset(e[1])
        elif e[0] == "step":
            out = st.step(torch.stack([xs[d][t] for d, t in e[1]]), e[2])
            st.advance(e[2])
            for i, (d, t) in enumerate(e[1]):
                got[(d, t)] = out[i]
        else:
            x, counts = XO.pad_chunks(xs, e[1])
            out = st.extend(x, e[2], counts)
            st.advance_chunks(e[2], counts, x.shape[0])
            for i, (d, first, c) in enumerate(e[1]):
                for j in range(c):
                    got[(d, first + j)] = out[j, i]
    assert len(got) == sum(n for _, _, n in SO.STAGGERED)
    for d, w in enumerate(want):
        have = torch.stack([got[(d, t)] for t in range(w.shape[0])])
        assert _rel(have, w) < TOL, (d, _rel(have, w))


def test_classifier_extend_then_step_equals_gan_ffn_forward_per_dialogue():
    Lc, cap, n_classes, Dh = 2, 3, 6, 16
    dims = {"acoustic": (20, 2, 32, 24), "visual": (48, 4, 64, 40), "text": (20, 2, 32, 24)}       # E, H, F, D1
    params = {k: SO.random_stack_params(e, f, Lc, seed=10 + i, head=(D1, Dh)) for i, (k, (e, h, f, D1)) in enumerate(dims.items())}
    heads = {k: v[1] for k, v in dims.items()}
    g = torch.Generator().manual_seed(7)
    fc_w = torch.rand(n_classes, Dh, generator=g, dtype=torch.float64) - 0.5
    fc_b = torch.rand(n_classes, generator=g, dtype=torch.float64) - 0.5
    lens = [9, 2, 5]
    xs = {k: [torch.rand(n, dims[k][0], generator=g, dtype=torch.float64) for n in lens] for k in dims}
    clf = XO.ExtendClassifier(params, heads, Lc, fc_w, fc_b, cap)
    counts = [n - 1 for n in lens]            # all but the last utterance in one call, then one step
    m = max(counts)
    pad = {k: torch.zeros(m, cap, dims[k][0], dtype=torch.float64) for k in dims}
    for k in dims:
        for i, c in enumerate(counts):
            pad[k][:c, i] = xs[k][i][:c]
    lp = clf.extend(pad["acoustic"], pad["visual"], pad["text"], [0, 1, 2], counts)
    last = clf.step(*(torch.stack([xs[k][i][-1] for i in range(cap)]) for k in dims), [0, 1, 2])
    assert clf.stacks["visual"].pos == lens
    gens = {k: O.OracleNet("gen", params[k], heads[k], dtype=torch.float64, n_layers=Lc) for k in dims}
    for i, n in enumerate(lens):
        with causal_attention(), torch.no_grad():
            want = O.gan_ffn_forward(xs["acoustic"][i].unsqueeze(1), xs["visual"][i].unsqueeze(1), xs["text"][i].unsqueeze(1), gens,
                                     fc_w, fc_b)[:, 0]
        have = torch.cat([lp[:n - 1, i], last[i:i + 1]])
        assert _rel(have, want) < TOL, (i, _rel(have, want))


def test_skipped_chunks_are_zero_and_leave_the_cache_alone():
    e, h, f, l, cap, max_len, m = 16, 2, 32, 2, 4, 6, 3
    P = SO.random_stack_params(e, f, l, seed=9)
    st = XO.ExtendStack(P, h, l, cap, max_len=max_len)
    g = torch.Generator().manual_seed(1)
    st.extend(torch.rand(4, 1, e, generator=g, dtype=torch.float64), [1], [4])
    st.advance_chunks([1], [4], 4)
    assert st.pos == [0, 4, 0, 0]

    def snap():
        return [[[r.clone() for r in st.K[k][s]] + [r.clone() for r in st.V[k][s]] for s in range(cap)] for k in range(l)]

    before = snap()
    # per chunk (slot, count): out of range at both ends, past max_len (4 + 3 > 6), count above m, negative count, count 0,
    # and one live chunk beside each pair
    for slots, counts, live in (([-1, cap, 0], [2, 2, 2], 2), ([1, 2, 3], [3, m + 1, 1], 2), ([2, 3, 0], [-1, 0, 3], 2)):
        x = torch.rand(m, 3, e, generator=g, dtype=torch.float64)
        qkv = torch.rand(m, 3, 3 * e, generator=g, dtype=torch.float64)
        c_live, s_live = counts[live], slots[live]
        x0 = st.pe_gather_chunk(x, slots, counts)
        assert bool((x0[:, :2] == 0).all()) and bool((x0[c_live:, 2] == 0).all())
        assert bool((x0[:c_live, 2] == x[:c_live, 2] + st.pe[:c_live]).all())
        o = st.attention_chunk(0, qkv, slots, counts)
        assert bool((o[:, :2] == 0).all()) and bool((o[c_live:, 2] == 0).all())
        assert bool((o[0, 2] == qkv[0, 2, 2 * e:]).all())          # one key: the output is its value
        st.advance_chunks(slots, counts, m)
        now = snap()
        for k in range(l):
            for s in range(cap):
                if s == s_live and k == 0:
                    assert len(now[k][s]) == len(before[k][s]) + 2 * c_live
                else:
                    assert len(now[k][s]) == len(before[k][s]) and all(bool((a == b).all()) for a, b in zip(now[k][s], before[k][s]))
        assert st.pos[1] == 4
        st.reset([s_live])
    assert st.pos == [0, 4, 0, 0]


def test_extend_entry_points_check_their_arguments():
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    cfg = ops.enc_cfg(110, 4, 100, 10, 2, train=False)
    err = lib.ganffn_last_error
    wsf = lib.ganffn_stream_extend_workspace_floats
    w8 = int(wsf(C.byref(cfg), 8))
    assert w8 > 0 and int(wsf(C.byref(cfg), 440)) > w8
    assert int(wsf(C.byref(cfg), 0)) < 0 and b"rows_max=0" in err()
    assert int(wsf(C.byref(cfg), -3)) < 0 and b"rows_max=-3" in err()
    train = ops.enc_cfg(110, 4, 100, 10, 2, train=True)
    assert int(wsf(C.byref(train), 8)) < 0 and b"train" in err()
    odd_hd = ops.enc_cfg(110, 4, 100, 20, 2, train=False)            # head_dim 5
    assert int(wsf(C.byref(odd_hd), 8)) < 0 and b"head_dim" in err()
    p = C.c_void_p(4096)              # aligned, never dereferenced: every check comes before any device call
    odd = C.c_void_p(4100)
    ext = lib.ganffn_encoder_stream_extend
    big = C.c_int64(1 << 40)

    def call(c=cfg, n=2, m=4, slot=p, count=p, pos=p, x=p, pe=p, params=p, cache=p, out=p, ws=p, ws_floats=big):
        return ext(C.byref(c), n, m, slot, count, pos, x, pe, params, cache, out, ws, ws_floats, None)

    assert call(count=None) < 0 and b"null" in err()
    assert call(ws=None) < 0 and b"null" in err()
    assert call(n=0) < 0 and b"n=0" in err()
    assert call(n=5) < 0 and b"n=5" in err()
    assert call(m=0) < 0 and b"m=0" in err()
    assert call(m=111) < 0 and b"m=111" in err()
    assert call(n=3, m=3, ws_floats=C.c_int64(w8)) < 0 and b"m*n=9" in err()          # rows_max = 8
    assert call(c=train) < 0 and b"train" in err()
    assert call(c=odd_hd) < 0 and b"head_dim" in err()
    assert call(x=odd) < 0 and b"aligned" in err()
    assert call(cache=odd) < 0 and b"aligned" in err()
    att = lib.ganffn_stream_attention_chunk

    def attn(qkv=p, cache=p, slot=p, count=p, pos=p, o=p, n=2, m=4, cap=4, max_len=110, e=100, h=10):
        return att(qkv, cache, slot, count, pos, o, n, m, cap, max_len, e, h, None)

    assert attn(qkv=None) < 0 and b"null" in err()
    assert attn(count=None) < 0 and b"null" in err()
    assert attn(n=0) < 0 and b"n=0" in err()
    assert attn(n=5) < 0 and b"n=5" in err()
    assert attn(cap=257, n=1) < 0 and b"capacity=257" in err()
    assert attn(m=0) < 0 and b"m=0" in err()
    assert attn(m=111) < 0 and b"m=111" in err()
    assert attn(max_len=111) < 0 and b"max_len" in err()
    assert attn(m=5, max_len=4) < 0 and b"m=5" in err()
    assert attn(h=20) < 0 and b"head_dim" in err()                     # head_dim 5: odd
    assert attn(e=1024, h=8) < 0 and b"E=1024" in err()
    assert attn(o=odd) < 0 and b"aligned" in err()
    assert attn(cache=odd) < 0 and b"aligned" in err()
    # the step's entry points and the version are what they were
    assert int(lib.ganffn_stream_workspace_floats(C.byref(cfg), 5)) < 0 and b"n_max" in err()
    assert lib.ganffn_version() == 100
    assert ops.STREAM_EXTEND_MAX_ROWS == 110 * 32


def test_extend_signature_and_host_checks():
    from gan_ffn_amd import model as M, streaming
    sig = inspect.signature(streaming.StreamSession.extend)
    assert str(sig) == "(self, acoustic, visual, text, lengths, slots=None)"
    assert str(inspect.signature(streaming.StreamSession.step)) == "(self, acoustic, visual, text, slots=None)"
    assert not hasattr(M.GAN_FFN_DialogueRNN, "stream") and not hasattr(M.MELDLSTMModel, "stream")
