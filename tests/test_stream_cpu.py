"""The streaming step on the CPU: the fp64 restatement (tests/stream_oracle.py: K / V lists per slot, slot / pos indirection, skip
rule, reset) against the causal oracle run on each dialogue alone — a step's row must be the matching row of the dialogue's full
causal forward — and the `stream` switch of GAN_FFN."""
import inspect

import pytest
import torch

from oracle import ganffn_oracle as O
from causal_oracle import causal_attention
import stream_oracle as SO

TOL = 1e-10          # of scale: both sides are fp64 and differ in summation order only


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _run_schedule(dialogues, step, reset, inputs):
    """drive `step(rows of each input, slots)` through the schedule -> {(dialogue, t): output row}"""
    got = {}
    for ev in SO.schedule(dialogues):
        if ev[0] == "reset":
            reset(ev[1])
            continue
        _, rows, slots = ev
        out = step([torch.stack([x[d][t] for d, t in rows]) for x in inputs], slots)
        for i, key in enumerate(rows):
            assert key not in got
            got[key] = out[i]
    assert len(got) == sum(n for _, _, n in dialogues)
    return got


def test_schedule_is_the_staggered_one():
    ev = SO.schedule(SO.STAGGERED)
    steps = [e for e in ev if e[0] == "step"]
    assert sorted(n for _, _, n in SO.STAGGERED)[-4:] == [6, 17, 40, 66] and [n for _, _, n in SO.STAGGERED][:4] == [66, 40, 1, 17]
    assert {len(e[1]) for e in steps} == {1, 2, 3, 4}                  # n < capacity and n == capacity
    assert [e for e in ev if e[0] == "reset"] == [("reset", [2])]      # one slot reset and reused
    assert len({a for _, a, _ in SO.STAGGERED}) == len(SO.STAGGERED)   # every dialogue starts at a step of its own
    for e in steps:
        assert len(set(e[2])) == len(e[2])


def test_stack_steps_equal_rows_of_the_causal_oracle_per_dialogue():
    E, H, F, L, cap = 64, 4, 128, 2, 4
    P = SO.random_stack_params(E, F, L, seed=5)
    g = torch.Generator().manual_seed(6)
    xs = [torch.rand(n, E, generator=g, dtype=torch.float64) for _, _, n in SO.STAGGERED]
    st = SO.StreamStack(P, H, L, cap)

    def step(inp, slots):
        out = st.step(inp[0], slots)
        st.advance(slots)
        return out

    got = _run_schedule(SO.STAGGERED, step, st.reset, [xs])
    worst = 0.0
    for d, x in enumerate(xs):
        with causal_attention():
            want = O.encoder_stack(x.unsqueeze(1), P, H, None, n_layers=L)[:, 0]
        # (and the oracle tells causal from bidirectional on this dialogue, unless it has a single row)
        if x.shape[0] > 1:
            bi = O.encoder_stack(x.unsqueeze(1), P, H, None, n_layers=L)[:, 0]
            assert _rel(bi[:-1], want[:-1]) > 1e-4
        have = torch.stack([got[(d, t)] for t in range(x.shape[0])])
        worst = max(worst, _rel(have, want))
        assert _rel(have, want) < TOL, (d, _rel(have, want))
    print("stream stack vs causal oracle per dialogue: worst err / scale %.3g" % worst)


def test_classifier_steps_equal_rows_of_gan_ffn_forward_per_dialogue():
    L, cap, n_classes, Dh = 2, 4, 6, 16
    dims = {"acoustic": (20, 2, 32, 24), "visual": (48, 4, 64, 40), "text": (20, 2, 32, 24)}       # E, H, F, D1
    params = {k: SO.random_stack_params(E, F, L, seed=10 + i, head=(D1, Dh)) for i, (k, (E, H, F, D1)) in enumerate(dims.items())}
    heads = {k: v[1] for k, v in dims.items()}
    g = torch.Generator().manual_seed(7)
    fc_w = (torch.rand(n_classes, Dh, generator=g, dtype=torch.float64) - 0.5)
    fc_b = (torch.rand(n_classes, generator=g, dtype=torch.float64) - 0.5)
    xs = {k: [torch.rand(n, dims[k][0], generator=g, dtype=torch.float64) for _, _, n in SO.STAGGERED] for k in dims}
    clf = SO.StreamClassifier(params, heads, L, fc_w, fc_b, cap)
    got = _run_schedule(SO.STAGGERED, lambda inp, slots: clf.step(inp[0], inp[1], inp[2], slots), clf.reset,
                        [xs["acoustic"], xs["visual"], xs["text"]])
    gens = {k: O.OracleNet("gen", params[k], heads[k], dtype=torch.float64, n_layers=L) for k in dims}
    for d in range(len(SO.STAGGERED)):
        with causal_attention(), torch.no_grad():
            want = O.gan_ffn_forward(xs["acoustic"][d].unsqueeze(1), xs["visual"][d].unsqueeze(1), xs["text"][d].unsqueeze(1), gens,
                                     fc_w, fc_b)[:, 0]
        have = torch.stack([got[(d, t)] for t in range(want.shape[0])])
        assert _rel(have, want) < TOL, (d, _rel(have, want))


def test_skipped_rows_are_zero_and_leave_the_cache_alone():
    E, H, F, L, cap, max_len = 16, 2, 32, 2, 3, 4
    P = SO.random_stack_params(E, F, L, seed=9)
    st = SO.StreamStack(P, H, L, cap, max_len=max_len)
    g = torch.Generator().manual_seed(1)
    for _ in range(max_len):                      # fill slot 1 to max_len
        st.step(torch.rand(1, E, generator=g, dtype=torch.float64), [1])
        st.advance([1])
    assert st.pos == [0, max_len, 0]
    before = [[[r.clone() for r in st.K[l][s]] + [r.clone() for r in st.V[l][s]] for s in range(cap)] for l in range(L)]
    # row 0: a full slot; row 1: slot out of range (both ends); row 2: a live slot
    for slots in ([1, cap, 0], [1, -1, 2]):
        x = torch.rand(3, E, generator=g, dtype=torch.float64)
        qkv = torch.rand(3, 3 * E, generator=g, dtype=torch.float64)
        x0 = st.pe_gather(x, slots)
        assert bool((x0[:2] == 0).all()) and bool((x0[2] == x[2] + st.pe[0]).all())
        o = st.attention(0, qkv, slots)
        assert bool((o[:2] == 0).all()) and bool((o[2] == qkv[2, 2 * E:]).all())      # one key: the output is its value
        st.advance(slots)
        assert st.pos[1] == max_len
        live = slots[2]
        for l in range(L):
            for s in range(cap):
                now = st.K[l][s] + st.V[l][s]
                if s == live and l == 0:
                    assert len(now) == len(before[l][s]) + 2
                else:
                    assert len(now) == len(before[l][s]) and all(bool((a == b).all()) for a, b in zip(now, before[l][s])), (l, s)
        st.reset([live])
    st.reset([1])
    assert st.pos == [0, 0, 0] and st.K[0][1] == []


def _net(causal, mask_padding=False):
    from gan_ffn_amd import model as M
    gens = [cls(100, num_layers=1) for cls in (M.AcousticGenerator, M.VisualGenerator, M.TextGenerator)]
    return M.GAN_FFN(*gens, causal=causal, mask_padding=mask_padding)


def test_stream_refuses_a_bidirectional_classifier():
    with pytest.raises(ValueError, match="causal"):
        _net(causal=False).stream()
    with pytest.raises(ValueError, match="causal"):
        _net(causal=False, mask_padding=True).stream(capacity=2)


def test_stream_defaults_and_argument_checks():
    from gan_ffn_amd import model as M, streaming, _lib
    sig = inspect.signature(M.GAN_FFN.stream).parameters
    assert sig["capacity"].default == 1 and sig["use_graph"].default is False and sig["max_len"].default == M.MAX_LEN == 110
    sig = inspect.signature(streaming.StreamSession.step).parameters
    assert list(sig) == ["self", "acoustic", "visual", "text", "slots"] and sig["slots"].default is None
    net = _net(causal=True)
    for kw in (dict(capacity=0), dict(capacity=257), dict(max_len=0), dict(max_len=111)):
        with pytest.raises(ValueError):
            net.stream(**kw)
    with pytest.raises(_lib.GanffnError, match="GPU"):       # parameters on the CPU: no fallback
        net.stream()
    # the DialogueRNN and MELD classifiers have bidirectional recurrent heads: nothing to stream
    assert not hasattr(M.GAN_FFN_DialogueRNN, "stream") and not hasattr(M.MELDLSTMModel, "stream")


def test_stream_entry_points_check_their_arguments():
    import ctypes as C
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    cfg = ops.enc_cfg(110, 4, 100, 10, 2, train=False)
    E, L, cap, S = 100, 2, 4, 110
    assert int(lib.ganffn_stream_cache_floats(C.byref(cfg))) == L * cap * 2 * S * E
    assert int(lib.ganffn_stream_workspace_floats(C.byref(cfg), 4)) > 0
    assert int(lib.ganffn_stream_workspace_floats(C.byref(cfg), 5)) < 0 and b"n_max" in lib.ganffn_last_error()
    train = ops.enc_cfg(110, 4, 100, 10, 2, train=True)
    assert int(lib.ganffn_stream_cache_floats(C.byref(train))) < 0 and b"train" in lib.ganffn_last_error()
    assert int(lib.ganffn_stream_cache_floats(C.byref(ops.enc_cfg(111, 4, 100, 10, 2)))) < 0
    assert int(lib.ganffn_stream_cache_floats(C.byref(ops.enc_cfg(110, 257, 100, 10, 2)))) < 0
    p = C.c_void_p(4096)              # aligned, never dereferenced: every check comes before any device call
    odd = C.c_void_p(4100)
    step = lib.ganffn_encoder_stream_step
    assert step(C.byref(cfg), 1, None, p, p, p, p, p, p, p, None) < 0 and b"null" in lib.ganffn_last_error()
    assert step(C.byref(cfg), 0, p, p, p, p, p, p, p, p, None) < 0 and b"n=0" in lib.ganffn_last_error()
    assert step(C.byref(cfg), 5, p, p, p, p, p, p, p, p, None) < 0 and b"n=5" in lib.ganffn_last_error()
    assert step(C.byref(train), 1, p, p, p, p, p, p, p, p, None) < 0 and b"train" in lib.ganffn_last_error()
    assert step(C.byref(cfg), 1, p, p, p, p, p, odd, p, p, None) < 0 and b"aligned" in lib.ganffn_last_error()
    att = lib.ganffn_stream_attention
    assert att(None, p, p, p, p, 1, 4, 110, 100, 10, None) < 0 and b"null" in lib.ganffn_last_error()
    assert att(p, p, p, p, p, 5, 4, 110, 100, 10, None) < 0 and b"n=5" in lib.ganffn_last_error()
    assert att(p, p, p, p, p, 1, 4, 111, 100, 10, None) < 0 and b"max_len" in lib.ganffn_last_error()
    assert att(p, p, p, p, p, 1, 4, 110, 100, 20, None) < 0 and b"head_dim" in lib.ganffn_last_error()       # head_dim 5: odd
    assert att(p, odd, p, p, p, 1, 4, 110, 100, 10, None) < 0 and b"aligned" in lib.ganffn_last_error()
    assert lib.ganffn_version() == 100
