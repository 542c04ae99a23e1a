"""The streamed causal MELD classifier on the CPU: the fp64 step over explicit Hs / Cs / E arrays (tests/meld_stream_oracle.py)
against meld_causal_oracle.forward run on each dialogue ALONE — a streamed row must be the matching row of the dialogue's full
causal forward, with the state NaN wherever a step must not read —, extend against steps, what the new entry points refuse before
any launch, and the `stream` switch of MELDLSTMModel."""
import copy
import ctypes as C
import inspect

import pytest
import torch

import meld_stream_oracle as MSO
import stream_oracle as SO

TOL = 1e-12                                            # tests/test_drnn_stream_cpu.py's
DIALOGUES = [(0, 0, 13), (1, 2, 1), (2, 2, 7)]        # (slot, the step it joins at, utterances): lengths [13, 1, 7], staggered


def _model(dims=(12, 8, 8), seed=1, causal=True, **kw):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(seed)
    m = DR.MELDLSTMModel(*dims, n_classes=7, dropout=0.5, causal=causal, **kw)
    with torch.no_grad():                               # transform is initialised small: scores away from tanh's linear range
        m.matchatt.transform.weight.mul_(20.0)
    return m


def _texts(D_m, lengths, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, D_m, generator=g, dtype=torch.float64) - 0.5 for n in lengths]


def _stream(head, U, dialogues):
    got = {}
    for ev in SO.schedule(dialogues):
        if ev[0] == "reset":
            head.reset(ev[1])
            continue
        _, rows, slots = ev
        lp = head.step(torch.stack([U[d][t] for d, t in rows]), slots)
        for i, key in enumerate(rows):
            got[key] = lp[i]
    return got


@pytest.mark.parametrize("poison", [False, True], ids=["", "nan_where_unread"])
def test_streamed_steps_equal_the_causal_classifier_on_each_dialogue_alone(poison):
    m = _model().double().eval()
    lengths = [n for _, _, n in DIALOGUES]
    U = _texts(12, lengths)
    head = MSO.StreamMeld(m, capacity=3, max_len=13)
    head.poison = poison
    got = _stream(head, U, DIALOGUES)
    assert {len(e[1]) for e in SO.schedule(DIALOGUES) if e[0] == "step"} == {1, 2, 3}       # positions differ within a call
    for d, n in enumerate(lengths):
        want = MSO.alone(m, U[d])
        have = torch.stack([got[(d, t)] for t in range(n)])
        assert not bool(torch.isnan(have).any())
        assert float((have - want).abs().max()) <= TOL, (d, float((have - want).abs().max()))
    assert head.pos == lengths
    # (the comparison sees the history: the same rows without their past are far from the dialogue's)
    fresh = MSO.StreamMeld(m, capacity=1, max_len=13)
    assert float((fresh.step(U[0][5:6], [0])[0] - MSO.alone(m, U[0])[5]).abs().max()) > 1e-4


def test_extend_then_steps_equals_steps():
    m = _model(seed=2).double().eval()
    lengths, pre = [9, 1, 6], [5, 1, 3]
    U = _texts(12, lengths, seed=8)
    want = _stream(MSO.StreamMeld(m, 3, 13), U, [(d, 0, n) for d, n in enumerate(lengths)])
    head = MSO.StreamMeld(m, 3, 13)
    head.poison = True
    x = torch.full((max(pre), 3, 12), 7.0, dtype=torch.float64)          # rows past a length: finite, never used
    for i, c in enumerate(pre):
        x[:c, i] = U[i][:c]
    lp = head.extend(x, pre, [0, 1, 2])
    assert head.pos == pre
    for i, c in enumerate(pre):
        for j in range(c):
            assert float((lp[j, i] - want[(i, j)]).abs().max()) <= TOL
    for k in range(max(n - p for n, p in zip(lengths, pre))):
        rows = [d for d in range(3) if pre[d] + k < lengths[d]]
        out = head.step(torch.stack([U[d][pre[d] + k] for d in rows]), rows)
        for i, d in enumerate(rows):
            assert float((out[i] - want[(d, pre[d] + k)]).abs().max()) <= TOL
    assert head.pos == lengths


def test_skipped_rows_leave_the_oracle_state_alone():
    m = _model().double().eval()
    st = MSO.LstmState(m.lstm, 3, 4)
    x = torch.rand(3, 12, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    before = st.clone()
    out = st.step(x, [1, 3, -1], [0, 4, 0])                       # a full slot, a slot at the capacity, slot -1
    assert bool((out == 0).all())
    for a, b in ((st.Hs, before.Hs), (st.Cs, before.Cs), (st.E, before.E)):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
    out = st.step(x, [0, 1, 2], [0, 4, -1], off=1, count=[1, 1, 2])      # masked by count, full, a negative position
    assert bool((out == 0).all())
    assert st.offsets() == (0, 96, 192, 288) and st.flat().numel() == 288


# ---- the C entry points: every refusal comes before any device call -------------------------------------------------------------
def _cfg(**kw):
    from gan_ffn_amd import ops
    d = dict(capacity=4, max_len=110, In=600, H=300, L=4)
    d.update(kw)
    return ops.lstm_stream_cfg(**d)


def test_size_functions_and_their_refusals():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    state, ws = lib.ganffn_stream_lstm_state_floats, lib.ganffn_stream_lstm_workspace_floats
    a4 = MSO.a4
    cfg = _cfg()
    assert int(state(C.byref(cfg))) == a4(4 * 4 * 300) * 2 + a4(4 * 110 * 300)
    odd = _cfg(capacity=3, max_len=5, In=12, H=20, L=1)
    assert int(state(C.byref(odd))) == a4(3 * 1 * 20) * 2 + a4(3 * 5 * 20)
    assert int(ws(C.byref(cfg), 4)) > int(ws(C.byref(cfg), 1)) > 0
    assert int(ws(C.byref(_cfg(L=5)), 4)) > int(ws(C.byref(cfg), 4))
    for n_max in (0, 5):
        assert int(ws(C.byref(cfg), n_max)) == -1 and b"n_max" in lib.ganffn_last_error()
    assert int(state(None)) == -1 and b"null" in lib.ganffn_last_error()
    bad = [(dict(capacity=0), b"capacity"), (dict(capacity=257), b"capacity"), (dict(max_len=0), b"max_len"),
           (dict(max_len=111), b"max_len"), (dict(In=602), b"multiples of 4"), (dict(In=0), b"multiples of 4"),
           (dict(H=6), b"multiples of 4"), (dict(H=1028), b"1024"), (dict(L=0), b"L=0"), (dict(L=17), b"L=17")]
    for kw, word in bad:
        for fn, args in ((state, ()), (ws, (1,))):
            assert int(fn(C.byref(_cfg(**kw)), *args)) == -1, kw
            assert word in lib.ganffn_last_error(), (kw, lib.ganffn_last_error())
    assert int(state(C.byref(_cfg(H=1024, L=16, capacity=256)))) > 0


def test_step_and_extend_refusals():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    step, extend = lib.ganffn_stream_lstm_step, lib.ganffn_stream_lstm_extend
    p, odd = 4096, 4100                # never dereferenced: every check comes before any device call
    arr = lambda *v: (C.c_void_p * len(v))(*v)           # noqa: E731  (the parameter arrays are host arrays: these are read)
    good = arr(p, p, p, p)

    def call_step(cfg=None, n=1, slot=p, pos=p, off=0, count=None, x=p, w_ih=good, w_hh=good, b_ih=good, b_hh=good, state=p, e=p,
                  ws=p):
        return step(C.byref(cfg if cfg is not None else _cfg()), n, slot, pos, off, count, x, w_ih, w_hh, b_ih, b_hh, state, e, ws, None)

    def call_extend(cfg=None, n=1, m=2, slot=p, count=p, pos=p, x=p, w_ih=good, w_hh=good, b_ih=good, b_hh=good, state=p, e=p, ws=p):
        return extend(C.byref(cfg if cfg is not None else _cfg()), n, m, slot, count, pos, x, w_ih, w_hh, b_ih, b_hh, state, e, ws,
                      None)

    def refused(rc, word):
        assert rc < 0 and word in lib.ganffn_last_error(), (rc, word, lib.ganffn_last_error())

    for call in (call_step, call_extend):
        for name in ("slot", "pos", "x", "w_ih", "w_hh", "b_ih", "b_hh", "state", "e", "ws"):
            refused(call(**{name: None}), b"null")
        for name in ("x", "state", "e", "ws"):
            refused(call(**{name: odd}), b"aligned")
        refused(call(n=0), b"n=0")
        refused(call(n=5), b"n=5")
        for kw, word in ((dict(capacity=257), b"capacity"), (dict(max_len=111), b"max_len"), (dict(In=602), b"multiples of 4"),
                         (dict(H=302), b"multiples of 4"), (dict(H=1028), b"1024"), (dict(L=0), b"L=0"), (dict(L=17), b"L=17")):
            refused(call(cfg=_cfg(**kw)), word)
        for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
            refused(call(**{name: arr(p, p, None, p)}), b"layer 2")
        refused(call(w_ih=arr(p, odd, p, p)), b"layer 1")
        refused(call(w_hh=arr(p, p, p, odd)), b"layer 3")
    refused(call_step(off=-1), b"off=-1")
    refused(call_step(off=110), b"off=110")
    refused(call_extend(count=None), b"count")
    refused(call_extend(m=0), b"m=0")
    refused(call_extend(m=111), b"m=111")


# ---- the switch ------------------------------------------------------------------------------------------------------------------
def test_stream_refuses_what_cannot_stream():
    with pytest.raises(ValueError, match="causal=True.*reverse direction starts at the dialogue's end"):
        _model((12, 8, 16), causal=False).stream()
    with pytest.raises(ValueError, match="causal"):
        _model((12, 8, 16), causal=False, packed=True).stream(capacity=0)          # the first check of all
    with pytest.raises(ValueError, match="D_h == D_e"):
        _model((12, 8, 16)).stream()
    with pytest.raises(ValueError, match="lstm_supported"):
        _model((12, 6, 6)).stream()                                                # D_e not a multiple of 4
    with pytest.raises(ValueError, match="lstm_supported"):
        _model((10, 8, 8)).stream()
    wide = _model()
    wide.lstm.hidden_size = 1028                                                   # (claimed, not allocated)
    with pytest.raises(ValueError, match="limits"):
        wide.stream()
    from gan_ffn_amd import dialogue_rnn as DR
    with pytest.raises(ValueError, match="n_classes=17"):
        DR.MELDLSTMModel(12, 8, 8, n_classes=17, causal=True).stream()


def test_stream_defaults_and_argument_checks():
    from gan_ffn_amd import model as M, streaming, _lib
    net = _model()
    sig = inspect.signature(net.stream).parameters           # an instance attribute: the class itself carries no `stream`
    assert list(sig) == ["capacity", "max_len"] and not hasattr(M.MELDLSTMModel, "stream")
    assert sig["capacity"].default == 1 and sig["max_len"].default == M.MAX_LEN == 110
    assert list(inspect.signature(streaming.MeldStreamSession.step).parameters) == ["self", "text", "slots"]
    assert list(inspect.signature(streaming.MeldStreamSession.extend).parameters) == ["self", "text", "lengths", "slots"]
    twin = copy.deepcopy(net)
    assert twin.stream.__self__ is twin and net.stream.__self__ is net       # a copy streams itself, not its original
    assert "stream" not in net.state_dict() and set(twin.state_dict()) == set(net.state_dict())
    for kw in (dict(capacity=0), dict(capacity=257), dict(max_len=0), dict(max_len=111)):
        with pytest.raises(ValueError):
            net.stream(**kw)
    with pytest.raises(_lib.GanffnError, match="GPU"):       # parameters on the CPU: no fallback (and after the range checks)
        net.stream()
    # the sessions share the slot and position bookkeeping, and the generator-backed ones what they always shared
    assert issubclass(streaming.MeldStreamSession, streaming._SlotStream) and issubclass(streaming._GeneratorStream, streaming._SlotStream)
    assert not issubclass(streaming.MeldStreamSession, streaming._GeneratorStream)
    for name in ("_check_slots", "reset", "_upload_slots", "_advance"):
        assert name in vars(streaming._SlotStream) and name not in vars(streaming._GeneratorStream)
