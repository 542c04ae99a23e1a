"""The streamed DialogueRNN head on the CPU: the fp64 step over explicit G / Q / E arrays (tests/drnn_stream_oracle.py) against
drnn_causal_oracle.uni_head run on each dialogue ALONE — a streamed row must be the matching row of the dialogue's full causal
head, with the state NaN at and above every position too —, extend against steps, what the new entry points refuse before any
launch, and the `stream` switch of GAN_FFN_DialogueRNN."""
import ctypes as C
import inspect

import pytest
import torch

import drnn_causal_oracle as DCO
import drnn_stream_oracle as DSO
import stream_oracle as SO

TOL = 1e-12
DIMS = dict(D_m=12, D_g=16, D_p=16, D_e=8, D_h=10, D_a=12)
DIALOGUES = [(0, 0, 13), (1, 2, 1), (2, 2, 7)]        # (slot, the step it joins at, utterances): lengths [13, 1, 7], staggered
# attention type, listener state, parties
CASES = [(a, False, 2) for a in ("general", "simple", "dot", "general2", "concat")] + \
        [("general", True, 2), ("concat", True, 2), ("general", False, 1), ("general", False, 9), ("general", True, 9)]


def _uni(att, listener, seed=1):
    from gan_ffn_amd import dialogue_rnn as DR
    d = dict(DIMS)
    if att == "dot":
        d["D_m"] = d["D_g"]
    torch.manual_seed(seed)
    return DR.UniModel(n_classes=6, listener_state=listener, context_attention=att, dropout_rec=0.1, dropout=0.6, **d).double().eval()


def _dialogues(um, parties, lengths, seed=5):
    g = torch.Generator().manual_seed(seed)
    U = [torch.rand(n, um.D_m, generator=g, dtype=torch.float64) - 0.5 for n in lengths]
    spk = [torch.randint(0, parties, (n,), generator=g).tolist() for n in lengths]
    return U, spk


def _alone(um, U, spk, parties):
    """uni_head on each dialogue alone -> [log_prob (n, C)]"""
    out = []
    for u, s in zip(U, spk):
        n = u.shape[0]
        res = DCO.uni_head(um, u.unsqueeze(1), DSO.one_hot(s, parties), torch.ones(1, n, dtype=torch.float64))
        out.append(res["log_prob"][:, 0])
    return out


def _stream(head, U, spk, dialogues):
    got = {}
    for ev in SO.schedule(dialogues):
        if ev[0] == "reset":
            head.reset(ev[1])
            continue
        _, rows, slots = ev
        lp = head.step(torch.stack([U[d][t] for d, t in rows]), [spk[d][t] for d, t in rows], slots)
        for i, key in enumerate(rows):
            got[key] = lp[i]
    return got


@pytest.mark.parametrize("poison", [False, True], ids=["", "nan_above_positions"])
@pytest.mark.parametrize("att,listener,parties", CASES, ids=["%s%s_p%d" % (a, "_listener" if l else "", p) for a, l, p in CASES])
def test_streamed_steps_equal_the_causal_head_on_each_dialogue_alone(att, listener, parties, poison):
    um = _uni(att, listener)
    lengths = [n for _, _, n in DIALOGUES]
    U, spk = _dialogues(um, parties, lengths)
    want = _alone(um, U, spk, parties)
    head = DSO.StreamUni(um, capacity=3, max_len=13, parties=parties)
    head.poison = poison
    got = _stream(head, U, spk, DIALOGUES)
    assert {len(e[1]) for e in SO.schedule(DIALOGUES) if e[0] == "step"} == {1, 2, 3}       # positions differ within a call
    for d, w in enumerate(want):
        have = torch.stack([got[(d, t)] for t in range(lengths[d])])
        assert not bool(torch.isnan(have).any())
        assert float((have - w).abs().max()) <= TOL, (d, float((have - w).abs().max()))
    assert head.pos == lengths


@pytest.mark.parametrize("att,listener,parties", [("general", False, 2), ("concat", True, 9)])
def test_extend_then_steps_equals_steps(att, listener, parties):
    um = _uni(att, listener)
    lengths, pre = [9, 1, 6], [5, 1, 3]
    U, spk = _dialogues(um, parties, lengths, seed=8)
    steps = DSO.StreamUni(um, 3, 13, parties)
    want = _stream(steps, U, spk, [(d, 0, n) for d, n in enumerate(lengths)])
    head = DSO.StreamUni(um, 3, 13, parties)
    head.poison = True
    m = max(pre)
    fus = torch.full((m, 3, um.D_m), 7.0, dtype=torch.float64)          # rows past a length: finite, never used
    sp = [[parties + 3] * 3 for _ in range(m)]                          # (and their speakers are ignored)
    for i, c in enumerate(pre):
        fus[:c, i] = U[i][:c]
        for j in range(c):
            sp[j][i] = spk[i][j]
    lp = head.extend(fus, sp, pre, [0, 1, 2])
    assert head.pos == pre
    for i, c in enumerate(pre):
        for j in range(c):
            assert float((lp[j, i] - want[(i, j)]).abs().max()) <= TOL
    rest = [(d, 0, lengths[d] - pre[d]) for d in range(3) if lengths[d] > pre[d]]
    live = [d for d in range(3) if lengths[d] > pre[d]]
    for k in range(max(n for _, _, n in rest)):
        rows = [d for d in live if pre[d] + k < lengths[d]]
        out = head.step(torch.stack([U[d][pre[d] + k] for d in rows]), [spk[d][pre[d] + k] for d in rows], rows)
        for i, d in enumerate(rows):
            assert float((out[i] - want[(d, pre[d] + k)]).abs().max()) <= TOL
    assert head.pos == lengths


def test_skipped_rows_leave_the_oracle_state_alone():
    um = _uni("general", True)
    st = DSO.HeadState(um.dialog_rnn_f.dialogue_cell, 3, 4, 2)
    g = torch.Generator().manual_seed(2)
    U = torch.rand(3, um.D_m, generator=g, dtype=torch.float64)
    pos = [0, 4, 0]
    before = st.clone()
    out = st.step(U, [0, 1, 2], [1, 3, 2], pos)                    # a full slot, a slot outside the capacity, a speaker = parties
    assert bool((out == 0).all())
    for a, b in ((st.G, before.G), (st.Q, before.Q), (st.E, before.E)):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
    out = st.step(U, [0, 1, 1], [0, 1, 2], pos, off=1, count=[1, 1, 2])      # masked by count; slot 2 at t = 1 reads a NaN history
    assert bool((out[:2] == 0).all())


# ---- the C entry points: every refusal comes before any device call -------------------------------------------------------------
def _cfg(**kw):
    from gan_ffn_amd import ops
    d = dict(capacity=4, max_len=110, parties=2, Dm=100, H=500, He=100, listener=False, att="general", Da=0)
    d.update(kw)
    return ops.drnn_stream_cfg(**d)


def test_size_functions_and_their_refusals():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    state, ws = lib.ganffn_drnn_stream_state_floats, lib.ganffn_drnn_stream_workspace_floats
    cfg = _cfg()
    assert int(state(C.byref(cfg))) == 4 * 110 * 500 + 4 * 2 * 500 + 4 * 110 * 100
    odd = _cfg(capacity=3, max_len=5, parties=3, Dm=12, H=20, He=12)           # every region a multiple of 4 floats
    assert int(state(C.byref(odd))) == DSO.a4(3 * 5 * 20) + DSO.a4(3 * 3 * 20) + DSO.a4(3 * 5 * 12)
    assert int(ws(C.byref(cfg), 4)) > int(ws(C.byref(cfg), 1)) > 0
    assert int(ws(C.byref(_cfg(listener=True)), 4)) > int(ws(C.byref(cfg), 4))
    for n_max in (0, 5):
        assert int(ws(C.byref(cfg), n_max)) == -1 and b"n_max" in lib.ganffn_last_error()
    assert int(state(None)) == -1 and b"null" in lib.ganffn_last_error()
    bad = [(dict(capacity=0), b"capacity"), (dict(capacity=257), b"capacity"), (dict(max_len=0), b"max_len"),
           (dict(max_len=111), b"max_len"), (dict(parties=0), b"parties"), (dict(parties=17), b"parties"), (dict(Dm=102), b"D_m"),
           (dict(H=0), b"D_m"), (dict(He=6), b"D_m"), (dict(H=516), b"512"), (dict(att="dot"), b"dot"),
           (dict(att="concat", Da=0), b"D_a"), (dict(att="concat", Da=516), b"D_a"), (dict(att="concat", Da=6), b"D_a")]
    for kw, word in bad:
        for fn, args in ((state, ()), (ws, (1,))):
            assert int(fn(C.byref(_cfg(**kw)), *args)) == -1, kw
            assert word in lib.ganffn_last_error(), (kw, lib.ganffn_last_error())
    c = _cfg(listener=True)
    c.listener = 2
    assert int(state(C.byref(c))) == -1 and b"listener" in lib.ganffn_last_error()
    c = _cfg()
    c.att.type = 5
    assert int(state(C.byref(c))) == -1 and b"attention type" in lib.ganffn_last_error()
    assert int(state(C.byref(_cfg(att="dot", Dm=100, H=100)))) > 0 and int(state(C.byref(_cfg(att="concat", Da=100)))) > 0


def _ptrs(aligned, listener=False, att=("w",)):
    from gan_ffn_amd import _lib
    p = _lib.DrnnPtrs(*([aligned] * 12 + [None]))
    lp = _lib.DrnnListenerPtrs(*([aligned] * 4)) if listener else None
    ap = _lib.DrnnAttPtrs(**{k: aligned for k in att})
    return p, lp, ap


def test_step_and_extend_refusals():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    step, extend = lib.ganffn_drnn_stream_step, lib.ganffn_drnn_stream_extend
    p, odd = 4096, 4100                # never dereferenced: every check comes before any device call
    prm, _, ap = _ptrs(p)
    ref = lambda s: C.byref(s) if s is not None else None

    def call_step(cfg=None, n=1, slot=p, pos=p, off=0, count=None, spk=p, U=p, prm=prm, lprm=None, aprm=ap, state=p, e=p, ws=p):
        return step(C.byref(cfg if cfg is not None else _cfg()), n, slot, pos, off, count, spk, U, ref(prm), ref(lprm), ref(aprm), state,
                    e, ws, None)

    def call_extend(cfg=None, n=1, m=2, slot=p, count=p, pos=p, spk=p, U=p, prm=prm, lprm=None, aprm=ap, state=p, e=p, ws=p):
        return extend(C.byref(cfg if cfg is not None else _cfg()), n, m, slot, count, pos, spk, U, ref(prm), ref(lprm), ref(aprm),
                      state, e, ws, None)

    def refused(rc, word):
        assert rc < 0 and word in lib.ganffn_last_error(), (rc, word, lib.ganffn_last_error())

    for call in (call_step, call_extend):
        for name in ("slot", "pos", "spk", "U", "state", "e", "ws", "prm"):
            refused(call(**{name: None}), b"null")
        for name in ("U", "state", "e", "ws"):
            refused(call(**{name: odd}), b"aligned")
        refused(call(n=0), b"n=0")
        refused(call(n=5), b"n=5")
        refused(call(cfg=_cfg(H=516)), b"512")
        refused(call(cfg=_cfg(Dm=102)), b"multiples of 4")
        refused(call(cfg=_cfg(parties=17)), b"parties")
        refused(call(cfg=_cfg(max_len=111)), b"max_len")
        refused(call(cfg=_cfg(att="dot")), b"dot")
        refused(call(cfg=_cfg(att="concat", Da=516)), b"D_a")
        refused(call(cfg=_cfg(att="concat", Da=100), aprm=_ptrs(p, att=("w",))[2]), b"vector_prod")
        refused(call(cfg=_cfg(att="general2"), aprm=_ptrs(p, att=("w",))[2]), b"transform.bias")
        refused(call(aprm=None), b"attention weight")
        refused(call(aprm=_ptrs(odd)[2]), b"attention weight")
        refused(call(cfg=_cfg(listener=True)), b"listener")
        refused(call(cfg=_cfg(listener=True), lprm=_lib.DrnnListenerPtrs(p, p, None, p)), b"listener")
        refused(call(prm=_lib.DrnnPtrs(*([p] * 4 + [None] + [p] * 7 + [None]))), b"cell parameter")
        refused(call(prm=_lib.DrnnPtrs(*([odd] + [p] * 11 + [None]))), b"aligned")
    refused(call_step(off=-1), b"off=-1")
    refused(call_step(off=110), b"off=110")
    refused(call_extend(count=None), b"count")
    refused(call_extend(m=0), b"m=0")
    refused(call_extend(m=111), b"m=111")


def test_general2_stream_attention_refusals():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    att = lib.ganffn_general2_stream_attention
    p, odd = 4096, 4100

    def refused(rc, word):
        assert rc < 0 and word in lib.ganffn_last_error(), (rc, word, lib.ganffn_last_error())
    good = dict(x=p, e=p, slot=p, count=None, pos=p, att=p, alpha=None, n=1, m=1, cap=4, max_len=110, D=100)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return att(a["x"], a["e"], a["slot"], a["count"], a["pos"], a["att"], a["alpha"], a["n"], a["m"], a["cap"], a["max_len"], a["D"],
                   None)
    for name in ("x", "e", "slot", "pos", "att"):
        refused(call(**{name: None}), b"null")
    for name in ("x", "e", "att"):
        refused(call(**{name: odd}), b"aligned")
    refused(call(n=0), b"n=0")
    refused(call(n=5), b"n=5")
    refused(call(cap=257), b"capacity=257")
    refused(call(max_len=111), b"max_len")
    refused(call(m=0), b"m=0")
    refused(call(m=111), b"m=111")
    refused(call(D=102), b"D=102")
    refused(call(D=1028), b"D=1028")


# ---- the switch ------------------------------------------------------------------------------------------------------------------
def _net(causal, **kw):
    from gan_ffn_amd import model as M
    torch.manual_seed(0)
    return M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100, num_layers=1), M.VisualGenerator(100, num_layers=1),
                                 M.TextGenerator(100, num_layers=1), D_m=100, D_g=40, D_p=40, D_e=20, D_h=24, D_a=100, n_classes=6,
                                 listener_state=False, context_attention="general", dropout_rec=0.1, dropout=0.6, causal=causal, **kw)


def test_stream_refuses_the_bidirectional_head():
    with pytest.raises(ValueError, match="reads the future"):
        _net(False).stream()
    with pytest.raises(ValueError, match="reads the future"):
        _net(False, mask_padding=True).stream(capacity=0, parties=0)         # the first check of all


def test_stream_defaults_and_argument_checks():
    from gan_ffn_amd import model as M, streaming, _lib
    net = _net(True)
    sig = inspect.signature(net.stream).parameters           # an instance attribute: the class itself carries no `stream`
    assert list(sig) == ["capacity", "max_len", "parties"] and not hasattr(M.GAN_FFN_DialogueRNN, "stream")
    assert sig["capacity"].default == 1 and sig["max_len"].default == M.MAX_LEN == 110 and sig["parties"].default == 2
    assert list(inspect.signature(streaming.DrnnStreamSession.step).parameters) == ["self", "acoustic", "visual", "text", "speakers",
                                                                                     "slots"]
    assert list(inspect.signature(streaming.DrnnStreamSession.extend).parameters) == ["self", "acoustic", "visual", "text", "speakers",
                                                                                       "lengths", "slots"]
    assert not hasattr(streaming.DrnnStreamSession, "use_graph")
    import copy
    assert copy.deepcopy(net).stream.__self__ is not net       # a copy streams itself, not its original
    for kw in (dict(parties=0), dict(parties=17), dict(capacity=0), dict(capacity=257), dict(max_len=0), dict(max_len=111)):
        with pytest.raises(ValueError):
            net.stream(**kw)
    with pytest.raises(_lib.GanffnError, match="GPU"):       # parameters on the CPU: no fallback (and after the range checks)
        net.stream()
    assert issubclass(streaming.DrnnStreamSession, streaming._GeneratorStream) and issubclass(streaming.StreamSession,
                                                                                              streaming._GeneratorStream)
