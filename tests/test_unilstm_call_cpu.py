"""The one-direction LSTM family (ganffn_unilstm_*, include/ganffn.h) without a GPU: the 8 symbols and their signatures, the size
functions against the layouts written out, what the entry points refuse (an error code and a message, before any launch), and
the argument list the four ops.unilstm_*_raw helpers hand to _lib.call."""
import ctypes as C

import pytest
import torch

LAYER_FWD = "x w_ih w_hh b_ih b_hh out saved ws"
LAYER_BWD = "d_out x out w_ih w_hh dx gw_ih gw_hh gb_ih gb_hh saved ws"
ARRAYS = "w_ih w_hh b_ih b_hh gw_ih gw_hh gb_ih gb_hh".split()
# name -> number of arguments
COUNTS = {"ganffn_unilstm_saved_floats": 1, "ganffn_unilstm_workspace_floats": 1, "ganffn_unilstm_layer_fwd": 11,
          "ganffn_unilstm_layer_bwd": 15, "ganffn_unilstm_stack_saved_floats": 1, "ganffn_unilstm_stack_workspace_floats": 1,
          "ganffn_unilstm_stack_fwd": 13, "ganffn_unilstm_stack_bwd": 17}


def test_the_eight_symbols_and_their_signatures():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    P, I, L, U64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    layer, stack = C.POINTER(_lib.LstmCfg), C.POINTER(_lib.LstmStackCfg)
    want = {"ganffn_unilstm_saved_floats": (L, [layer]), "ganffn_unilstm_workspace_floats": (L, [layer]),
            "ganffn_unilstm_layer_fwd": (I, [layer] + [P] * 10), "ganffn_unilstm_layer_bwd": (I, [layer] + [P] * 14),
            "ganffn_unilstm_stack_saved_floats": (L, [stack]), "ganffn_unilstm_stack_workspace_floats": (L, [stack]),
            "ganffn_unilstm_stack_fwd": (I, [stack] + [P] * 10 + [U64, P]), "ganffn_unilstm_stack_bwd": (I, [stack] + [P] * 14 + [U64, P])}
    got = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith("ganffn_unilstm_")}
    assert sorted(got) == sorted(want) == sorted(COUNTS)
    for name, (res, args) in want.items():
        assert hasattr(lib, name), name
        assert got[name][0] is res and list(got[name][1]) == args and len(args) == COUNTS[name], name


def _sizes(lib, cfg):
    head = "ganffn_unilstm_stack_" if hasattr(cfg, "L") else "ganffn_unilstm_"
    return tuple(int(getattr(lib, head + w)(C.byref(cfg))) for w in ("saved_floats", "workspace_floats"))


def test_sizes_equal_the_layouts_written_out():
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    S, B, In, H, L = 5, 3, 12, 8, 3
    T = S * B
    layer = _lib.LstmCfg(S, B, In, H)
    n_saved, n_ws = _sizes(lib, layer)
    assert ops.unilstm_sizes(layer) == (n_saved, n_ws)
    assert n_saved == T * 4 * H + T * H                                 # gates [1][T x 4H] | c [1][T x H]
    fwd = T * 4 * H + B * 4 * H                                         # xg | G
    assert n_ws >= fwd + 64 and n_ws >= T * 4 * H + 2 * B * H + 64 + 64 # dG | dh | dc | slabs (>= 0) | the two slack terms
    # ... and half the two-direction layer's saved block, region by region
    assert 2 * n_saved == int(lib.ganffn_lstm_batch_saved_floats(C.byref(layer)))
    stack = _lib.LstmStackCfg(S, B, In, H, L, 0.5, 1)
    s_saved, s_ws = _sizes(lib, stack)
    assert ops.unilstm_sizes(stack) == (s_saved, s_ws)
    assert s_saved == L * n_saved + (L - 1) * 2 * T * H                 # per layer but the last: its output and the dropped output, T x H each
    # workspace: the widest layer's own (rounded to 4 floats) | two [T x H] gradient buffers
    widest = max(_sizes(lib, _lib.LstmCfg(S, B, w, H))[1] for w in (In, H))
    assert s_ws == (widest + 3) // 4 * 4 + 2 * T * H


def test_sizes_are_monotone_in_the_dialogue_count():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    prev = (0, 0, 0, 0)
    for B in range(1, 257):
        cur = _sizes(lib, _lib.LstmCfg(5, B, 12, 8)) + _sizes(lib, _lib.LstmStackCfg(5, B, 12, 8, 3, 0.5, 1))
        assert all(c > p for c, p in zip(cur, prev)), B
        prev = cur


def test_size_functions_refuse():
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    for cfg in (_lib.LstmCfg(5, 257, 12, 8), _lib.LstmCfg(5, 0, 12, 8), _lib.LstmCfg(5, 3, 6, 8), _lib.LstmCfg(5, 3, 12, 6),
                _lib.LstmStackCfg(5, 3, 12, 8, 17, 0.5, 1), _lib.LstmStackCfg(5, 3, 12, 8, 0, 0.5, 1),
                _lib.LstmStackCfg(5, 3, 12, 8, 2, 1.0, 1), _lib.LstmStackCfg(5, 257, 12, 8, 2, 0.5, 1)):
        assert _sizes(lib, cfg) == (-1, -1)
        with pytest.raises(_lib.GanffnError):
            ops.unilstm_sizes(cfg)


class _Host:
    """16-byte aligned host buffers: the refusals below come before any launch, so nothing is read through these pointers"""

    def __init__(self):
        self.keep = []

    def buf(self, n_floats=64, misalign=0):
        raw = (C.c_char * (4 * n_floats + 32))()
        self.keep.append(raw)
        a = C.addressof(raw)
        return C.c_void_p((a + 15) // 16 * 16 + misalign)

    def arr(self, n):
        a = (C.c_void_p * n)(*[self.buf().value for _ in range(n)])
        self.keep.append(a)
        return a


def _layer_fwd(lib, h, cfg, x="buf", ws_mis=0):
    return lib.ganffn_unilstm_layer_fwd(C.byref(cfg), None, h.buf() if x == "buf" else None, h.arr(1), h.arr(1), h.arr(1), h.arr(1),
                                        h.buf(), h.buf(), h.buf(misalign=ws_mis), None)


def _stack_fwd(lib, h, cfg, rng=None):
    n = max(1, min(cfg.L, 16))
    return lib.ganffn_unilstm_stack_fwd(C.byref(cfg), None, h.buf(), h.arr(n), h.arr(n), h.arr(n), h.arr(n), h.buf(), h.buf(), h.buf(),
                                        rng, C.c_uint64(0), None)


def _stack_bwd(lib, h, cfg, rng=None):
    n = max(1, min(cfg.L, 16))
    return lib.ganffn_unilstm_stack_bwd(C.byref(cfg), None, h.buf(), h.buf(), h.buf(), h.arr(n), h.arr(n), None, None, None, None, None,
                                        h.buf(), h.buf(), rng, C.c_uint64(0), None)


def test_entry_points_refuse_with_an_error_and_do_not_crash():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    h = _Host()
    ok = _lib.LstmCfg(5, 3, 12, 8)
    refused = [
        ("B = 257", lambda: _layer_fwd(lib, h, _lib.LstmCfg(5, 257, 12, 8))),
        ("In = 6", lambda: _layer_fwd(lib, h, _lib.LstmCfg(5, 3, 6, 8))),
        ("null x", lambda: _layer_fwd(lib, h, ok, x=None)),
        ("misaligned workspace", lambda: _layer_fwd(lib, h, ok, ws_mis=4)),
        ("null x, backward", lambda: lib.ganffn_unilstm_layer_bwd(C.byref(ok), None, h.buf(), None, h.buf(), h.arr(1), h.arr(1), None,
                                                                  None, None, None, None, h.buf(), h.buf(), None)),
        ("L = 17", lambda: _stack_fwd(lib, h, _lib.LstmStackCfg(5, 3, 12, 8, 17, 0.5, 1))),
        ("p = 1.0", lambda: _stack_fwd(lib, h, _lib.LstmStackCfg(5, 3, 12, 8, 3, 1.0, 1))),
        ("B = 257, stack", lambda: _stack_fwd(lib, h, _lib.LstmStackCfg(5, 257, 12, 8, 3, 0.5, 1))),
        ("train mode without rng", lambda: _stack_fwd(lib, h, _lib.LstmStackCfg(5, 3, 12, 8, 3, 0.5, 1))),
        ("train mode without rng, backward", lambda: _stack_bwd(lib, h, _lib.LstmStackCfg(5, 3, 12, 8, 3, 0.5, 1))),
    ]
    for what, call in refused:
        assert call() != 0, what
        assert lib.ganffn_last_error(), what


@pytest.mark.parametrize("packed", [False, True])
def test_raw_calls_pass_cfg_lengths_the_arrays_and_the_stream(packed, monkeypatch):
    from gan_ffn_amd import _lib, ops
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    B = 40
    s = {k: torch.zeros(4) for k in "x out saved ws d_out dx rng".split()}
    s.update({k: "<%s>" % k for k in ARRAYS})                   # the pointer arrays go through as they are
    lengths = torch.zeros(B, dtype=torch.int32) if packed else None
    layer, stack = _lib.LstmCfg(5, B, 12, 8), _lib.LstmStackCfg(5, B, 12, 8, 3, 0.5, 1)
    ops.unilstm_layer_fwd_raw(layer, *[s[k] for k in LAYER_FWD.split()], lengths=lengths)
    ops.unilstm_layer_bwd_raw(layer, *[s[k] for k in LAYER_BWD.split()], lengths=lengths)
    ops.unilstm_stack_fwd_raw(stack, *[s[k] for k in LAYER_FWD.split()], s["rng"], 77, lengths=lengths)
    ops.unilstm_stack_bwd_raw(stack, *[s[k] for k in LAYER_BWD.split()], s["rng"], 78, lengths=lengths)
    want = [("ganffn_unilstm_layer_fwd", layer, LAYER_FWD, None), ("ganffn_unilstm_layer_bwd", layer, LAYER_BWD, None),
            ("ganffn_unilstm_stack_fwd", stack, LAYER_FWD + " rng", 77), ("ganffn_unilstm_stack_bwd", stack, LAYER_BWD + " rng", 78)]
    assert len(calls) == 4
    for (name, a), (want_name, cfg, table, add) in zip(calls, want):
        assert name == want_name
        assert len(a) == len(_lib.SIGNATURES[name][1]) == COUNTS[name], name
        a = list(a)
        assert C.addressof(a.pop(0)._obj) == C.addressof(cfg), name                  # byref(cfg) first
        got = a.pop(0)                                                               # then lengths: a pointer, or NULL
        if packed:
            assert isinstance(got, C.c_void_p) and got.value == lengths.data_ptr(), name
        else:
            assert got is None, name
        assert a.pop() == "the stream"
        if add is not None:
            got = a.pop()
            assert isinstance(got, C.c_uint64) and got.value == add
        assert len(a) == len(table.split())
        for got, k in zip(a, table.split()):
            if k in ARRAYS:
                assert got is s[k], (name, k)
            else:
                assert isinstance(got, C.c_void_p) and got.value == s[k].data_ptr(), (name, k)
    # what may be left out: dx and the gradient arrays go through as null
    calls.clear()
    ops.unilstm_stack_bwd_raw(stack, s["d_out"], s["x"], s["out"], s["w_ih"], s["w_hh"], None, None, None, None, None, s["saved"],
                              s["ws"], s["rng"], 0, lengths=lengths)
    (name, a), = calls
    assert list(a[7:12]) == [None] * 5 and len(a) == COUNTS[name]

