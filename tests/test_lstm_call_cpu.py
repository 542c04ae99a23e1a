"""The one place that decides which entry-point family of the LSTM a call takes, without a GPU: ops.lstm_family against the
rule written out here, the argument list the four ops.lstm_*_raw helpers hand to _lib.call for every family — the one-direction
family (ndir=1) among them — (name, count against _lib.SIGNATURES, order, lengths in second place), ops.lstm_sizes against the size
functions the table names, and the twenty ganffn_lstm_* signatures against a literal copy."""
import ctypes as C

import pytest
import torch

# family -> what its layer calls, stack calls, layer size functions and stack size functions are called
NAMES = {"": ("ganffn_lstm_layer_%s", "ganffn_lstm_stack_%s", "ganffn_lstm_%s_floats", "ganffn_lstm_stack_%s_floats"),
         "batch": ("ganffn_lstm_batch_layer_%s", "ganffn_lstm_stack_batch_%s", "ganffn_lstm_batch_%s_floats", "ganffn_lstm_stack_batch_%s_floats"),
         "packed": ("ganffn_lstm_packed_layer_%s", "ganffn_lstm_stack_packed_%s", "ganffn_lstm_batch_%s_floats", "ganffn_lstm_stack_batch_%s_floats"),
         "uni": ("ganffn_unilstm_layer_%s", "ganffn_unilstm_stack_%s", "ganffn_unilstm_%s_floats", "ganffn_unilstm_stack_%s_floats")}
# (B, packed, ndir) of a call that takes the family; the one-direction family takes lengths (here NULL) behind cfg whatever B
TAKES = {"": (3, False, 2), "batch": (33, False, 2), "packed": (3, True, 2), "uni": (40, False, 1)}


def test_family_rule():
    from gan_ffn_amd import ops
    for B, want in ((1, ""), (32, ""), (33, "batch"), (256, "batch")):
        assert ops.lstm_family(B, False) == want, B
        assert ops.lstm_family(B, True) == "packed", B
        assert ops.lstm_family(B, False, 2) == want and ops.lstm_family(B, True, 2) == "packed", B
        assert ops.lstm_family(B, False, 1) == ops.lstm_family(B, True, 1) == "uni", B


LAYER_FWD = "x w_ih w_hh b_ih b_hh out saved ws"
LAYER_BWD = "d_out x out w_ih w_hh dx gw_ih gw_hh gb_ih gb_hh saved ws"
ARRAYS = "w_ih w_hh b_ih b_hh gw_ih gw_hh gb_ih gb_hh".split()


@pytest.mark.parametrize("family", list(TAKES))
def test_raw_calls_pass_the_familys_argument_list(family, monkeypatch):
    from gan_ffn_amd import _lib, ops
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    B, packed, ndir = TAKES[family]
    kw = {} if ndir == 2 else {"ndir": ndir}                    # two directions: the default
    s = {k: torch.zeros(4) for k in "x out saved ws d_out dx rng".split()}
    s.update({k: "<%s>" % k for k in ARRAYS})                   # the pointer arrays go through as they are
    lengths = torch.zeros(B, dtype=torch.int32) if packed else None
    layer, stack = _lib.LstmCfg(5, B, 12, 8), _lib.LstmStackCfg(5, B, 12, 8, 3, 0.5, 1)
    ops.lstm_layer_fwd_raw(layer, *[s[k] for k in LAYER_FWD.split()], lengths=lengths, **kw)
    ops.lstm_layer_bwd_raw(layer, *[s[k] for k in LAYER_BWD.split()], lengths=lengths, **kw)
    ops.lstm_stack_fwd_raw(stack, *[s[k] for k in LAYER_FWD.split()], s["rng"], 77, lengths=lengths, **kw)
    ops.lstm_stack_bwd_raw(stack, *[s[k] for k in LAYER_BWD.split()], s["rng"], 78, lengths=lengths, **kw)
    assert len(calls) == 4
    want = [(NAMES[family][0] % "fwd", layer, LAYER_FWD, None), (NAMES[family][0] % "bwd", layer, LAYER_BWD, None),
            (NAMES[family][1] % "fwd", stack, LAYER_FWD + " rng", 77), (NAMES[family][1] % "bwd", stack, LAYER_BWD + " rng", 78)]
    for (name, a), (want_name, cfg, table, add) in zip(calls, want):
        assert name == want_name
        assert len(a) == len(_lib.SIGNATURES[name][1]), name
        a = list(a)
        assert C.addressof(a.pop(0)._obj) == C.addressof(cfg), name                  # byref(cfg) first
        if packed:
            got = a.pop(0)                                                           # then lengths, when given
            assert isinstance(got, C.c_void_p) and got.value == lengths.data_ptr(), name
        elif ndir == 1:
            assert a.pop(0) is None, name                                            # one direction: always there, NULL for the padded run
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
    # what may be left out is: dx and the gradient arrays go through as null
    calls.clear()
    ops.lstm_stack_bwd_raw(stack, s["d_out"], s["x"], s["out"], s["w_ih"], s["w_hh"], None, None, None, None, None, s["saved"],
                           s["ws"], s["rng"], 0, lengths=lengths, **kw)
    (name, a), = calls
    k = 6 + (packed or ndir == 1)
    assert list(a[k:k + 5]) == [None] * 5 and len(a) == len(_lib.SIGNATURES[name][1])


@pytest.mark.parametrize("family", list(TAKES))
def test_sizes_come_from_the_size_functions_the_table_names(family):
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    B, packed, ndir = TAKES[family]
    for cfg, names in ((_lib.LstmCfg(5, B, 12, 8), NAMES[family][2]), (_lib.LstmStackCfg(5, B, 12, 8, 3, 0.5, 1), NAMES[family][3])):
        want = tuple(int(getattr(lib, names % w)(C.byref(cfg))) for w in ("saved", "workspace"))
        assert want[0] > 0 and want[1] > 0
        assert ops.lstm_sizes(cfg, packed, ndir) == want
        if ndir == 2:
            assert ops.lstm_sizes(cfg, packed) == want
    assert ops.lstm_sizes(_lib.LstmCfg(5, B, 12, 8)) == ops.lstm_sizes(_lib.LstmCfg(5, B, 12, 8), False)


def test_sizes_raise_what_the_library_refuses():
    from gan_ffn_amd import _lib, ops
    for cfg, packed in ((_lib.LstmCfg(5, 257, 12, 8), False), (_lib.LstmCfg(5, 3, 6, 8), True), (_lib.LstmStackCfg(5, 3, 12, 8, 17, 0.5, 1), False),
                        (_lib.LstmStackCfg(5, 257, 12, 8, 2, 0.5, 1), True)):
        with pytest.raises(_lib.GanffnError):
            ops.lstm_sizes(cfg, packed)


def test_the_twenty_signatures_are_what_they_were():
    from gan_ffn_amd import _lib
    P, I, L, U64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    layer, stack = C.POINTER(_lib.LstmCfg), C.POINTER(_lib.LstmStackCfg)
    want = {
        "ganffn_lstm_saved_floats": (L, [layer]),
        "ganffn_lstm_workspace_floats": (L, [layer]),
        "ganffn_lstm_layer_fwd": (I, [layer] + [P] * 9),
        "ganffn_lstm_layer_bwd": (I, [layer] + [P] * 13),
        "ganffn_lstm_stack_saved_floats": (L, [stack]),
        "ganffn_lstm_stack_workspace_floats": (L, [stack]),
        "ganffn_lstm_stack_fwd": (I, [stack] + [P] * 9 + [U64, P]),
        "ganffn_lstm_stack_bwd": (I, [stack] + [P] * 13 + [U64, P]),
        "ganffn_lstm_batch_saved_floats": (L, [layer]),
        "ganffn_lstm_batch_workspace_floats": (L, [layer]),
        "ganffn_lstm_batch_layer_fwd": (I, [layer] + [P] * 9),
        "ganffn_lstm_batch_layer_bwd": (I, [layer] + [P] * 13),
        "ganffn_lstm_stack_batch_saved_floats": (L, [stack]),
        "ganffn_lstm_stack_batch_workspace_floats": (L, [stack]),
        "ganffn_lstm_stack_batch_fwd": (I, [stack] + [P] * 9 + [U64, P]),
        "ganffn_lstm_stack_batch_bwd": (I, [stack] + [P] * 13 + [U64, P]),
        "ganffn_lstm_packed_layer_fwd": (I, [layer] + [P] * 10),
        "ganffn_lstm_packed_layer_bwd": (I, [layer] + [P] * 14),
        "ganffn_lstm_stack_packed_fwd": (I, [stack] + [P] * 10 + [U64, P]),
        "ganffn_lstm_stack_packed_bwd": (I, [stack] + [P] * 14 + [U64, P]),
    }
    got = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith("ganffn_lstm_")}
    assert sorted(got) == sorted(want) and len(want) == 20
    for name, (res, args) in want.items():
        assert got[name][0] is res and list(got[name][1]) == args, name
