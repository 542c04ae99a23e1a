"""The ops wrappers of the native calls made from more than one Python site, without a GPU: what general2_attention_{fwd,bwd}_raw,
add3_raw, dropout_raw and linear1_fwd_raw hand to _lib.call — the name, the count against _lib.SIGNATURES, the order, and the Python
type of every argument (a bare int, a ctypes scalar, a c_void_p, or None for NULL)."""
import ctypes as C

import pytest
import torch


@pytest.fixture
def calls(monkeypatch):
    from gan_ffn_amd import _lib, ops
    got = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: got.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    return got


def _tensors(names):
    return {k: torch.zeros(4) for k in names.split()}


def _is_ptr(got, t):
    return isinstance(got, C.c_void_p) and got.value == t.data_ptr()


def _is(got, ctype, value):
    return type(got) is ctype and got.value == value


ATT_FWD = "x mem mask att alpha tanh_s"
ATT_BWD = "d_att x mem mask alpha tanh_s du dx dmem"


@pytest.mark.parametrize("flags", [None, 1, 0])
def test_general2_attention_picks_the_entry_point_by_flags(flags, calls):
    """flags None: the plain entry points; ATTN_CAUSAL or 0: the _mask ones, the flags a c_uint32 behind the mask"""
    from gan_ffn_amd import _lib, ops
    assert ops.ATTN_CAUSAL == 1
    t = _tensors(ATT_FWD + " d_att du dx dmem")
    S, B, D = 6, 3, 8
    ops.general2_attention_fwd_raw(*[t[k] for k in ATT_FWD.split()], S, B, D, flags)
    ops.general2_attention_bwd_raw(*[t[k] for k in ATT_BWD.split()], S, B, D, flags=flags)
    assert len(calls) == 2
    tail = "" if flags is None else "_mask"
    for (name, a), want_name, table, at in zip(calls, ("fwd", "bwd"), (ATT_FWD, ATT_BWD), (3, 4)):
        assert name == "ganffn_general2_attention_" + want_name + tail
        assert len(a) == len(_lib.SIGNATURES[name][1]), name
        a = list(a)
        if flags is not None:
            assert _is(a.pop(at), C.c_uint32, flags), name
        assert a[len(table.split()):] == [S, B, D, "the stream"] and all(type(v) is int for v in a[-4:-1]), name
        for got, k in zip(a, table.split()):
            assert _is_ptr(got, t[k]), (name, k)


def test_add3(calls):
    from gan_ffn_amd import _lib, ops
    t = _tensors("a b c out")
    ops.add3_raw(t["a"], t["b"], t["c"], t["out"], 1234)
    (name, a), = calls
    assert name == "ganffn_add3" and len(a) == len(_lib.SIGNATURES[name][1]) == 6
    assert all(_is_ptr(g, t[k]) for g, k in zip(a, "a b c out".split()))
    assert _is(a[4], C.c_int64, 1234) and a[5] == "the stream"


@pytest.mark.parametrize("with_rng", [True, False])
def test_dropout_and_linear1(with_rng, calls):
    """rows / columns / sizes and the train flag go through as bare ints, p / site / add as c_float / c_uint32 / c_uint64, a missing
    rng state as NULL"""
    from gan_ffn_amd import _lib, ops
    t = _tensors("x w b out rng")
    rng = t["rng"] if with_rng else None
    ops.dropout_raw(t["x"], t["out"], 18, 8, 0.25, 5, rng, 77)
    ops.linear1_fwd_raw(t["x"], t["w"], t["b"], t["out"], 18, 8, 12, 0.5, 7, rng, 78, with_rng)
    (n_d, d), (n_l, l) = calls
    assert n_d == "ganffn_dropout" and len(d) == len(_lib.SIGNATURES[n_d][1]) == 9
    assert _is_ptr(d[0], t["x"]) and _is_ptr(d[1], t["out"]) and d[2:4] == (18, 8) and type(d[2]) is int and type(d[3]) is int
    assert _is(d[4], C.c_float, 0.25) and _is(d[5], C.c_uint32, 5) and _is(d[7], C.c_uint64, 77) and d[8] == "the stream"
    assert n_l == "ganffn_ffn_linear1_fwd" and len(l) == len(_lib.SIGNATURES[n_l][1]) == 13
    assert all(_is_ptr(g, t[k]) for g, k in zip(l, "x w b out".split()))
    assert l[4:7] == (18, 8, 12) and all(type(v) is int for v in l[4:7])
    assert _is(l[7], C.c_float, 0.5) and _is(l[8], C.c_uint32, 7) and _is(l[10], C.c_uint64, 78)
    assert l[11] == (1 if with_rng else 0) and type(l[11]) is int and l[12] == "the stream"
    for got in (d[6], l[9]):
        assert _is_ptr(got, t["rng"]) if with_rng else got is None
