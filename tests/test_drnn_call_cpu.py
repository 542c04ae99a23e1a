"""The one place that decides which entry-point family of the DialogueRNN recurrence a call takes, and the one packed
parameter slab of the step runners, without a GPU: ops.drnn_family against a table written out here, the argument list
ops.drnn_fwd_raw / drnn_bwd_raw hand to _lib.call for every family (name, count against _lib.SIGNATURES, order), ops.drnn_floats
against the families' own size functions, and engine._ParamSlab's packing on CPU tensors."""
import ctypes as C

import pytest
import torch

ATT_TYPES = ["general", "simple", "dot", "general2", "concat"]

# (parties, attention type, listener) -> family, for at most 32 dialogues; more than 32 dialogues: "batch", whatever the rest
FAMILY_UP_TO_32 = {
    (1, "general", 0): "party", (1, "general", 1): "party", (1, "simple", 0): "party", (1, "simple", 1): "party",
    (1, "dot", 0): "party", (1, "dot", 1): "party", (1, "general2", 0): "party", (1, "general2", 1): "party",
    (1, "concat", 0): "party", (1, "concat", 1): "party",
    (2, "general", 0): "", (2, "general", 1): "listener", (2, "simple", 0): "att", (2, "simple", 1): "att",
    (2, "dot", 0): "att", (2, "dot", 1): "att", (2, "general2", 0): "att", (2, "general2", 1): "att",
    (2, "concat", 0): "att", (2, "concat", 1): "att",
    (3, "general", 0): "party", (3, "general", 1): "party", (3, "simple", 0): "party", (3, "simple", 1): "party",
    (3, "dot", 0): "party", (3, "dot", 1): "party", (3, "general2", 0): "party", (3, "general2", 1): "party",
    (3, "concat", 0): "party", (3, "concat", 1): "party",
}


def test_family_rule_against_the_table():
    from gan_ffn_amd import _lib, ops
    assert sorted(_lib.DRNN_ATT_TYPES) == sorted(ATT_TYPES) and len(FAMILY_UP_TO_32) == 3 * 5 * 2
    for (parties, att, listener), want in FAMILY_UP_TO_32.items():
        for att_type in (att, _lib.DRNN_ATT_TYPES[att]):                 # by name and by DrnnAtt.type value
            for B in (1, 32):
                assert ops.drnn_family(B, parties, att_type, bool(listener)) == want, (B, parties, att_type, listener)
            for B in (33, 256):
                assert ops.drnn_family(B, parties, att_type, bool(listener)) == "batch", (B, parties, att_type, listener)


# the argument lists, written out: forward and backward of every family (the offset and the stream follow)
FWD = {"": "cfg ndir U spk mval P e alpha saved ws rng",
       "listener": "cfg ndir U spk mval P LP e alpha saved ws rng",
       "att": "cfg acfg ndir U spk mval P LP AP e alpha saved ws rng",
       "party": "cfg acfg parties ndir U spk mval P LP AP e alpha saved ws rng",
       "batch": "cfg acfg parties ndir U spk mval P LP AP e alpha saved ws rng"}
BWD = {"": "cfg ndir d_e U spk mval P G dU alpha saved ws rng",
       "listener": "cfg ndir d_e U spk mval P LP G LG dU alpha saved ws rng",
       "att": "cfg acfg ndir d_e U spk mval P LP AP G LG AG dU alpha saved ws rng",
       "party": "cfg acfg parties ndir d_e U spk mval P LP AP G LG AG dU alpha saved ws rng",
       "batch": "cfg acfg parties ndir d_e U spk mval P LP AP G LG AG dU alpha saved ws rng"}
# family -> (B, parties, attention type, listener) of a call that takes it
TAKES = {"": (3, 2, "general", False), "listener": (3, 2, "general", True), "att": (3, 2, "dot", True),
         "party": (3, 3, "general", False), "batch": (33, 2, "general", True)}


@pytest.mark.parametrize("family", list(TAKES))
def test_raw_calls_pass_the_familys_argument_list(family, monkeypatch):
    from gan_ffn_amd import _lib, ops
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    B, parties, att, listener = TAKES[family]
    s = {k: "<%s>" % k for k in "U spk mval P LP AP e alpha saved ws rng d_e G LG AG dU".split()}
    s.update(cfg=_lib.DrnnCfg(5, B, 100, 500, 100, 0.1, 1), acfg=_lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], 0), parties=parties, ndir=2)
    if not listener:
        s["LP"] = s["LG"] = None
    ops.drnn_fwd_raw(*[s[k] for k in "cfg acfg parties ndir U spk mval P LP AP e alpha saved ws rng".split()], 77)
    ops.drnn_bwd_raw(*[s[k] for k in "cfg acfg parties ndir d_e U spk mval P LP AP G LG AG dU alpha saved ws rng".split()], 78)
    assert len(calls) == 2
    infix = family + "_" if family else ""
    for (name, a), what, table, add in zip(calls, ("fwd", "bwd"), (FWD, BWD), (77, 78)):
        assert name == "ganffn_drnn_" + infix + what
        assert len(a) == len(_lib.SIGNATURES[name][1]), name
        want = [s[k] for k in table[family].split()]
        assert len(a) == len(want) + 2
        for i, (got, w) in enumerate(zip(a, want)):
            assert got is w, (name, i, got, w)
        assert isinstance(a[-2], C.c_uint64) and a[-2].value == add
        assert a[-1] == "the stream"


@pytest.mark.parametrize("B", [3, 33])
def test_sizes_equal_the_familys_own_size_functions(B):
    from gan_ffn_amd import _lib, ops
    lib = _lib.load()
    cfg = _lib.DrnnCfg(5, B, 100, 500, 100, 0.1, 1)
    seen = set()
    for att, da in (("general", 0), ("concat", 8)):
        a = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], da)
        for listener in (0, 1):
            for parties in (2, 3):
                if B > 32:
                    fam, args = "batch_", (C.byref(cfg), C.byref(a), listener, parties)
                elif parties == 3:
                    fam, args = "party_", (C.byref(cfg), C.byref(a), listener, parties)
                elif att == "concat":
                    fam, args = "att_", (C.byref(cfg), C.byref(a), listener)
                else:
                    fam, args = ("listener_" if listener else ""), (C.byref(cfg),)
                want = tuple(int(getattr(lib, "ganffn_drnn_%s%s_floats" % (fam, w))(*args)) for w in ("saved", "workspace"))
                assert want[0] > 0 and want[1] > 0
                assert ops.drnn_floats(cfg, a, bool(listener), parties) == want, (att, listener, parties)
                seen.add(fam)
    assert seen == ({"batch_"} if B > 32 else {"", "listener_", "att_", "party_"})


def test_sizes_raise_past_the_party_limit():
    from gan_ffn_amd import _lib, ops
    cfg = _lib.DrnnCfg(5, 33, 100, 500, 100, 0.1, 1)
    with pytest.raises(_lib.GanffnError):
        ops.drnn_floats(cfg, _lib.DrnnAtt(0, 0), False, ops.DRNN_MAX_PARTIES + 1)


def test_param_slab_packs_pads_and_notices_a_moved_parameter():
    from gan_ffn_amd import engine as E
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(2, 3)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 2, 2))]
    before = [p.detach().clone() for p in params]
    ps = E._ParamSlab(params, torch.device("cpu"))
    assert ps.offs == [0, 8, 16] and ps.total == 24 and ps.slab.numel() == 24
    for t in (ps.grad, ps.exp_avg, ps.exp_avg_sq):
        assert t.shape == ps.slab.shape and not t.any()
    assert ps.step.dtype == torch.int32 and ps.step.tolist() == [0]
    for i, (p, b) in enumerate(zip(params, before)):
        assert p.shape == b.shape and torch.equal(p.detach(), b)
        assert p.data_ptr() == ps.slab.data_ptr() + 4 * ps.offs[i]
        assert torch.equal(ps.view(i), b.reshape(-1))
        assert ps.view(i, grad=True).data_ptr() == ps.grad.data_ptr() + 4 * ps.offs[i] and ps.view(i, True).numel() == b.numel()
    assert not ps.slab[6:8].any() and not ps.slab[13:16].any()           # the padding
    assert ps.in_place()
    params[1].data = params[1].data.clone()
    assert not ps.in_place()
