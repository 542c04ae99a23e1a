"""What the DialogueRNN entry points refuse, without a GPU: every refusal below happens before the first HIP call, so the C
entry points are called with placeholder pointers and the nonzero return code and a stable piece of ganffn_last_error()
are compared with what is written out here.  The argument lists per family are those of test_drnn_call_cpu.py."""
import ctypes as C

import pytest

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
SIZES = {"": "cfg", "listener": "cfg", "att": "cfg acfg listener", "party": "cfg acfg listener parties",
         "batch": "cfg acfg listener parties"}
FAMILIES = list(FWD)
DESCRIPTOR_FAMILIES = ["att", "party", "batch"]
FAKE = 0x1000          # a 16-byte aligned address nothing dereferences: the refusals come first


def _args(**over):
    """the full named argument set of a call nothing is wrong with (placeholder pointers), then `over`"""
    from gan_ffn_amd import _lib
    two = lambda: (C.c_void_p * 2)(FAKE, FAKE)
    a = {k: two() for k in "U spk mval e alpha saved ws d_e dU".split()}

    def structs(cls):
        arr = (cls * 2)()
        for s in arr:
            for name, _ in cls._fields_:
                setattr(s, name, FAKE)
        return arr

    a.update(P=structs(_lib.DrnnPtrs), G=structs(_lib.DrnnPtrs), LP=structs(_lib.DrnnListenerPtrs),
             LG=structs(_lib.DrnnListenerPtrs), AP=structs(_lib.DrnnAttPtrs), AG=structs(_lib.DrnnAttPtrs),
             cfg=_lib.DrnnCfg(5, 3, 8, 8, 8, 0.0, 0), acfg=_lib.DrnnAtt(0, 0), parties=2, ndir=1, listener=0,
             rng=(C.c_uint64 * 2)(1, 2))
    a.update(over)
    return a


def _call(family, what, a):
    """(return code, last error) of ganffn_drnn_<family>_<what> with the family's argument list taken from `a`"""
    from gan_ffn_amd import _lib
    lib = _lib.load()
    name = "ganffn_drnn_%s%s" % (family + "_" if family else "", what)
    table = {"fwd": FWD, "bwd": BWD}.get(what, SIZES)[family]
    by_ref = lambda k: C.byref(a[k]) if k in ("cfg", "acfg") and a[k] is not None else a[k]
    args = [by_ref(k) for k in table.split()]
    if what in ("fwd", "bwd"):
        args += [C.c_uint64(0), None]
    assert len(args) == len(_lib.SIGNATURES[name][1]), name
    rc = getattr(lib, name)(*args)
    return int(rc), (lib.ganffn_last_error() or b"").decode()


def _refused(family, what, a, piece):
    rc, msg = _call(family, what, a)
    assert rc == -1, (family, what, rc)
    assert piece in msg, (family, what, msg)


SIZE_FNS = ("saved_floats", "workspace_floats")


@pytest.mark.parametrize("family", FAMILIES)
def test_null_cfg(family):
    for what in ("fwd", "bwd") + SIZE_FNS:
        _refused(family, what, _args(cfg=None), "null drnn cfg")


@pytest.mark.parametrize("family", ["", "listener", "att", "party"])
def test_33_dialogues_only_through_the_batch_family(family):
    from gan_ffn_amd import _lib
    cfg = _lib.DrnnCfg(5, 33, 8, 8, 8, 0.0, 0)
    for what in ("fwd", "bwd") + SIZE_FNS:
        _refused(family, what, _args(cfg=cfg), "drnn: S=5 (<= 112), B=33 (<= 32)")
    for what in SIZE_FNS:
        rc, _ = _call("batch", what, _args(cfg=cfg))
        assert rc > 0
    # and the batch calls get past the limit: the next refusal is their own
    _refused("batch", "fwd", _args(cfg=cfg, U=None), "drnn_fwd: null pointer")
    _refused("batch", "bwd", _args(cfg=cfg, U=None), "drnn_bwd: null pointer")
    _refused("batch", "fwd", _args(cfg=_lib.DrnnCfg(5, 257, 8, 8, 8, 0.0, 0)), "B=257 (<= 256)")


@pytest.mark.parametrize("parties", [0, 17])
@pytest.mark.parametrize("family", ["party", "batch"])
def test_party_count_outside_the_limits(family, parties):
    for what in ("fwd", "bwd") + SIZE_FNS:
        _refused(family, what, _args(parties=parties), "drnn_party: parties=%d outside [1, 16]" % parties)
    # the party count is looked at before the cfg
    _refused(family, "fwd", _args(parties=parties, cfg=None), "drnn_party: parties=%d" % parties)
    _refused(family, "bwd", _args(parties=parties, cfg=None), "drnn_party: parties=%d" % parties)


@pytest.mark.parametrize("family", DESCRIPTOR_FAMILIES)
def test_attention_descriptor(family):
    from gan_ffn_amd import _lib
    T = _lib.DRNN_ATT_TYPES
    for what in ("fwd", "bwd") + SIZE_FNS:
        _refused(family, what, _args(acfg=_lib.DrnnAtt(T["concat"], 6)), "drnn_att: concat needs D_a a multiple of 4 in [4, 512], got D_a=6")
        _refused(family, what, _args(acfg=_lib.DrnnAtt(T["dot"], 0), cfg=_lib.DrnnCfg(5, 3, 8, 12, 8, 0.0, 0)),
                 "drnn_att: dot attention needs D_m == D_g, got D_m=8 D_g=12")
        _refused(family, what, _args(acfg=_lib.DrnnAtt(5, 0)), "drnn_att: unknown attention type 5")
        _refused(family, what, _args(acfg=_lib.DrnnAtt(-1, 0)), "drnn_att: unknown attention type -1")
    for what in ("fwd", "bwd"):
        _refused(family, what, _args(acfg=None), "drnn_%s_%s: null attention descriptor" % (family, what))
        _refused(family, what, _args(AP=None), "drnn_att: null attention parameters")
        ap = _args()["AP"]
        ap[0].w = None
        _refused(family, what, _args(AP=ap), "drnn_att: direction 0: null or misaligned attention weight")
        ap = _args()["AP"]
        ap[0].b = None
        _refused(family, what, _args(AP=ap, acfg=_lib.DrnnAtt(T["general2"], 0)), "drnn_att: direction 0: general2 needs transform.bias")
        ap = _args()["AP"]
        ap[0].v = None
        _refused(family, what, _args(AP=ap, acfg=_lib.DrnnAtt(T["concat"], 8)), "drnn_att: direction 0: concat needs vector_prod.weight")
        # dot has no parameters: a null aparams passes, the next refusal is the driver's own
        _refused(family, what, _args(AP=None, acfg=_lib.DrnnAtt(T["dot"], 0), saved=None), "drnn_%s: null pointer" % what)
    for what in SIZE_FNS:
        _refused(family, what, _args(acfg=None), "drnn_att: null attention descriptor")


def test_listener_entry_needs_listener_parameters():
    for what in ("fwd", "bwd"):
        _refused("listener", what, _args(LP=None), "drnn_listener_%s: null listener parameters" % what)
        _refused("listener", what, _args(LP=None, cfg=None), "drnn_listener_%s: null listener parameters" % what)
        lp = _args()["LP"]
        lp[0].l_whh = None
        _refused("listener", what, _args(LP=lp), "drnn_listener_%s: direction 0: null listener parameter" % what)
        _refused("att", what, _args(LP=lp), "drnn_listener_%s: direction 0: null listener parameter" % what)


@pytest.mark.parametrize("family", FAMILIES)
def test_three_directions(family):
    for what in ("fwd", "bwd"):
        _refused(family, what, _args(ndir=3), "drnn: ndir=3")
        _refused(family, what, _args(ndir=0), "drnn: ndir=0")


@pytest.mark.parametrize("family", FAMILIES)
def test_train_mode_needs_the_rng_and_every_call_its_arrays(family):
    from gan_ffn_amd import _lib
    train = _lib.DrnnCfg(5, 3, 8, 8, 8, 0.1, 1)
    for what in ("fwd", "bwd"):
        _refused(family, what, _args(cfg=train, rng=None), "drnn_%s: rng required in train mode" % what)
        _refused(family, what, _args(P=None), "drnn_%s: null pointer" % what)
        _refused(family, what, _args(P=None, ndir=2), "drnn_%s: null pointer" % what)
        u = (C.c_void_p * 2)(None, FAKE)
        _refused(family, what, _args(U=u), "drnn_%s: direction 0: null" % what)
    _refused(family, "bwd", _args(G=None), "drnn_bwd: null pointer")
    _refused(family, "fwd", _args(cfg=_lib.DrnnCfg(5, 3, 8, 8, 8, 1.0, 1)), "drnn: dropout p out of [0,1)")
    _refused(family, "fwd", _args(cfg=_lib.DrnnCfg(5, 3, 8, 516, 8, 0.0, 0)), "> 512")
    _refused(family, "fwd", _args(cfg=_lib.DrnnCfg(113, 3, 8, 8, 8, 0.0, 0)), "drnn: S=113 (<= 112)")
    _refused(family, "fwd", _args(cfg=_lib.DrnnCfg(5, 3, 8, 8, 6, 0.0, 0)), "must be multiples of 4")
