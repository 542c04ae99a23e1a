"""The encoder and head size functions and refusals of csrc/api.hip, without a GPU.

Sizes: every value of the nine size functions over the grid below equals the table in encoder_layout_sizes.json, which was
recorded from the library of the commit before the layouts were written once (`PYTHONPATH=. GANFFN_LIB=<that library> python
tests/test_encoder_layout_cpu.py` rewrites it; never from a library whose layout code is under test).  Every engine and the
streaming session size their buffers from these functions, so a layout that moves shows here first.

Refusals: each one below happens before the first HIP call, so the entry points are called with placeholder pointers; the
return code and the message of ganffn_last_error() are compared with what is written out here, word for word."""
import ctypes as C
import json
import os

from head_cases import WIDTHS as HEAD_WIDTHS

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "encoder_layout_sizes.json")
GRID_S, GRID_B, GRID_L = (1, 3, 94, 110), (1, 2, 32, 33), (1, 2, 8, 10, 64)
GRID_EHF = ((100, 10, 2048), (64, 4, 128), (512, 8, 2048), (12, 1, 4), (640, 10, 2048))
HEAD_T = (1, 3, 6016)
ENC_COLUMNS = ["saved", "workspace", "hidden_offset(0)", "hidden_offset(L-1)", "hidden_offset(L)", "fwd_pair_workspace",
               "stream_cache", "stream_workspace(1)", "stream_workspace(B)", "stream_workspace(B+1)", "stream_extend_workspace(1)",
               "stream_extend_workspace(S*B)", "stream_extend_workspace(S*B+1)"]
FAKE = 0x1000          # a 16-byte aligned address nothing dereferences: the refusals come first
ODD = 0x1004           # and one that is not 16-byte aligned


def _table():
    """{"encoder": [[S, B, E, H, F, L, <ENC_COLUMNS>]], "heads": [[T, E, D1, D2, kind, saved, workspace]]} of the loaded library"""
    from gan_ffn_amd import _lib
    lib = _lib.load()
    enc, heads = [], []
    for S in GRID_S:
        for B in GRID_B:
            for E, H, F in GRID_EHF:
                for L in GRID_L:
                    c = C.byref(_lib.EncCfg(S, B, E, H, F, L, 0.1, 0.2, 1e-5, 0))
                    enc.append([S, B, E, H, F, L, lib.ganffn_encoder_saved_floats(c), lib.ganffn_encoder_workspace_floats(c)] +
                               [lib.ganffn_encoder_saved_hidden_offset(c, l) for l in (0, L - 1, L)] +
                               [lib.ganffn_encoder_fwd_pair_workspace_floats(c), lib.ganffn_stream_cache_floats(c)] +
                               [lib.ganffn_stream_workspace_floats(c, n) for n in (1, B, B + 1)] +
                               [lib.ganffn_stream_extend_workspace_floats(c, r) for r in (1, S * B, S * B + 1)])
    for T in HEAD_T:
        for E, D1, D2 in HEAD_WIDTHS:
            for kind in (0, 1):
                c = C.byref(_lib.HeadCfg(T, E, D1, D2, kind, 0.2, 0))
                heads.append([T, E, D1, D2, kind, lib.ganffn_head_saved_floats(c), lib.ganffn_head_workspace_floats(c)])
    return {"encoder": [[int(v) for v in r] for r in enc], "heads": [[int(v) for v in r] for r in heads]}


def test_every_size_equals_the_recorded_table():
    with open(TABLE) as f:
        want = json.load(f)
    got = _table()
    assert len(got["encoder"]) == len(GRID_S) * len(GRID_B) * len(GRID_EHF) * len(GRID_L) == len(want["encoder"])
    assert len(got["heads"]) == len(HEAD_T) * len(HEAD_WIDTHS) * 2 == len(want["heads"])
    for g, w in zip(got["encoder"], want["encoder"]):
        assert g == w, dict(zip(["S", "B", "E", "H", "F", "L"] + ENC_COLUMNS, zip(g, w)))
    for g, w in zip(got["heads"], want["heads"]):
        assert g == w, dict(zip(["T", "E", "D1", "D2", "kind", "saved", "workspace"], zip(g, w)))
    # the table is not vacuous: every function has accepted and refused (-1) rows where it has limits
    rows = want["encoder"]
    assert all(r[6] > 0 and r[7] > 0 and r[8] > 0 and r[9] > 0 and r[10] == -1 and r[11] > 0 for r in rows)
    assert any(r[12] > 0 for r in rows) and all(r[15] == -1 and r[18] == -1 for r in rows)
    assert any(h[5] == -1 for h in want["heads"]) and any(h[5] > 0 and h[4] == 1 for h in want["heads"])


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
ENC = {"fwd": "cfg x pe params out saved ws rng add stream",
       "fwd_len": "cfg key_len x pe params out saved ws rng add stream",
       "fwd_mask": "cfg key_len flags x pe params out saved ws rng add stream",
       "fwd_pair": "cfg x pe params out out2 saved ws rng add stream",
       "fwd_pair_len": "cfg key_len x pe params out out2 saved ws rng add stream",
       "bwd": "cfg lo hi dx params grads saved ws rng add stream",
       "bwd2": "cfg lo hi dx params grads saved ws rng add need stream",
       "bwd_len": "cfg key_len lo hi dx params grads saved ws rng add need stream",
       "bwd_mask": "cfg key_len flags lo hi dx params grads saved ws rng add need stream",
       "bwd_parts": "cfg dx params grads saved ws rng add need poff pstride nparts stream",
       "bwd_parts_len": "cfg key_len dx params grads saved ws rng add need poff pstride nparts stream"}
FWD, PAIR = ("fwd", "fwd_len", "fwd_mask"), ("fwd_pair", "fwd_pair_len")
BWD, PARTS = ("bwd", "bwd2", "bwd_len", "bwd_mask"), ("bwd_parts", "bwd_parts_len")
HEAD = {"fwd": "cfg x w1 b1 w2 b2 w3 b3 out saved ws rng add stream",
        "bwd": "cfg d_out x w1 w2 w3 gw1 gb1 gw2 gb2 gw3 gb3 dx saved ws rng add stream"}


def _cfg(S=5, E=100, H=10, F=2048, L=2, train=0, p=0.1):
    from gan_ffn_amd import _lib
    return _lib.EncCfg(S, 3, E, H, F, L, p, p, 1e-5, train)


def _hcfg(kind=1, train=0):
    from gan_ffn_amd import _lib
    return _lib.HeadCfg(3, 100, 64, 16, kind, 0.2, train)


def _call(prefix, table, what, over):
    """(return code, last error) of <prefix><what> with placeholder arguments nothing is wrong with, then `over`"""
    from gan_ffn_amd import _lib
    lib = _lib.load()
    a = {k: FAKE for k in table[what].split()}
    a.update(cfg=_cfg() if table is ENC else _hcfg(), key_len=None, flags=C.c_uint32(0), lo=0, hi=2, need=1, add=C.c_uint64(0),
             stream=None, poff=C.byref(C.c_int64(0)), pstride=C.byref(C.c_int64(0)), nparts=C.byref(C.c_int(0)))
    a.update(over)
    if a["cfg"] is not None:
        a["cfg"] = C.byref(a["cfg"])
    args = [a[k] for k in table[what].split()]
    assert len(args) == len(_lib.SIGNATURES[prefix + what][1]), what
    rc = getattr(lib, prefix + what)(*args)
    return int(rc), (lib.ganffn_last_error() or b"").decode()


def _refused(what, message, head=False, **over):
    rc, msg = _call("ganffn_head_" if head else "ganffn_encoder_", HEAD if head else ENC, what, over)
    assert rc == -1, (what, rc, msg)
    assert msg == message, (what, msg)


def test_null_cfg():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    for what in ENC:
        _refused(what, "null cfg", cfg=None)
    for what in HEAD:
        _refused(what, "null head cfg", head=True, cfg=None)
    for fn in ("ganffn_encoder_saved_floats", "ganffn_encoder_workspace_floats", "ganffn_encoder_fwd_pair_workspace_floats",
               "ganffn_stream_cache_floats", "ganffn_head_saved_floats", "ganffn_head_workspace_floats"):
        assert getattr(lib, fn)(None) == -1 and b"null" in lib.ganffn_last_error(), fn
    assert lib.ganffn_encoder_saved_hidden_offset(None, 0) == -1
    assert lib.ganffn_stream_workspace_floats(None, 1) == -1 and lib.ganffn_stream_extend_workspace_floats(None, 1) == -1
    assert lib.ganffn_encoder_fwd_pair_supported(None) == 0 and lib.ganffn_encoder_bwd_parts_supported(None) == -1


def test_a_bad_cfg_is_refused_before_anything_else():
    for what in ENC:
        _refused(what, "S=111 out of range [1,110] (PositionalEncoding max_len, model.py:1179)", cfg=_cfg(S=111), x=None, dx=None)
        _refused(what, "E=100 not divisible by H=7", cfg=_cfg(H=7))


def test_unknown_flag_bits():
    _refused("fwd_mask", "encoder_fwd: unknown flag bits 0x2", flags=C.c_uint32(2))
    _refused("fwd_mask", "encoder_fwd: unknown flag bits 0xfffffffe", flags=C.c_uint32(0xFFFFFFFF), x=None)
    _refused("bwd_mask", "encoder_bwd: unknown flag bits 0x6", flags=C.c_uint32(7))
    _refused("bwd_mask", "encoder_bwd: unknown flag bits 0x80000000", flags=C.c_uint32(0x80000000), dx=None, lo=5)
    # the causal bit itself passes: the next refusal is another one
    _refused("fwd_mask", "encoder_fwd: null pointer", flags=C.c_uint32(1), x=None)
    _refused("bwd_mask", "encoder_bwd: null pointer", flags=C.c_uint32(1), dx=None)


def test_null_pointers():
    for what in FWD:
        for k in "x pe params out ws".split():
            _refused(what, "encoder_fwd: null pointer", **{k: None})
    for what in PAIR:
        for k in "x pe params out out2 saved ws".split():
            _refused(what, "encoder_fwd_pair: null pointer", **{k: None})
    for what in BWD + PARTS:
        for k in "dx params saved ws".split():
            _refused(what, "encoder_bwd: null pointer", **{k: None})
    for what in PARTS:
        for k in "grads poff pstride nparts".split():
            _refused(what, "encoder_bwd_parts: null pointer", **{k: None})
        _refused(what, "encoder_bwd_parts: null pointer", grads=None, dx=None)
    for k in "x w1 b1 w2 b2 out saved".split():
        _refused("fwd", "head_fwd: null pointer", head=True, **{k: None})
    for k in "d_out x w1 w2 dx saved ws".split():
        _refused("bwd", "head_bwd: null pointer", head=True, **{k: None})
    _refused("fwd", "head_fwd: disc needs fc3", head=True, w3=None)
    _refused("fwd", "head_fwd: disc needs fc3", head=True, b3=None)
    _refused("bwd", "head_bwd: disc needs fc3", head=True, w3=None)


def test_layer_range():
    for what in BWD:
        for lo, hi in ((1, 1), (-1, 2), (0, 3), (2, 1)):
            _refused(what, "encoder_bwd: bad layer range [%d,%d)" % (lo, hi), lo=lo, hi=hi)
        # the range is looked at after the pointers and before the alignment
        _refused(what, "encoder_bwd: null pointer", lo=1, hi=1, saved=None)
        _refused(what, "encoder_bwd: bad layer range [1,1)", lo=1, hi=1, ws=ODD)


def test_misaligned_buffers():
    for what in FWD:
        for k in "x params out ws saved".split():
            _refused(what, "encoder_fwd: buffers must be 16-byte aligned", **{k: ODD})
    for what in PAIR:
        for k in "x params out out2 saved ws".split():
            _refused(what, "encoder_fwd_pair: buffers must be 16-byte aligned", **{k: ODD})
    for what in BWD + PARTS:
        for k in "dx params saved ws grads".split():
            _refused(what, "encoder_bwd: buffers must be 16-byte aligned", **{k: ODD})
    _refused("bwd", "head_bwd: workspace must be 16-byte aligned", head=True, ws=ODD)


def test_train_mode_needs_the_rng():
    train = _cfg(train=1)
    for what in FWD:
        _refused(what, "encoder_fwd: rng required in train mode", cfg=train, rng=None)
        _refused(what, "encoder_fwd: buffers must be 16-byte aligned", cfg=train, rng=None, ws=ODD)
    for what in PAIR:
        _refused(what, "encoder_fwd_pair: rng required in train mode", cfg=train, rng=None)
    for what in BWD + PARTS:
        _refused(what, "encoder_bwd: rng required in train mode", cfg=train, rng=None)
    _refused("fwd", "head_fwd: rng required in train mode", head=True, cfg=_hcfg(train=1), rng=None)
    _refused("bwd", "head_bwd: rng required in train mode", head=True, cfg=_hcfg(train=1), rng=None)


def test_stacks_without_unreduced_weight_gradients():
    message = ("encoder_bwd_parts: this stack's weight gradients are reduced in the launch "
               "(ask ganffn_encoder_bwd_parts_supported)")
    for what in PARTS:
        _refused(what, message, cfg=_cfg(E=64, H=4, F=128))
        _refused(what, message, cfg=_cfg(L=11))
        _refused(what, message, cfg=_cfg(F=1024), dx=None)


def test_unpaired_head_gradients():
    for kind in (0, 1):
        for n in "123":
            _refused("bwd", "head_bwd: gb%s given without gw%s (a bias gradient needs its weight gradient)" % (n, n), head=True,
                     cfg=_hcfg(kind), **{"gw" + n: None})
        _refused("bwd", "head_bwd: gw3 given without gb3 (the fc3 gradients are reduced together)", head=True, cfg=_hcfg(kind), gb3=None)
        # refused after the rng and before any launch; a pair that is absent altogether is no refusal of this kind
        _refused("bwd", "head_bwd: rng required in train mode", head=True, cfg=_hcfg(kind, train=1), rng=None, gw1=None)
        _refused("bwd", "head_bwd: gb2 given without gw2 (a bias gradient needs its weight gradient)", head=True, cfg=_hcfg(kind),
                 gw1=None, gb1=None, gw2=None)


def test_head_cfg():
    from gan_ffn_amd import _lib
    for what in HEAD:
        _refused(what, "disc head: D2=36 > 32", head=True, cfg=_lib.HeadCfg(3, 100, 64, 36, 1, 0.2, 0))
        _refused(what, "head: kind=2", head=True, cfg=_lib.HeadCfg(3, 100, 64, 16, 2, 0.2, 0), x=None)
        _refused(what, "head: D1=62 D2=16 must be multiples of 4", head=True, cfg=_lib.HeadCfg(3, 100, 62, 16, 1, 0.2, 0))


if __name__ == "__main__":
    with open(TABLE, "w") as f:
        json.dump(_table(), f, separators=(",", ":"))
        f.write("\n")
