"""The LSTM size functions and refusals of csrc/lstm.hip, without a GPU.

Sizes: every value of the eight size functions over the grid below equals the table in lstm_layout_sizes.json, which was recorded
from the library of the commit before the layouts were written once (`PYTHONPATH=. GANFFN_LIB=<that library> python
tests/test_lstm_layout_cpu.py` rewrites it; never from a library whose layout code is under test).  ops.lstm_forward and
MeldEngine size their buffers from these functions, so a layout that moves shows here first.

Refusals: each one below happens before the first HIP call, so the twelve entry points are called with placeholder pointers;
the return code and a stable piece of ganffn_last_error() are compared with what is written out here."""
import ctypes as C
import json
import os

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lstm_layout_sizes.json")
GRID_S, GRID_B, GRID_L = (1, 2, 7, 33, 128), (1, 3, 32, 33, 256), (1, 2, 4, 16)
GRID_INH = ((4, 4), (12, 8), (8, 12), (600, 300))
# cfgs some or every family refuses, (S, B, In, H, L, p): B = 0, B past every limit, In no multiple of 4, L = 0, L = 17, p = 1
REFUSED = ((5, 0, 12, 8, 2, 0.5), (5, 257, 12, 8, 2, 0.5), (5, 3, 6, 8, 2, 0.5), (5, 3, 12, 8, 0, 0.5), (5, 3, 12, 8, 17, 0.5),
           (5, 3, 12, 8, 2, 1.0))
LAYER_FNS = ["ganffn_lstm_saved_floats", "ganffn_lstm_workspace_floats", "ganffn_lstm_batch_saved_floats", "ganffn_lstm_batch_workspace_floats"]
STACK_FNS = ["ganffn_lstm_stack_saved_floats", "ganffn_lstm_stack_workspace_floats", "ganffn_lstm_stack_batch_saved_floats",
             "ganffn_lstm_stack_batch_workspace_floats"]
FAKE = 0x1000          # a 16-byte aligned address nothing dereferences: the refusals come first
ODD = 0x1004           # and one that is not 16-byte aligned


def _table():
    """{"layer": [[S, B, In, H, <LAYER_FNS>]], "stack": [[S, B, In, H, L, p, <STACK_FNS>]]} of the loaded library"""
    from gan_ffn_amd import _lib
    lib = _lib.load()
    layer, stack = [], []
    cfgs = [(S, B, In, H, L, 0.5) for S in GRID_S for B in GRID_B for In, H in GRID_INH for L in GRID_L] + list(REFUSED)
    for S, B, In, H, L, p in cfgs:
        if L == GRID_L[0] or (S, B, In, H, L, p) in REFUSED:
            c = C.byref(_lib.LstmCfg(S, B, In, H))
            layer.append([S, B, In, H] + [int(getattr(lib, fn)(c)) for fn in LAYER_FNS])
        c = C.byref(_lib.LstmStackCfg(S, B, In, H, L, p, 1))
        stack.append([S, B, In, H, L, p] + [int(getattr(lib, fn)(c)) for fn in STACK_FNS])
    return {"layer": layer, "stack": stack}


def test_every_size_equals_the_recorded_table():
    with open(TABLE) as f:
        want = json.load(f)
    got = _table()
    n = len(GRID_S) * len(GRID_B) * len(GRID_INH)
    assert len(got["layer"]) == n + len(REFUSED) == len(want["layer"])
    assert len(got["stack"]) == n * len(GRID_L) + len(REFUSED) == len(want["stack"])
    for g, w in zip(got["layer"], want["layer"]):
        assert g == w, dict(zip(["S", "B", "In", "H"] + LAYER_FNS, zip(g, w)))
    for g, w in zip(got["stack"], want["stack"]):
        assert g == w, dict(zip(["S", "B", "In", "H", "L", "p"] + STACK_FNS, zip(g, w)))
    # the table is not vacuous: 33 and 256 dialogues only in the batch family, whose values are the plain family's up to 32; the
    # cfgs of REFUSED are refused (-1) by every function whose cfg holds the offending field
    for rows, k in ((want["layer"], 4), (want["stack"], 6)):
        grid = rows[:-len(REFUSED)]
        assert all(r[k + 2] > 0 and r[k + 3] > 0 for r in grid)
        assert all((r[k], r[k + 1]) == ((r[k + 2], r[k + 3]) if r[1] <= 32 else (-1, -1)) for r in grid)
        assert any(r[1] > 32 for r in grid)
    assert [r[4:] for r in want["layer"][-len(REFUSED):-3]] == [[-1] * 4] * 3 and all(r[4] > 0 for r in want["layer"][-3:])
    assert [r[6:] for r in want["stack"][-len(REFUSED):]] == [[-1] * 4] * len(REFUSED)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
ARGS = {"layer_fwd": "cfg x w_ih w_hh b_ih b_hh out saved ws stream",
        "layer_bwd": "cfg d_out x out w_ih w_hh dx gw_ih gw_hh gb_ih gb_hh saved ws stream",
        "stack_fwd": "cfg x w_ih w_hh b_ih b_hh out saved ws rng add stream",
        "stack_bwd": "cfg d_out x out w_ih w_hh dx gw_ih gw_hh gb_ih gb_hh saved ws rng add stream"}
# family -> the entry point of each call (the packed ones take lengths behind cfg) and the family's dialogue limit
ENTRY = {"": dict(layer_fwd="ganffn_lstm_layer_fwd", layer_bwd="ganffn_lstm_layer_bwd", stack_fwd="ganffn_lstm_stack_fwd",
                  stack_bwd="ganffn_lstm_stack_bwd"),
         "batch": dict(layer_fwd="ganffn_lstm_batch_layer_fwd", layer_bwd="ganffn_lstm_batch_layer_bwd",
                       stack_fwd="ganffn_lstm_stack_batch_fwd", stack_bwd="ganffn_lstm_stack_batch_bwd"),
         "packed": dict(layer_fwd="ganffn_lstm_packed_layer_fwd", layer_bwd="ganffn_lstm_packed_layer_bwd",
                        stack_fwd="ganffn_lstm_stack_packed_fwd", stack_bwd="ganffn_lstm_stack_packed_bwd")}
MAX_B = {"": 32, "batch": 256, "packed": 256}
CALLS = [(fam, what) for fam in ENTRY for what in ARGS]
N_LAYERS = 2


def _cfg(what, S=5, B=3, In=12, H=8, L=N_LAYERS, p=0.5, train=0):
    from gan_ffn_amd import _lib
    return _lib.LstmCfg(S, B, In, H) if what.startswith("layer") else _lib.LstmStackCfg(S, B, In, H, L, p, train)


def _pointers(n=2 * N_LAYERS, **entries):
    """an array of n placeholder pointers ([L][2]; a layer call reads the first two), then entries {index: value}"""
    a = (C.c_void_p * n)(*[FAKE] * n)
    for i, v in entries.items():
        a[int(i)] = v
    return a


def _call(fam, what, over):
    """(return code, last error) of the family's entry point with placeholder arguments nothing is wrong with, then `over`"""
    from gan_ffn_amd import _lib
    lib = _lib.load()
    names = ARGS[what].split()
    if fam == "packed":
        names.insert(1, "lengths")
    a = {k: FAKE for k in names}
    a.update({k: _pointers() for k in "w_ih w_hh b_ih b_hh gw_ih gw_hh gb_ih gb_hh".split() if k in a})
    a.update(cfg=_cfg(what), add=C.c_uint64(0), stream=None)
    a.update(over)
    if a["cfg"] is not None:
        a["cfg"] = C.byref(a["cfg"])
    args = [a[k] for k in names]
    name = ENTRY[fam][what]
    assert len(args) == len(_lib.SIGNATURES[name][1]), name
    rc = getattr(lib, name)(*args)
    return int(rc), (lib.ganffn_last_error() or b"").decode()


def _refused(fam, what, piece, **over):
    rc, msg = _call(fam, what, over)
    assert rc == -1, (fam, what, rc, msg)
    assert piece in msg, (fam, what, msg)


@pytest.mark.parametrize("fam,what", CALLS)
def test_null_cfg(fam, what):
    _refused(fam, what, "null lstm cfg" if what.startswith("layer") else "null lstm stack cfg", cfg=None)


def test_size_functions_refuse_a_null_cfg():
    from gan_ffn_amd import _lib
    lib = _lib.load()
    for fn in LAYER_FNS + STACK_FNS:
        assert getattr(lib, fn)(None) == -1 and b"null lstm" in lib.ganffn_last_error(), fn


@pytest.mark.parametrize("fam,what", CALLS)
def test_dialogues_out_of_the_familys_range(fam, what):
    limit = MAX_B[fam]
    for B in (0, limit + 1, 257):
        _refused(fam, what, "lstm: S=5 B=%d (B <= %d per call)" % (B, limit), cfg=_cfg(what, B=B))
    _refused(fam, what, "lstm: S=0 B=3 (B <= %d per call)" % limit, cfg=_cfg(what, S=0))
    # the limit itself passes, and so do 33 dialogues behind the batch and packed entry points: the next refusal is another one
    for B in (limit, min(33, limit)):
        _refused(fam, what, "lstm_%s: null pointer" % what, cfg=_cfg(what, B=B), x=None)


@pytest.mark.parametrize("fam,what", CALLS)
def test_widths_must_be_multiples_of_4(fam, what):
    _refused(fam, what, "lstm: In=6 H=8 must be multiples of 4", cfg=_cfg(what, In=6))
    _refused(fam, what, "lstm: In=12 H=10 must be multiples of 4", cfg=_cfg(what, H=10))
    _refused(fam, what, "lstm: In=0 H=8 must be multiples of 4", cfg=_cfg(what, In=0), x=None)


@pytest.mark.parametrize("fam", list(ENTRY))
def test_stack_depth_and_dropout_out_of_range(fam):
    for what in ("stack_fwd", "stack_bwd"):
        for L in (0, 17, -1):
            _refused(fam, what, "lstm stack: L=%d (1 .. 16 layers)" % L, cfg=_cfg(what, L=L))
        _refused(fam, what, "lstm stack: dropout p=1 must be in [0, 1)", cfg=_cfg(what, p=1.0))
        _refused(fam, what, "lstm stack: dropout p=-0.5 must be in [0, 1)", cfg=_cfg(what, p=-0.5), x=None)
        # the depth is looked at before the dropout, the dropout before the dialogues
        _refused(fam, what, "lstm stack: L=17", cfg=_cfg(what, L=17, p=1.0, B=0))
        _refused(fam, what, "lstm stack: dropout p=1", cfg=_cfg(what, p=1.0, B=0))


@pytest.mark.parametrize("fam,what", CALLS)
def test_null_pointers(fam, what):
    fwd = what.endswith("fwd")
    for k in ("x w_ih w_hh b_ih b_hh out saved ws" if fwd else "d_out x out w_ih w_hh saved ws").split():
        _refused(fam, what, "lstm_%s: null pointer" % what, **{k: None})
    if not fwd:
        # dx and the gradient arrays may be null: the next refusal is another one
        _refused(fam, what, "buffers must be 16-byte aligned", dx=None, gw_ih=None, gw_hh=None, gb_ih=None, gb_hh=None, ws=ODD)


@pytest.mark.parametrize("fam,what", CALLS)
def test_misaligned_buffers(fam, what):
    # a stack call's buffers are looked at by the layer calls it makes: those of the layer it runs first (layer 0 forward, the
    # last layer backward) before any launch, and only those are tried here
    names = {"layer_fwd": "x out saved ws", "layer_bwd": "d_out x out saved ws dx", "stack_fwd": "x saved ws", "stack_bwd": "d_out out saved ws"}
    for k in names[what].split():
        _refused(fam, what, "lstm_layer_%s: buffers must be 16-byte aligned" % what[-3:], **{k: ODD})


@pytest.mark.parametrize("fam,what", [c for c in CALLS if c[1].endswith("fwd")])
def test_forward_weights_of_every_direction(fam, what):
    # the layer a call runs first: the only one of a layer call, layer 0 of a stack forward
    for d in (0, 1):
        for k in "w_ih w_hh b_ih b_hh".split():
            _refused(fam, what, "lstm_layer_fwd: direction %d: null / unaligned weights" % d, **{k: _pointers(**{str(d): None})})
        for k in "w_ih w_hh".split():
            _refused(fam, what, "lstm_layer_fwd: direction %d: null / unaligned weights" % d, **{k: _pointers(**{str(d): ODD})})


@pytest.mark.parametrize("fam,what", [c for c in CALLS if c[1].endswith("bwd")])
def test_backward_weights_of_every_direction(fam, what):
    """the backward reads w_ih[d] and w_hh[d] of both directions: a null or unaligned one is refused in the forward's words
    (before the drivers stated their refusals once, the backward went on to launch with it)"""
    first = 0 if what.startswith("layer") else 2 * (N_LAYERS - 1)         # a stack backward runs its last layer first
    for d in (0, 1):
        for k in "w_ih w_hh".split():
            for bad in (None, ODD):
                _refused(fam, what, "lstm_layer_bwd: direction %d: null / unaligned weights" % d, **{k: _pointers(**{str(first + d): bad})})


@pytest.mark.parametrize("fam", list(ENTRY))
def test_train_mode_with_layers_to_drop_between_needs_the_rng(fam):
    for what in ("stack_fwd", "stack_bwd"):
        _refused(fam, what, "lstm_%s: rng required in train mode" % what, cfg=_cfg(what, train=1), rng=None)
        # asked for after the pointers; not at all in eval mode, with p = 0 or with one layer: the next refusal is another one
        _refused(fam, what, "lstm_%s: null pointer" % what, cfg=_cfg(what, train=1), rng=None, x=None)
        for cfg in (_cfg(what, train=0), _cfg(what, train=1, p=0.0), _cfg(what, train=1, L=1)):
            _refused(fam, what, "buffers must be 16-byte aligned", cfg=cfg, rng=None, ws=ODD)


@pytest.mark.parametrize("what", list(ARGS))
def test_packed_entry_points_refuse_null_lengths_before_anything_else(what):
    name = "lstm_%s_packed_%s" % tuple(what.split("_")) if what.startswith("stack") else "lstm_packed_" + what
    _refused("packed", what, name + ": null lengths", lengths=None)
    _refused("packed", what, name + ": null lengths", lengths=None, cfg=None)


if __name__ == "__main__":
    with open(TABLE, "w") as f:
        json.dump(_table(), f, separators=(",", ":"))
        f.write("\n")
