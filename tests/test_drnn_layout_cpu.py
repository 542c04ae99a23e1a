"""The ten DialogueRNN size functions of csrc/dialogue_rnn.hip (drnn_layout behind five entry-point families), without a GPU.

Every value over the grid below is held against the table in drnn_layout_sizes.json, which was recorded from the library of the
commit before the layout sized its shared step regions for the wider cell (`PYTHONPATH=. GANFFN_LIB=<that library> python
tests/test_drnn_layout_cpu.py` rewrites it; never from a library whose layout code is under test).  DialogueRNNFn and DrnnEngine
size their buffers from these functions, so a layout that moves shows here first.

What may differ from the table, and by how much: with D_e > 128 the emotion cell runs per step and takes GI and GH as
[B x 3 D_e] and dhdir as [B x D_e]; the recorded layout gave those regions B*3*D_g, B*3*D_g and B*D_g floats, so for
D_e > max(D_g, 128) the workspace has to be at least 3 B (D_e - D_g) + 3 B (D_e - D_g) + B (D_e - D_g) = 7 B (D_e - D_g) floats
larger than recorded.  The saved block and every configuration with D_e <= D_g or D_e <= 128 are equal to the table.

The grid: S = 1, a few steps and DR_MAXS = 112; B at 1, 3, both sides of the 32-dialogue limit of the families other than batch,
and GANFFN_MAX_DIALOGUES; the widths are the narrowest the checks accept, both sides of D_e = 128 against D_g, configuration 5's,
and D_g = 512; every attention type with its own regions (dot only where D_m == D_g; concat at both ends of D_a); listener on and
off; 1, 2 and 16 parties."""
import ctypes as C
import json
import os

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "drnn_layout_sizes.json")
GRID_S, GRID_B, GRID_P = (1, 5, 112), (1, 3, 32, 33, 256), (1, 2, 16)
GRID_W = ((4, 4, 4), (8, 136, 132), (8, 64, 132), (100, 500, 100), (8, 512, 4))          # (D_m, D_g = D_p, D_e)
GRID_ATT = (("general", 0), ("dot", 0), ("general2", 0), ("concat", 4), ("concat", 512))   # dot: only where D_m == D_g
# cfgs every function refuses, (S, B, D_m, D_g, D_e): B past every family's limit, D_g past 512, S past DR_MAXS
REFUSED = ((5, 257, 8, 64, 4), (5, 3, 8, 516, 4), (113, 3, 8, 64, 4))
FN_FAMILY = [fam for fam in ("", "listener_", "att_", "party_", "batch_") for _ in range(2)]
FNS = ["ganffn_drnn_%s%s_floats" % (fam, what) for fam, what in zip(FN_FAMILY, ("saved", "workspace") * 5)]
COLS = ["S", "B", "D_m", "D_g", "D_e", "att", "D_a", "listener", "parties"]
N_KEY = len(COLS)
EC_MAXHE = 128          # the widest emotion cell the chain kernels take (dialogue_rnn.hip)


def _grid():
    rows = [(S, B, Dm, H, He, att, Da, lis, P) for S in GRID_S for B in GRID_B for Dm, H, He in GRID_W for att, Da in GRID_ATT
            if att != "dot" or Dm == H for lis in (0, 1) for P in GRID_P]
    return rows + [(S, B, Dm, H, He, "general", 0, 0, 2) for S, B, Dm, H, He in REFUSED]


def _table():
    """[[S, B, D_m, D_g, D_e, att, D_a, listener, parties, <FNS>]] of the loaded library"""
    from gan_ffn_amd import _lib
    lib = _lib.load()
    out = []
    for S, B, Dm, H, He, att, Da, lis, P in _grid():
        c = C.byref(_lib.DrnnCfg(S, B, Dm, H, He, 0.5, 1))
        a = C.byref(_lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], Da))
        args = {"": (c,), "listener_": (c,), "att_": (c, a, lis), "party_": (c, a, lis, P), "batch_": (c, a, lis, P)}
        out.append([S, B, Dm, H, He, att, Da, lis, P] + [int(getattr(lib, fn)(*args[fam])) for fn, fam in zip(FNS, FN_FAMILY)])
    return out


def _recorded():
    with open(TABLE) as f:
        return json.load(f)


def test_every_size_is_the_recorded_one_or_larger_by_the_shared_regions():
    want, got = _recorded(), _table()
    n_att = sum(len(GRID_ATT) - (0 if Dm == H else 1) for Dm, H, _ in GRID_W)
    assert len(got) == len(GRID_S) * len(GRID_B) * n_att * 2 * len(GRID_P) + len(REFUSED) == len(want)
    n_equal = n_wider = 0
    for g, w in zip(got, want):
        assert g[:N_KEY] == w[:N_KEY]
        S, B, Dm, H, He = g[:5]
        tag = dict(zip(COLS + FNS, zip(g, w)))
        if He <= H or He <= EC_MAXHE:
            assert g == w, tag
            n_equal += 1
            continue
        n_wider += 1
        for fn, gv, wv in zip(FNS, g[N_KEY:], w[N_KEY:]):
            if wv < 0 or fn.endswith("saved_floats"):
                assert gv == wv, (fn, tag)
            else:
                assert gv >= wv + 7 * B * (He - H), (fn, tag)
    assert n_equal > 0 and n_wider > 0


def test_the_recorded_table_is_not_vacuous():
    want = _recorded()
    grid, refused = want[:-len(REFUSED)], want[-len(REFUSED):]
    k = {fn[len("ganffn_drnn_"):-len("_floats")]: N_KEY + i for i, fn in enumerate(FNS)}
    for r in grid:
        S, B, Dm, H, He, att, Da, lis, P = r[:N_KEY]
        # 33 and 256 dialogues only behind the batch family; up to 32 every family answers
        assert all((r[k[f]] > 0) == (B <= 32) for f in k if not f.startswith("batch")), r
        assert r[k["batch_saved"]] > 0 and r[k["batch_workspace"]] > 0, r
        if B <= 32:
            # the party family is the batch family, the att family its two-party case, the two without a descriptor the
            # general-attention case of that
            assert (r[k["party_saved"]], r[k["party_workspace"]]) == (r[k["batch_saved"]], r[k["batch_workspace"]]), r
            if P == 2:
                assert (r[k["att_saved"]], r[k["att_workspace"]]) == (r[k["party_saved"]], r[k["party_workspace"]]), r
                if att == "general":
                    fam = "listener_" if lis else ""
                    assert (r[k[fam + "saved"]], r[k[fam + "workspace"]]) == (r[k["att_saved"]], r[k["att_workspace"]]), r
    assert any(r[1] > 32 for r in grid) and any(r[4] > max(r[3], EC_MAXHE) for r in grid) and any(r[5] == "dot" for r in grid)
    # B past every family's limit, D_g = 516 and S = 113: refused by all ten
    assert [tuple(r[:5]) for r in refused] == list(REFUSED)
    assert all(r[N_KEY:] == [-1] * len(FNS) for r in refused)


def test_refused_configurations_return_minus_one():
    got = _table()
    for r in got[-len(REFUSED):]:
        assert r[N_KEY:] == [-1] * len(FNS), r
    for r in got[:-len(REFUSED)]:
        if r[1] > 32:         # past the 32-dialogue families' limit; the batch family answers
            assert r[N_KEY:N_KEY + 8] == [-1] * 8 and r[N_KEY + 8] > 0 and r[N_KEY + 9] > 0, r


if __name__ == "__main__":
    with open(TABLE, "w") as f:
        json.dump(_table(), f, separators=(",", ":"))
        f.write("\n")
