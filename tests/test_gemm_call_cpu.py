"""The refusals and the workspace sizes of the GEMM driver (csrc/gemm.hip: check_gemm, gemm_plan's split rules, the grouped
weight-gradient launcher), without a GPU.

Refusals: every case below is refused before the first HIP call, so the entry points are called with placeholder pointers
(0x1000; 0x1004 where misalignment is the point).  The return code and the whole text of ganffn_last_error() are compared with
gemm_call_refusals.json.  Sizes: the three families of size functions that stand on the TN split rules, over a grid with shapes
on both sides of every threshold of those rules, against the same file.

The file was recorded from the library of the commit before the drivers got their one call descriptor (`PYTHONPATH=.
GANFFN_LIB=<that library> python tests/test_gemm_call_cpu.py` rewrites it; never from a library whose driver is under test).

Refusals of the driver that no entry point reaches, and why:
  * "gemm_nt: K=%d must be a multiple of 4", "gemm_nn: K=%d and N=%d ...", "gemm_tn: M=%d and N=%d ...", "gemm_tn_grouped: M, N
    must be multiples of 4": every entry point passes dense leading dimensions (lda = K, ldb = N, ...), or has refused such widths
    itself (encoder, head, LSTM and DialogueRNN cfg checks), so "gemm: leading dims must be multiples of 4" comes first;
  * "gemm_nt_pair: epilogue %d has no two-segment form", "gemm_nt_pair: bad second segment", "gemm_nt_pair: no two-segment form of
    the weight-resident kernel", "gemm_n100: bad second segment", "gemm_n100: no two-segment form of this variant": a second
    segment comes from ganffn_encoder_fwd_pair* only, whose own checks (ganffn_encoder_fwd_pair_supported) come first;
  * "gemm: unknown epilogue %d": ganffn_gemm_hook offers three epilogues and refuses the rest itself;
  * "gemm_tn: partial-slab workspace must be 16-byte aligned": ganffn_linear_bwd drops an unaligned workspace, the head and LSTM
    backward refuse one themselves;
  * "gemm_tn_grouped: n=%d out of [1,%d]": ganffn_gemm_tn_grouped refuses the same range in its own words first;
  * "gemm_tn_grouped: unreduced gradient slabs exist only for the d_model-100 kernel": slabs come from ganffn_encoder_bwd_parts*
    only, which refuses every stack but the d_model-100 one first."""
import ctypes as C
import json
import os

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_call_refusals.json")
FAKE = 0x1000          # a 16-byte aligned address nothing dereferences: the refusals come first
ODD = 0x1004           # and one that is not 16-byte aligned
BIG = 1 << 20          # x 1024 floats = 4 GiB


def _ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _nt(A=FAKE, W=FAKE, bias=FAKE, Cc=FAKE, M=64, N=64, K=64):
    return "ganffn_gemm_nt", [A, W, bias, Cc, M, N, K, None]


def _nn(A=FAKE, B=FAKE, Cc=FAKE, M=64, N=64, K=64):
    return "ganffn_gemm_nn", [A, B, Cc, M, N, K, None]


def _tn(At=FAKE, B=FAKE, Cc=FAKE, colsum=FAKE, M=64, N=64, K=64):
    return "ganffn_gemm_tn_acc", [At, B, Cc, colsum, M, N, K, None]


def _hook(mode=0, epi=0, A=FAKE, W=FAKE, bias=FAKE, aux=None, Cc=FAKE, stride=0, M=64, N=64, K=64, p=0.0, rng=FAKE, train=0, max_slabs=1):
    return "ganffn_gemm_hook", [mode, epi, A, W, bias, aux, Cc, stride, M, N, K, p, 0, rng, 0, train, max_slabs, None, None]


def _k100(which=0, a=FAKE, w=FAKE, bias=FAKE, out=FAKE, hmask=FAKE, h_saved=None, T=64, p=0.0, rng=FAKE, train=0):
    return "ganffn_ffn_k100_hook", [which, a, w, bias, out, hmask, h_saved, T, p, 0, rng, 0, train, None]


def _n100(A=FAKE, W=FAKE, kmajor=0, bias=FAKE, slabs=FAKE, stride=6400, T=64, K=2048, max_slabs=16, n_slabs=True):
    return "ganffn_gemm_n100", [A, W, kmajor, bias, slabs, stride, T, K, max_slabs, C.pointer(C.c_int(0)) if n_slabs else None, None]


def _grouped(n=1, At=(FAKE,), B=(FAKE,), Cc=(FAKE,), colsum=None, M=(64,), N=(64,), K=(1024,), ws=None, floats=0):
    return "ganffn_gemm_tn_grouped", [n, At and _ptrs(*At), B and _ptrs(*B), Cc and _ptrs(*Cc), colsum and _ptrs(*colsum),
                                      M and _ints(*M), N and _ints(*N), K and _ints(*K), ws, floats, None]


def _lin_fwd(x=FAKE, w=FAKE, b=FAKE, y=FAKE, T=64, K=64, N=64):
    return "ganffn_linear_fwd", [x, w, b, y, T, K, N, None]


def _lin_bwd(dy=FAKE, x=FAKE, w=FAKE, dx=FAKE, gw=FAKE, gb=FAKE, T=64, K=64, N=64, ws=None, floats=0):
    return "ganffn_linear_bwd", [dy, x, w, dx, gw, gb, T, K, N, ws, floats, None]


def _lin1(x=FAKE, w1=FAKE, b1=FAKE, h=FAKE, T=64, E=64, F=64, p=0.0, rng=FAKE, train=0):
    return "ganffn_ffn_linear1_fwd", [x, w1, b1, h, T, E, F, p, 0, rng, 0, train, None]


# name -> (entry point, arguments); the name says what is wrong with the call
CASES = {
    # check_common through the three plain entry points
    "nt null A": _nt(A=None), "nt null W": _nt(W=None), "nt null C": _nt(Cc=None),
    "nt M 0": _nt(M=0), "nt N 0": _nt(N=0), "nt K 0": _nt(K=0), "nt M negative": _nt(M=-64),
    "nt K 6": _nt(K=6), "nt A odd": _nt(A=ODD), "nt W odd": _nt(W=ODD),
    "nt A 4 GiB": _nt(M=BIG, K=1024), "nt W 4 GiB": _nt(N=BIG, K=1024), "nt just under 4 GiB, null C": _nt(M=BIG - 1, K=1024, Cc=None),
    "nn null A": _nn(A=None), "nn null B": _nn(B=None), "nn null C": _nn(Cc=None),
    "nn M 0": _nn(M=0), "nn K 6": _nn(K=6), "nn N 6": _nn(N=6), "nn A odd": _nn(A=ODD), "nn B odd": _nn(B=ODD),
    "nn A 4 GiB": _nn(M=BIG, K=1024), "nn B 4 GiB": _nn(K=BIG, N=1024),
    "tn null At": _tn(At=None), "tn null B": _tn(B=None), "tn null C": _tn(Cc=None),
    "tn K 0": _tn(K=0), "tn M 6": _tn(M=6), "tn N 6": _tn(N=6), "tn At odd": _tn(At=ODD), "tn B odd": _tn(B=ODD),
    "tn At 4 GiB": _tn(K=BIG, M=1024), "tn B 4 GiB": _tn(K=BIG, N=1024),
    # the K = 100 -> N >= 1024 shape (the weight-resident kernel's) and the short-K one are refused like any other
    "nt wres shape null A": _nt(A=None, M=70, N=1024, K=100), "nn wres shape B odd": _nn(B=ODD, M=70, N=1024, K=100),
    "nt short K A odd": _nt(A=ODD, M=70, N=64, K=128),
    # ganffn_gemm_hook: its own refusals, then check_gemm's
    "hook mode 2": _hook(mode=2), "hook epilogue 2": _hook(epi=2), "hook epilogue 6": _hook(epi=6),
    "hook mask without aux": _hook(epi=3), "hook dropout without rng": _hook(epi=1, p=0.5, train=1, rng=None),
    "hook null A": _hook(A=None), "hook nn W odd": _hook(mode=1, W=ODD), "hook slabs A odd": _hook(A=ODD, M=64, N=64, K=2048, max_slabs=8, stride=4096),
    "hook relu K 6": _hook(epi=1, K=6), "hook mask 4 GiB": _hook(mode=1, epi=3, aux=FAKE, M=BIG, K=1024),
    # ganffn_ffn_k100_hook
    "k100 which 2": _k100(which=2), "k100 null a": _k100(a=None), "k100 T 0": _k100(T=0), "k100 linear1 without bias": _k100(bias=None),
    "k100 dropout without rng": _k100(p=0.5, train=1, rng=None), "k100 dgrad without pattern": _k100(which=1, hmask=None),
    "k100 linear1 a odd": _k100(a=ODD), "k100 dgrad w odd": _k100(which=1, w=ODD), "k100 null out": _k100(out=None),
    # ganffn_gemm_n100 and the n100 launcher's refusals
    "n100 null n_slabs": _n100(n_slabs=False), "n100 max_slabs 0": _n100(max_slabs=0), "n100 max_slabs 17": _n100(max_slabs=17),
    "n100 K 100": _n100(K=100), "n100 K 272": _n100(K=272), "n100 null A": _n100(A=None), "n100 null W": _n100(W=None),
    "n100 null slabs": _n100(slabs=None), "n100 T 0": _n100(T=0), "n100 A odd": _n100(A=ODD), "n100 W odd": _n100(W=ODD),
    "n100 slabs odd": _n100(slabs=ODD), "n100 bias odd": _n100(bias=ODD), "n100 stride 6": _n100(stride=6),
    "n100 kmajor A odd": _n100(kmajor=1, A=ODD), "n100 A 4 GiB": _n100(T=BIG, K=1024), "n100 kmajor W 4 GiB": _n100(kmajor=1, K=10737440),
    # ganffn_gemm_tn_grouped
    "grouped n 0": _grouped(n=0), "grouped n 41": _grouped(n=41), "grouped null M": _grouped(M=None),
    "grouped null At": _grouped(At=(None,)), "grouped null C": _grouped(Cc=(None,)), "grouped K 0": _grouped(K=(0,)),
    "grouped M 6": _grouped(M=(6,)), "grouped B odd": _grouped(B=(ODD,)), "grouped 4 GiB": _grouped(K=(BIG,), M=(1024,)),
    "grouped second problem null B": _grouped(n=2, At=(FAKE, FAKE), B=(FAKE, None), Cc=(FAKE, FAKE), M=(64, 64), N=(64, 64), K=(512, 1024)),
    "grouped workspace odd": _grouped(ws=ODD, floats=1 << 24),
    "grouped 100-wide, workspace odd": _grouped(M=(100,), N=(2048,), K=(1024,), ws=ODD, floats=1 << 24),
    "grouped two K, workspace odd": _grouped(n=2, At=(FAKE, FAKE), B=(FAKE, FAKE), Cc=(FAKE, FAKE), M=(64, 128), N=(64, 64), K=(512, 1024),
                                             ws=ODD, floats=1 << 24),
    # the plain linear pair and linear1: their own refusals, then check_gemm's
    "linear_fwd null x": _lin_fwd(x=None), "linear_fwd T 0": _lin_fwd(T=0), "linear_fwd x 4 GiB": _lin_fwd(T=BIG, K=1024),
    "linear_bwd null dy": _lin_bwd(dy=None), "linear_bwd N 0": _lin_bwd(N=0), "linear_bwd dy 4 GiB": _lin_bwd(T=BIG, N=1024),
    "linear_bwd no dx, x 4 GiB": _lin_bwd(dx=None, T=BIG, K=1024, N=4),
    "linear1 null x": _lin1(x=None), "linear1 dropout without rng": _lin1(p=0.5, train=1, rng=None), "linear1 E 6": _lin1(E=6),
    "linear1 x odd": _lin1(x=ODD), "linear1 w 4 GiB": _lin1(F=BIG, E=1024),
}

# sizes: (T, K, N) of ganffn_linear_bwd_workspace_floats — the TN rule of a [N x K] gradient over T tokens: 768 / tiles splits,
# at most 16 and at most ceil(T / 64).  Tiles: 1, 2, 4, 48 | 49 and 51 | 52 (16 splits or 15), 64, 736 | 768 (2 splits or none)
GRID_T = (1, 64, 65, 128, 129, 960, 961, 1024, 1025, 3008)
GRID_KN = ((4, 4), (6, 4), (64, 64), (100, 64), (100, 100), (384, 512), (448, 448), (192, 1088), (832, 256), (512, 512), (2048, 100),
           (1472, 2048), (1536, 2048), (1540, 2048))
# (E, D1, D2) of the two heads (kind 0 generator, 1 discriminator: D2 <= 32)
GRID_HEAD = ((100, 64, 16), (512, 256, 32), (100, 100, 100), (300, 128, 32), (2048, 1024, 512), (6, 64, 16))


def _sizes(lib):
    from gan_ffn_amd import _lib
    linear = [[T, K, N, int(lib.ganffn_linear_bwd_workspace_floats(T, K, N))] for T in GRID_T for K, N in GRID_KN]
    head = [[T, E, D1, D2, kind, int(lib.ganffn_head_workspace_floats(C.byref(_lib.HeadCfg(T, E, D1, D2, kind, 0.2, 1))))]
            for T in GRID_T for E, D1, D2 in GRID_HEAD for kind in (0, 1)]
    return {"linear_bwd": linear, "head": head, "grouped": int(lib.ganffn_gemm_tn_grouped_workspace_floats())}


def _run(lib, name):
    fn, args = CASES[name]
    rc = getattr(lib, fn)(*args)
    return [int(rc), (lib.ganffn_last_error() or b"").decode()]


def _lib_loaded():
    from gan_ffn_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def want():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_covers_the_cases_and_every_one_is_a_refusal(want):
    assert sorted(want["refusals"]) == sorted(CASES)
    assert all(rc == -1 and msg for rc, msg in want["refusals"].values())
    # every text of the dense drivers that an entry point can reach is in the table
    texts = " | ".join(msg for _, msg in want["refusals"].values())
    for piece in ("gemm: null pointer", "gemm: bad shape", "gemm: leading dims", "gemm: operands must be 16-byte aligned",
                  "gemm_nt: an operand of 4 GiB", "gemm_nn: an operand of 4 GiB", "gemm_tn: an operand of 4 GiB",
                  "gemm_n100: bad arguments", "gemm_n100: operands must be 16-byte aligned", "gemm_n100: an operand of 4 GiB",
                  "gemm_n100: max_slabs", "gemm_n100: K=", "gemm_hook: mode", "gemm_hook: the mask epilogue", "gemm_hook: rng",
                  "ffn_k100_hook: bad arguments", "ffn_k100_hook: linear1 needs its bias", "ffn_k100_hook: rng", "ffn_k100_hook: the linear2 dgrad",
                  "gemm_tn_grouped: bad arguments", "gemm_tn_grouped: an operand of 4 GiB", "gemm_tn_grouped: partial-slab workspace"):
        assert piece in texts, piece


@pytest.mark.parametrize("name", list(CASES))
def test_refusal_equals_the_recorded_one(want, name):
    assert _run(_lib_loaded(), name) == want["refusals"][name]


def test_every_size_equals_the_recorded_table(want):
    got = _sizes(_lib_loaded())
    assert got["grouped"] == want["sizes"]["grouped"] > 0
    for k in ("linear_bwd", "head"):
        assert len(got[k]) == len(want["sizes"][k])
        for g, w in zip(got[k], want["sizes"][k]):
            assert g == w, (k, g, w)
    # the grid is not vacuous: shapes that split and shapes that do not, the 16-split cap and the 15 beside it, and widths the
    # MFMA path does not take (0) or the head refuses (-1)
    lin = {tuple(r[:3]): r[3] for r in want["sizes"]["linear_bwd"]}
    assert lin[(3008, 448, 448)] == 16 * (448 * 448 + 448) and lin[(3008, 192, 1088)] == 16 * (1088 * 192 + 1088)
    assert lin[(3008, 832, 256)] == 15 * (256 * 832 + 256)
    assert lin[(3008, 1472, 2048)] == 2 * (2048 * 1472 + 2048) and lin[(3008, 1536, 2048)] == 0 and lin[(3008, 1540, 2048)] == 0
    assert lin[(64, 64, 64)] == 0 and lin[(65, 64, 64)] == 2 * (64 * 64 + 64) and lin[(1024, 64, 64)] == lin[(1025, 64, 64)] == 16 * (64 * 64 + 64)
    assert lin[(3008, 6, 4)] == 0
    heads = [r[5] for r in want["sizes"]["head"]]
    assert -1 in heads and any(h > 0 for h in heads)


if __name__ == "__main__":
    lib = _lib_loaded()
    with open(TABLE, "w") as f:
        json.dump({"refusals": {name: _run(lib, name) for name in CASES}, "sizes": _sizes(lib)}, f, indent=0, sort_keys=True)
        f.write("\n")
