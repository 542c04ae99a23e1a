"""The refusals of the row-stage driver (csrc/elementwise.hip: check_row_fwd / check_row_bwd behind row_fwd / row_bwd) that an
entry point reaches, without a GPU.

Every case below is refused before the first HIP call, so ganffn_add_dropout_layernorm_fwd / _bwd are called with placeholder
pointers (0x1000).  The return code and the whole text of ganffn_last_error() are compared with row_call_refusals.json.

The file was recorded from the library of the commit before the row stages got their one call descriptor (`PYTHONPATH=.
GANFFN_LIB=<that library> python tests/test_row_call_cpu.py` rewrites it; never from a library whose driver is under test).

Refusals of the driver that no entry point reaches, and why:
  * "rc_pe_inproj_fwd: ...", "rc_outproj_ln_fwd: ...", "rc_ln_inproj_fwd: ...", "rc_ln_bwd: ..." (bad arguments, bad second segment,
    alignment, the in-proj's and the two dgrads' operands) and "...: no rowchain kernel has a GEMM on both sides": the rowchain plan is
    chosen by the encoder walks only (ganffn_encoder_fwd* / _bwd*), whose check_pass has refused null and unaligned buffers, and
    every operand of a stage is an offset of a multiple of 4 floats into one of them; the two LayerNorm entry points run under the
    separate-launch plan at every width;
  * "layernorm: bad second segment", "pe_dropout: bad arguments", "pe_dropout: bad second segment", "row stage: ...": a second
    segment and a positional-encoding stage come from the encoder walks only, which build both segments from checked buffers;
  * "layernorm: nslab=%d out of [1,%d]": the entry points pass one slab, the walks pass the count gemm() reported under a cap of 16;
  * "layernorm: bad arguments": the entry points refuse the same operands in their own words first;
  * "layernorm: the in-proj and out-proj dgrads run inside the rowchain kernels only", "layernorm: reduce list is full": the walk
    names those operands under the rowchain plan only, and appends two records per layer of at most 64 to a list of 128."""
import ctypes as C
import json
import os

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_call_refusals.json")
FAKE = 0x1000          # a 16-byte aligned address nothing dereferences: the refusals come first


def _fwd(x=FAKE, y=FAKE, w=FAKE, b=FAKE, out=FAKE, xhat=FAKE, rstd=FAKE, T=8, E=64, p=0.0, rng=FAKE):
    return "ganffn_add_dropout_layernorm_fwd", [x, y, w, b, out, xhat, rstd, T, E, 1e-5, p, 3, rng, 0, None]


def _bwd(d_out=FAKE, xhat=FAKE, rstd=FAKE, w=FAKE, dz=FAKE, dy=FAKE, gw=FAKE, gb=FAKE, T=8, E=64, p=0.0, rng=FAKE):
    return "ganffn_add_dropout_layernorm_bwd", [d_out, xhat, rstd, w, dz, dy, gw, gb, T, E, p, 3, rng, 0, None]


# name -> (entry point, arguments); the name says what is wrong with the call
CASES = {
    "fwd null x": _fwd(x=None), "fwd null y": _fwd(y=None), "fwd null w": _fwd(w=None), "fwd null b": _fwd(b=None),
    "fwd null out": _fwd(out=None), "fwd T 0": _fwd(T=0), "fwd T negative": _fwd(T=-8), "fwd E 0": _fwd(E=0),
    "fwd E 644": _fwd(E=644), "fwd E 644, one row": _fwd(E=644, T=1), "fwd dropout without rng": _fwd(p=0.5, rng=None),
    "fwd E 644, dropout without rng": _fwd(E=644, p=0.5, rng=None), "fwd null x, E 644": _fwd(x=None, E=644),
    "bwd null d_out": _bwd(d_out=None), "bwd null xhat": _bwd(xhat=None), "bwd null rstd": _bwd(rstd=None), "bwd null w": _bwd(w=None),
    "bwd null dz": _bwd(dz=None), "bwd T 0": _bwd(T=0), "bwd E 0": _bwd(E=0), "bwd E 644": _bwd(E=644),
    "bwd E 644, no parameter gradients": _bwd(E=644, gw=None, gb=None), "bwd dropout without rng": _bwd(p=0.5, rng=None),
    "bwd E 644, dropout without rng": _bwd(E=644, p=0.5, rng=None), "bwd null dz, E 644": _bwd(dz=None, E=644),
}


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
    # every text of the row-stage driver that an entry point can reach is in the table, beside the entry points' own
    texts = " | ".join(msg for _, msg in want["refusals"].values())
    for piece in ("layernorm: E=644 > 640", "add_dropout_layernorm_fwd: bad arguments", "add_dropout_layernorm_fwd: rng required",
                  "add_dropout_layernorm_bwd: bad arguments", "add_dropout_layernorm_bwd: rng required"):
        assert piece in texts, piece


@pytest.mark.parametrize("name", list(CASES))
def test_refusal_equals_the_recorded_one(want, name):
    assert _run(_lib_loaded(), name) == want["refusals"][name]


if __name__ == "__main__":
    lib = _lib_loaded()
    with open(TABLE, "w") as f:
        json.dump({"refusals": {name: _run(lib, name) for name in CASES}}, f, indent=0, sort_keys=True)
        f.write("\n")
